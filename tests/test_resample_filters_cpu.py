"""CPU: the selectable Pillow resampling filters (BILINEAR, BOX, HAMMING, LANCZOS beside the
default BICUBIC; csrc/resize.hpp) through the host twin of the kernels' coefficient code,
dino_resample_coeffs_host: its taps applied in Pillow's order reproduce Image.resize bit for
bit, every tap fits the 24-bit multiply and the digit planes of the fast paths, filter 0 is
the bicubic there always was, the scaled workspace bound covers every filter's true scratch,
and MI355XBackend's resample_filter option resolves to the filter each pipeline gets."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
from PIL import Image

from dataloader_amd import _lib, fallback
from dataloader_amd.params import (OUT_FP32, RESAMPLE_FILTERS, VIEW_PARAMS_DTYPE, make_aug_config,
                                   resample_bound_scale, resample_filter_code)
from tests.helpers import dec_scratch, emu_resized_crop, view_scratch

PRECISION_BITS = 22
P = ctypes.c_void_p
NEW_FILTERS = ("bilinear", "box", "hamming", "lanczos")
PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "box": Image.BOX, "hamming": Image.HAMMING,
              "lanczos": Image.LANCZOS}


def ksize_of(lib, f: int, n_in: int, n_out: int) -> int:
    k = ctypes.c_int32(0)
    _lib.check(lib.dino_resample_coeffs_host(f, n_in, n_out, 0, 0, ctypes.byref(k), None, None), "coeffs_host")
    return int(k.value)


def host_coeffs(lib, f: int, n_in: int, n_out: int, x0: int = 0, n: int | None = None):
    """(bounds[n, 2], taps[n, ksize]) of the outputs x0 .. x0 + n - 1 from the library's host code."""
    n = n_out - x0 if n is None else n
    k = ksize_of(lib, f, n_in, n_out)
    bounds = np.zeros((n, 2), np.int32)
    taps = np.zeros((n, k), np.int32)
    kk = ctypes.c_int32(0)
    _lib.check(lib.dino_resample_coeffs_host(f, n_in, n_out, x0, n, ctypes.byref(kk), bounds.ctypes.data_as(P),
                                             taps.ctypes.data_as(P)), "coeffs_host")
    assert kk.value == k
    return bounds, taps


def resample_with_host_taps(lib, f: int, rgb: np.ndarray, ow: int, oh: int) -> np.ndarray:
    """rgb resampled to ow x oh as Pillow does it: the horizontal pass, then the vertical one,
    each only when that side changes; int32 sums from 2^21, shift by 22, clip."""
    def one_pass(src, n_out):  # along axis 1
        n_in = src.shape[1]
        if n_in == n_out:
            return src
        b, k = host_coeffs(lib, f, n_in, n_out)
        out = np.empty((src.shape[0], n_out, 3), np.uint8)
        for x in range(n_out):
            x0, cnt = int(b[x, 0]), int(b[x, 1])
            acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, x0:x0 + cnt].astype(np.int64),
                                                             k[x, :cnt].astype(np.int64), axes=([1], [0]))
            assert np.abs(acc).max() < 2 ** 31
            out[:, x] = np.clip(acc >> PRECISION_BITS, 0, 255)
        return out

    tmp = one_pass(rgb, ow)
    return one_pass(tmp.transpose(1, 0, 2), oh).transpose(1, 0, 2)


SHAPES = [(37, 5, 16), (9, 90, 32), (200, 131, 30), (3, 2, 12), (1, 1, 8)]
# BOX at exact ratios: pixel centres fall exactly on the filter's (asymmetric) bounds
BOX_SHAPES = [(32, 24, 16, 12), (48, 27, 16, 9), (8, 6, 16, 12), (30, 30, 10, 15)]


@pytest.mark.parametrize("name", NEW_FILTERS)
def test_host_taps_reproduce_pillow(name):
    lib = _lib.load()
    f = RESAMPLE_FILTERS[name]
    rng = np.random.default_rng(40 + f)
    shapes = [(W, H, S, S) for W, H, S in SHAPES] + (BOX_SHAPES if name == "box" else [])
    for W, H, ow, oh in shapes:
        for rgb in (rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8),
                    rng.integers(0, 2, size=(H, W, 3), dtype=np.uint8) * 255):  # (sums that leave [0, 255])
            ref = np.asarray(Image.fromarray(rgb, "RGB").resize((ow, oh), PIL_FILTER[name]))
            got = resample_with_host_taps(lib, f, rgb, ow, oh)
            assert np.array_equal(ref, got), (name, W, H, ow, oh, int((ref != got).sum()))


def test_filter_zero_is_the_emulators_bicubic(emu):
    """Filter 0 through the new host entry: the tap counts and the pixels of the emulator (the
    kernels' own code called with the signatures it always had)."""
    lib = _lib.load()
    rng = np.random.default_rng(5)
    for W, H, S in SHAPES[:4]:
        assert ksize_of(lib, 0, W, S) == emu.emu_resample_ksize(W, S)
        assert ksize_of(lib, 0, H, S) == emu.emu_resample_ksize(H, S)
        rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        rec = np.zeros((), VIEW_PARAMS_DTYPE)
        rec["out_size"], rec["crop_w"], rec["crop_h"] = S, W, H
        assert np.array_equal(resample_with_host_taps(lib, 0, rgb, S, S), emu_resized_crop(emu, rgb, rec)), (W, H, S)
        assert np.array_equal(resample_with_host_taps(lib, 0, rgb, S, S),
                              np.asarray(Image.fromarray(rgb, "RGB").resize((S, S), Image.BICUBIC)))


def test_host_entry_rejects_bad_arguments():
    lib = _lib.load()
    k = ctypes.c_int32(0)
    for f in (-1, 5, 99):
        assert lib.dino_resample_coeffs_host(f, 10, 5, 0, 0, ctypes.byref(k), None, None) != 0
        assert b"unknown filter" in lib.dino_last_error()
    b, t = np.zeros(2, np.int32), np.zeros(64, np.int32)
    assert lib.dino_resample_coeffs_host(1, 10, 5, 4, 2, ctypes.byref(k), b.ctypes.data_as(P), t.ctypes.data_as(P)) != 0
    assert lib.dino_resample_coeffs_host(1, 0, 5, 0, 0, ctypes.byref(k), None, None) != 0
    for name, code in RESAMPLE_FILTERS.items():
        assert resample_filter_code(name) == resample_filter_code(code) == code
    assert resample_filter_code(None) == 0
    for bad in ("nearest", "", 5, -1, 1.5, True):
        with pytest.raises(ValueError):
            resample_filter_code(bad)


def _segments(out_size: int, every: bool):
    """(x0, n) ranges of the output positions swept: all of them for small outputs, else both
    edges and 32 interior positions (tests/test_rcoeffs_range_cpu.py _positions)."""
    if every or out_size <= 64:
        return [(0, out_size)]
    mid = np.unique(np.linspace(16, out_size - 17, 32).astype(np.int64))
    return [(0, 16)] + [(int(m), 1) for m in mid] + [(out_size - 16, 16)]


def _sweep_pairs():
    outs_all = list(range(1, 41)) + [96, 128, 224, 518, 1024]
    pairs = []
    for i in range(1, 321):  # small inputs: every position, every small output and the view sizes
        pairs += [(i, o, True) for o in outs_all if o <= 40 or i <= 64 or i % 16 == 1]
    big_in = [321, 480, 500, 640, 767, 1023, 1024, 1025, 1600, 2047, 4001, 4096, 9999, 16384, 32768, 65535]
    for i in big_in:  # large inputs: edges and a spread of interior phases
        pairs += [(i, o, False) for o in (1, 2, 3, 7, 30, 32, 96, 224, 518, 1023, 1024)]
    for o in (30, 32, 96, 224, 1024):  # scales just off 1 and just off small integers
        pairs += [(o + d, o, False) for d in (-3, -2, -1, 1, 2, 3) if o + d > 0]
        pairs += [(m * o + d, o, False) for m in (2, 3, 4) for d in (-1, 0, 1)]
    return pairs


@pytest.mark.parametrize("name", NEW_FILTERS)
def test_every_tap_fits_the_fast_paths(name):
    """The sweep of tests/test_rcoeffs_range_cpu.py over the library's own coefficient code for
    each new filter: |k| < 2^23 (tap_mad's 24-bit multiply), k inside the three signed base-256
    digit planes of k_rcoeffs ([-2^23 - 2^15, 2^23 - 2^15)), and 255 sum|k| + 2^21 inside int32
    (no partial sum of a pass overflows in any order).  Prints where the maxima lie."""
    lib = _lib.load()
    f = RESAMPLE_FILTERS[name]
    pairs = _sweep_pairs()
    worst_k, worst_s = (0, None), (0, None)
    for i, o, every in pairs:
        for x0, n in _segments(o, every):
            _, k = host_coeffs(lib, f, i, o, x0, n)
            a = np.abs(k.astype(np.int64))
            m, s = a.max(axis=1), a.sum(axis=1)
            if int(m.max()) > worst_k[0]:
                worst_k = (int(m.max()), (i, o, x0 + int(m.argmax())))
            if int(s.max()) > worst_s[0]:
                worst_s = (int(s.max()), (i, o, x0 + int(s.argmax())))
            assert int(k.min()) >= -(1 << 23) - (1 << 15), (i, o, x0)
    one = 1 << PRECISION_BITS
    print(f"{name}: largest |k| = {worst_k[0]} = {worst_k[0] / one:.4f} x 2^22 at (in, out, position) = {worst_k[1]}; "
          f"largest sum|k| = {worst_s[0]} = {worst_s[0] / one:.4f} x 2^22 at {worst_s[1]}; {len(pairs)} size pairs")
    assert worst_k[0] >= one  # (the sweep reaches weight 1.0)
    assert worst_k[0] < (1 << 23) - (1 << 15), worst_k
    assert 255 * worst_s[0] + (1 << (PRECISION_BITS - 1)) < 2 ** 31, worst_s
    if name != "lanczos":  # non-negative filters: a normalised weight is at most 1, and the taps
        # of an output sum to 1 plus at most half a unit of rounding each (<= 2 x 65535 + 3 taps)
        assert worst_k[0] == one and worst_s[0] <= one + 65537, (worst_k, worst_s)


@pytest.mark.parametrize("name", ("bicubic",) + NEW_FILTERS)
@pytest.mark.parametrize("S", (30, 96, 224))
def test_scaled_bound_covers_the_filters_scratch(emu, name, S):
    """The workspace bound for a filter is the probes' (bicubic) bound times
    resample_bound_scale, as IngestEngine.reserve applies it.  It is at least the scratch that
    the kernels lay out (plan.hpp view_scratch) with the filter's true tap counts, for every
    crop of the image; the same for the decode-only recipe's bound."""
    from dataloader_amd.config import DINOAugConfig
    from dataloader_amd.pipeline import resize_scratch_bound
    lib = _lib.load()
    f = RESAMPLE_FILTERS[name]
    scale = resample_bound_scale(name)
    assert scale == (2 if name == "lanczos" else 1)
    cfg = make_aug_config(DINOAugConfig(global_crop_size=S, local_crop_size=S, n_global_crops=1, n_local_crops=0),
                          S, S, OUT_FP32)
    sides = (1, 7, S, 8 * S + 1, 2048)
    for W in sides:
        for H in sides:
            bound = scale * fallback.augment_need(np.array([[0, W, H, 3]], np.int32), cfg)
            for cw in (c for c in sides if c <= W):
                for ch in (c for c in sides if c <= H):
                    kh = 0 if cw == S else ksize_of(lib, f, cw, S)
                    kv = 0 if ch == S else ksize_of(lib, f, ch, S)
                    need = view_scratch(emu, S, ch, kh, kv)["total"]
                    assert need <= bound, (name, S, W, H, cw, ch, need, bound)
            kh = 0 if W == S else ksize_of(lib, f, W, S)
            for oh in (S, 2 * S + 1):
                kv = 0 if H == oh else ksize_of(lib, f, H, oh)
                need = dec_scratch(emu, S, oh, H, kh, kv)["total"]
                assert need <= scale * resize_scratch_bound(W, H, S, oh), (name, S, W, H, oh)


class _StubPipeline:
    def __init__(self, *args, **kwargs):
        self.kwargs = kwargs


class _Source:
    _batch_size = 4


def test_backend_resample_filter_option(monkeypatch):
    """What MI355XBackend hands each pipeline (which sets it on its engines): None is bicubic
    everywhere, a name applies to every recipe, "spec" follows EvalAugSpec.interpolation and is
    bicubic for the other specs; an unknown name is a ValueError at construction."""
    from dataloader_amd import backend, pipeline
    from dataloader_amd.config import (DinoV2AugSpec, EvalAugSpec, LeJEPAAugSpec, PipelineConfig, UserAugSpec)
    monkeypatch.setattr(backend, "MI355XAugPipeline", _StubPipeline)
    monkeypatch.setattr(pipeline, "MI355XUserAugPipeline", _StubPipeline)
    pc = PipelineConfig(fuse_normalization=False)
    specs = [DinoV2AugSpec(), LeJEPAAugSpec(), EvalAugSpec(), EvalAugSpec(interpolation="bilinear"),
             UserAugSpec(aug_fn=lambda x: {"x": x}, _output_map=["x"], warn_not_dali=False)]

    def built(be):
        return [be.build_pipeline(_Source(), s, pc).kwargs["resample_filter"] for s in specs]

    assert built(backend.MI355XBackend()) == [None] * 5
    assert built(backend.MI355XBackend(resample_filter=None)) == [None] * 5
    for name in RESAMPLE_FILTERS:
        assert built(backend.MI355XBackend(resample_filter=name)) == [name] * 5
        assert resample_filter_code(name) == RESAMPLE_FILTERS[name]
    assert built(backend.MI355XBackend(resample_filter="spec")) == [None, None, "bicubic", "bilinear", None]
    assert resample_filter_code(None) == RESAMPLE_FILTERS["bicubic"] == 0
    for bad in ("nearest", "cubic", "", 1, "SPEC "):
        with pytest.raises(ValueError):
            backend.MI355XBackend(resample_filter=bad)
    with pytest.raises(ValueError):  # a spec naming a filter Pillow's family does not have
        backend.MI355XBackend(resample_filter="spec").build_pipeline(_Source(), EvalAugSpec(interpolation="area"), pc)

"""GPU: the selectable Pillow resampling filters (dino_ctx_set_resample_filter: BILINEAR, BOX,
HAMMING, LANCZOS) against Pillow itself, bit for bit: Image.fromarray(rgb).crop(box).resize(
(w, h), Image.<FILTER>), then oracle.cpu_ref.to_tensor_normalized.  Inputs are raw RGB
containers, so the pixels are exact; view records are explicit with the colour ops off unless
a test says otherwise."""

from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

from dataloader_amd import _lib, fallback
from dataloader_amd.config import DINOAugConfig
from dataloader_amd.engine import IngestEngine, pack_jpegs, params_from_device, params_to_device
from dataloader_amd.params import OUT_FP32, RESAMPLE_FILTERS, make_aug_config
from dataloader_amd.pipeline import resize_scratch_bound
from oracle import cpu_ref
from tests.helpers import params_to_record, record_to_params

pytestmark = pytest.mark.gpu

NEW_FILTERS = ("bilinear", "box", "hamming", "lanczos")
PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "box": Image.BOX, "hamming": Image.HAMMING,
              "lanczos": Image.LANCZOS}
GOLDEN = Path(__file__).resolve().parent / "golden"
MEAN, STD = DINOAugConfig().mean, DINOAugConfig().std


def _engine_for(gpu_device, images, S, nv, name):
    """Raw containers of the images decoded into an engine with filter `name`, its workspaces
    sized by the probe (IngestEngine.reserve scales the augment bound to the filter)."""
    B = len(images)
    cfg = DINOAugConfig(global_crop_size=S, local_crop_size=S, n_global_crops=nv, n_local_crops=0)
    eng = IngestEngine(gpu_device, max_batch=B, max_views=nv, max_crop_size=S)
    eng.set_resample_filter(name)
    buf, off = pack_jpegs([fallback.raw_container(im) for im in images], pin=False)
    raw = np.ones(B, np.uint8)
    pinfo, ws, aws = fallback.probe(buf.data_ptr(), off.numpy(), B, 0, make_aug_config(cfg, S, S, OUT_FP32), raw)
    assert (pinfo[:, 0] == 0).all(), pinfo
    eng.reserve(ws, aws)
    info = eng.decode(buf.to(gpu_device), off.to(gpu_device), B, raw_mask=torch.from_numpy(raw).to(gpu_device))
    assert (info.cpu().numpy()[:, 0] == 0).all()
    return eng, cfg


def _augment(eng, cfg, S, records, device):
    recs = np.stack([params_to_record(p) for slot in records for p in slot])
    views = eng.augment(make_aug_config(cfg, S, S, OUT_FP32), params_to_device(recs, device))
    torch.cuda.synchronize()
    info = eng.batch_info(torch.empty(len(records), 4, dtype=torch.int32, device=device)).cpu().numpy()
    assert (info[:, 0] == 0).all(), info  # (no view left out for want of scratch)
    return [v.cpu() for v in views]


def _pillow_view(im: np.ndarray, p, name: str) -> torch.Tensor:
    img = Image.fromarray(im, "RGB").crop((p.crop_left, p.crop_top, p.crop_left + p.crop_w, p.crop_top + p.crop_h))
    img = img.resize((p.out_size, p.out_size), PIL_FILTER[name])
    if p.flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return cpu_ref.to_tensor_normalized(img, MEAN, STD, torch.float32)


def _check(images, records, views, name, what):
    bad = []
    for b, im in enumerate(images):
        for v, p in enumerate(records[b]):
            ref = _pillow_view(im, p, name)
            if not torch.equal(ref, views[v][b]):
                d = (ref - views[v][b]).abs()
                bad.append((b, p.crop_w, p.crop_h, p.flip, int((d > 0).sum()), float(d.max())))
    assert not bad, f"{what} {name}: views differ (image, cw, ch, flip, values, max): {bad}"


def _images(shapes, seed):
    """Per shape: uniform noise in the top half, 0 / 255 bits below (sums that leave [0, 255])."""
    rng = np.random.default_rng(seed)
    out = []
    for w, h in shapes:
        im = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        im[h // 2:] = rng.integers(0, 2, size=(h - h // 2, w, 3), dtype=np.uint8) * 255
        out.append(im)
    return out


@pytest.mark.parametrize("S", [30, 96, 132])
@pytest.mark.parametrize("name", NEW_FILTERS)
def test_views_match_pillow(gpu_device, name, S):
    """The fused vertical kernel (S = 30 scalar, 96 by words) and k_vert + k_final (132), from
    a 200 x 131 image: upscale 7 x 5, mild downscale 131 x 131, the whole image (strong
    downscale at S = 30), 1 x 1, crop_w == S (no horizontal pass) and crop_h == S (no vertical
    pass; at S = 132 that crop comes from the batch's second image, 140 x 150, which the first
    is too low for, and which takes the other crops too).  Every third view is flipped."""
    images = _images([(200, 131), (140, 150)], 100 + S)
    records = []
    for im in images:
        H, W, _ = im.shape
        crops = [(7, 5), (131, 131), (W, H), (1, 1), (S, min(50, H)), (50, S if S <= H else H)]
        records.append([cpu_ref.ViewParams(out_size=S, crop_top=(H - ch) if k & 1 else 0,
                                           crop_left=(W - cw) if k & 2 else 0, crop_h=ch, crop_w=cw, flip=k % 3 == 1)
                        for k, (cw, ch) in enumerate(crops)])
    assert any(p.crop_h == S for slot in records for p in slot) and any(p.crop_w == S for slot in records for p in slot)
    eng, cfg = _engine_for(gpu_device, images, S, 6, name)
    views = _augment(eng, cfg, S, records, gpu_device)
    eng.close()
    _check(images, records, views, name, f"S={S}")


def _lanczos_direct_width(emu, S: int) -> int:
    """The first crop width whose LANCZOS taps do not fit k_hresize's LDS (hresize_tile R = 0,
    the direct path), from the kernel's own tile function as tests/helpers.py walks it."""
    lib = _lib.load()
    out = (ctypes.c_int32 * 5)()
    k = ctypes.c_int32(0)
    for cw in range(S + 1, 20000):
        _lib.check(lib.dino_resample_coeffs_host(RESAMPLE_FILTERS["lanczos"], cw, S, 0, 0, ctypes.byref(k), None, None),
                   "dino_resample_coeffs_host")
        emu.emu_hresize_tile(S, cw, 8, k.value, out)
        if out[2] == 0:
            return cw
    raise AssertionError("no direct-path width")


def test_lanczos_tile_stress(gpu_device, emu):
    """LANCZOS at S = 96: a 1500 x 40 crop of a 1600 x 48 image (24 tap groups, the generic
    group loop, narrow slices), and a crop of the first width that takes the direct path."""
    S = 96
    wd = _lanczos_direct_width(emu, S)
    images = _images([(1600, 48), (wd, 8)], 7)
    records = [[cpu_ref.ViewParams(out_size=S, crop_top=5, crop_left=60, crop_h=40, crop_w=1500)],
               [cpu_ref.ViewParams(out_size=S, crop_top=0, crop_left=0, crop_h=8, crop_w=wd, flip=True)]]
    eng, cfg = _engine_for(gpu_device, images, S, 1, "lanczos")
    views = _augment(eng, cfg, S, records, gpu_device)
    eng.close()
    _check(images, records, views, "lanczos", f"direct width {wd}")


@pytest.mark.parametrize("name", ["bilinear", "lanczos"])
def test_vertical_first(gpu_device, name):
    """A 3 x 400 crop to S = 30: over 100 times as high as wide, so Pillow runs the vertical
    pass first (resample_vfirst holds for every filter) and so does k_rcoeffs."""
    S = 30
    images = _images([(14, 450)], 9)
    records = [[cpu_ref.ViewParams(out_size=S, crop_top=20, crop_left=4, crop_h=400, crop_w=3),
                cpu_ref.ViewParams(out_size=S, crop_top=0, crop_left=11, crop_h=400, crop_w=3, flip=True)]]
    eng, cfg = _engine_for(gpu_device, images, S, 2, name)
    views = _augment(eng, cfg, S, records, gpu_device)
    eng.close()
    _check(images, records, views, name, "vertical first")


RESIZES = [(40, 24, 16, 16), (24, 40, 32, 16), (16, 16, 16, 16)]


def _resize_engine(gpu_device, im, ow, oh, name):
    h, w, _ = im.shape
    eng = IngestEngine(gpu_device, max_batch=1, max_views=1, max_crop_size=8)
    eng.set_resample_filter(name)
    buf, off = pack_jpegs([fallback.raw_container(im)], pin=False)
    eng.reserve(0, resize_scratch_bound(w, h, ow, oh))
    raw = torch.ones(1, dtype=torch.uint8, device=gpu_device)
    info = eng.decode(buf.to(gpu_device), off.to(gpu_device), 1, raw_mask=raw)
    assert int(info.cpu()[0, 0]) == 0
    out = eng.resize_batch(ow, oh, MEAN, STD, OUT_FP32)
    torch.cuda.synchronize()
    st = eng.batch_info(torch.empty(1, 4, dtype=torch.int32, device=gpu_device)).cpu().numpy()
    assert st[0, 0] == 0, st
    return eng, out.cpu()


@pytest.mark.parametrize("name", NEW_FILTERS)
def test_decode_only_recipe(gpu_device, name):
    """dino_resize_batch per filter: both axes down, one up and one down, and the identity."""
    for k, (w, h, ow, oh) in enumerate(RESIZES):
        im = _images([(w, h)], 20 + k)[0]
        eng, out = _resize_engine(gpu_device, im, ow, oh, name)
        eng.close()
        ref = cpu_ref.to_tensor_normalized(Image.fromarray(im, "RGB").resize((ow, oh), PIL_FILTER[name]), MEAN, STD,
                                           torch.float32)
        assert out.shape == (1, 3, oh, ow)
        assert torch.equal(ref, out[0]), (name, w, h, ow, oh, float((ref - out[0]).abs().max()))


@pytest.mark.parametrize("name", NEW_FILTERS)
def test_device_taps_equal_host_taps(gpu_device, name):
    """The tables k_dcoeffs wrote (the same resample_coeffs_one as k_rcoeffs, with the device's
    double sin / cos for HAMMING and LANCZOS), read back through dino_debug_region 7, equal
    dino_resample_coeffs_host's exactly: bounds and every 22-bit tap, up- and downscaling."""
    lib = _lib.load()
    f = RESAMPLE_FILTERS[name]
    P = ctypes.c_void_p
    for w, h, ow, oh in [(40, 24, 16, 16), (24, 40, 32, 16), (200, 131, 30, 64), (37, 90, 64, 33), (1600, 48, 96, 97)]:
        im = np.zeros((h, w, 3), np.uint8)
        eng, _ = _resize_engine(gpu_device, im, ow, oh, name)
        want = []
        for n_in, n_out in ((w, ow), (h, oh)):
            k = ctypes.c_int32(0)
            _lib.check(lib.dino_resample_coeffs_host(f, n_in, n_out, 0, 0, ctypes.byref(k), None, None), "ksize")
            b, t = np.zeros((n_out, 2), np.int32), np.zeros((n_out, k.value), np.int32)
            _lib.check(lib.dino_resample_coeffs_host(f, n_in, n_out, 0, n_out, ctypes.byref(k), b.ctypes.data_as(P),
                                                     t.ctypes.data_as(P)), "taps")
            want.append((b, t))
        (hb, ht), (vb, vt) = want
        v0 = (ow * (2 + ht.shape[1]) * 4 + 15) // 16 * 16  # plan.hpp dec_scratch
        n = v0 + oh * (2 + vt.shape[1]) * 4
        got = eng.debug_region(0, 7, n).cpu().numpy()
        eng.close()
        g32 = got[:n // 4 * 4].view(np.int32)
        assert np.array_equal(g32[:2 * ow].reshape(ow, 2), hb), (name, w, ow)
        assert np.array_equal(g32[2 * ow:2 * ow + ht.size].reshape(ht.shape), ht), (name, w, ow)
        q = v0 // 4
        assert np.array_equal(g32[q:q + 2 * oh].reshape(oh, 2), vb), (name, h, oh)
        assert np.array_equal(g32[q + 2 * oh:q + 2 * oh + vt.size].reshape(vt.shape), vt), (name, h, oh)


def test_setter_rejects_unknown_codes(gpu_device):
    eng = IngestEngine(gpu_device, max_batch=1, max_views=1, max_crop_size=8)
    for bad in (-1, 5, 1000):
        assert eng.lib.dino_ctx_set_resample_filter(eng._ctx, bad) != 0
        assert b"unknown filter" in eng.lib.dino_last_error()
    with pytest.raises(ValueError):
        eng.set_resample_filter("nearest")
    eng.set_resample_filter("lanczos")
    assert eng.resample_filter == 4
    eng.set_resample_filter(None)
    assert eng.resample_filter == 0
    eng.close()


def test_backend_eval_route(gpu_device):
    """MI355XBackend(resample_filter="spec") honours EvalAugSpec.interpolation: Pillow's
    BILINEAR resize of the shorter side + centre crop; with resample_filter=None the same spec
    is the bicubic oracle's, as CPUBackend's."""
    from dataloader_amd.backend import MI355XBackend
    from dataloader_amd.config import EvalAugSpec, PipelineConfig
    from dataloader_amd.pipeline import MI355XPipelineIterator
    jpegs = [(GOLDEN / n).read_bytes() for n in ("q50_71x53.jpg", "q95_48x64.jpg", "s444_40x40.jpg", "wide_160x40.jpg")]
    spec = EvalAugSpec(crop_size=32, interpolation="bilinear")

    class Src:
        _batch_size = len(jpegs)
        _resolution_src = None

        def __call__(self):
            return jpegs

    def run(be):
        pipe = be.build_pipeline(Src(), spec, PipelineConfig(output_dtype="fp32"), None)
        out = next(MI355XPipelineIterator(pipe, spec.output_map, len(jpegs)))[0]["view_0"].cpu()
        torch.cuda.synchronize()
        pipe.close()
        return out

    got = run(MI355XBackend(resample_filter="spec"))
    for b, j in enumerate(jpegs):
        img = cpu_ref.decode_rgb(j)
        nw, nh, left, top = cpu_ref.eval_geometry(img.size[0], img.size[1], 32)
        img = img.resize((nw, nh), Image.BILINEAR).crop((left, top, left + 32, top + 32))
        assert torch.equal(cpu_ref.to_tensor_normalized(img, spec.mean, spec.std, torch.float32), got[b]), b
    got = run(MI355XBackend(resample_filter=None))
    for b, j in enumerate(jpegs):
        assert torch.equal(cpu_ref.eval_one(j, 32, spec.mean, spec.std, out_dtype=torch.float32), got[b]), b


def test_dinov2_recipe_bilinear(gpu_device):
    """The DINOv2 recipe with device-drawn records, B = 4, BILINEAR: each view's Pillow-resized
    crop through oracle.cpu_ref's own post-resize ops (flip, ColorJitter in the drawn order,
    grayscale, solarize), bit-exact.  The blur probabilities are zero here: the blur is compared
    with torch's conv2d to within one level by this project's rule, not
    bit for bit, it runs after the resize and does not know the filter."""
    S, L = 64, 32
    cfg = DINOAugConfig(global_crop_size=S, local_crop_size=L, n_local_crops=4, blur_prob_global1=0.0,
                        blur_prob_global2=0.0, blur_prob_local=0.0, solarize_prob=0.5)
    nv = cfg.n_views
    images = _images([(160, 120), (97, 140), (200, 131), (64, 64)], 31)
    B = len(images)
    eng = IngestEngine(gpu_device, max_batch=B, max_views=nv, max_crop_size=S)
    eng.set_resample_filter("bilinear")
    buf, off = pack_jpegs([fallback.raw_container(im) for im in images], pin=False)
    raw = np.ones(B, np.uint8)
    ccfg = make_aug_config(cfg, S, L, OUT_FP32)
    _, ws, aws = fallback.probe(buf.data_ptr(), off.numpy(), B, 0, ccfg, raw)
    eng.reserve(ws, aws)
    eng.decode(buf.to(gpu_device), off.to(gpu_device), B, raw_mask=torch.from_numpy(raw).to(gpu_device))
    prm = eng.sample_params(ccfg, seed=11, batch_index=3)
    views = [v.cpu() for v in eng.augment(ccfg, prm)]
    torch.cuda.synchronize()
    recs = params_from_device(prm)
    eng.close()
    assert recs["jitter"].any() and recs["gray"].any() and recs["solarize"].any() and recs["flip"].any()
    assert not recs["blur"].any()
    for b, im in enumerate(images):
        for v in range(nv):
            p = record_to_params(recs[b * nv + v])
            img = Image.fromarray(im, "RGB").crop((p.crop_left, p.crop_top, p.crop_left + p.crop_w, p.crop_top + p.crop_h))
            img = img.resize((p.out_size, p.out_size), Image.BILINEAR)
            if p.flip:
                img = img.transpose(Image.FLIP_LEFT_RIGHT)
            if p.jitter:
                img = cpu_ref.color_jitter(img, p)
            if p.gray:
                img = img.convert("L").convert("RGB")
            if p.solarize:
                img = ImageOps.solarize(img, 128)
            ref = cpu_ref.to_tensor_normalized(img, cfg.mean, cfg.std, torch.float32)
            assert torch.equal(ref, views[v][b]), (b, v, float((ref - views[v][b]).abs().max()))

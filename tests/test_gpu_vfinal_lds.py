"""GPU: k_vfinal (the fused vertical pass + epilogue of views up to 128) with its separable
blur through an LDS float strip.

Check A: every case on the default route (k_vfinal) and again in a context created under
DINO_VFINAL_MAX_S=0 (k_vert + k_final) gives the same bits, blurred or not: k_final's
separable form (KS 3..9) and its 2-D form (KS 11) fix the fma order that k_vfinal follows.
Check B: unblurred views equal oracle.cpu_ref bit for bit; blurred ones stay within the
bound of tests/test_gpu_parity.py (one uint8 level, 1/255/std in output units plus one ulp of
the output type, on <= 0.5 % of a view's values), which comes from the reference's own
irreproducible torch.exp kernel.

Sizes: 96 (the workload's), 128 (the fused kernel's limit), 12 (the smallest word-path view
that admits KS 9) and 10 (S % 4 != 0, the scalar path).  Per size: blur off, KS 3/5/7/9 and
the generic 11 (S >= 12), each with solarize and flip on and off, half of them with a
ColorJitter that holds a contrast op (the mean path), one grayscale view, one view without a
horizontal pass where the image allows, and two blurred crops at the image's top-left and
bottom-right corners (halo reflection and the vertical pass's edge rows together).

test_host_separable_order_within_bound restates the separable fma order on the host (float32
fma emulated exactly in float64) and holds it to the same bound on the same inputs; it needs
no GPU work."""

from __future__ import annotations

import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

from dataloader_amd.config import DINOAugConfig
from dataloader_amd.engine import IngestEngine, pack_jpegs, params_to_device
from dataloader_amd.params import OUT_BF16, OUT_FP32, OUT_FP8_E4M3, make_aug_config
from dataloader_amd.synthetic import make_jpeg
from oracle import cpu_ref
from tests.helpers import params_to_record

pytestmark = pytest.mark.gpu

SIZES = (96, 128, 12, 10)
SHAPES = ((64, 48), (97, 61))  # (w, h), 4:2:0
ONE_LEVEL = 1.0 / 255.0 / min(cpu_ref.IMAGENET_STD)
ULP = {torch.bfloat16: 0.0161, torch.float32: 1e-6, torch.float8_e4m3fn: 0.26}  # as tests/test_gpu_parity.py
SIGMA = {3: 0.4, 5: 1.0, 7: 1.6, 9: 2.0, 11: 2.6}  # (ksize = max(3, int(4 sigma + 1) | 1))
JITTER = dict(jitter=True, order=(3, 0, 1, 2), brightness=1.2, contrast=0.7, saturation=1.3, hue=0.04)


@functools.lru_cache(maxsize=None)
def _jpegs():
    return tuple(make_jpeg(w, h, 40 + k, subsampling=2) for k, (w, h) in enumerate(SHAPES))


def _slot(S: int, w: int, h: int) -> list:
    """The view records of one w x h image at view size S."""
    crops = [(3, 2, w - 7, h - 5), (w // 3, h // 4, w // 2, h // 2), (1, 0, w - 1, h // 3), (0, 5, w // 4, h - 5)]
    out, n = [], 0
    for ks in (1, 3, 5, 7, 9, 11):
        if ks // 2 >= S or (ks == 11 and S < 12):
            continue
        for sol in (False, True):
            for flip in (False, True):
                left, top, cw, ch = crops[n % len(crops)]
                n += 1
                out.append(cpu_ref.ViewParams(out_size=S, crop_top=top, crop_left=left, crop_h=ch, crop_w=cw, flip=flip,
                                              blur=ks > 1, ksize=ks if ks > 1 else 0, sigma=SIGMA.get(ks, 0.0),
                                              solarize=sol, **(JITTER if sol != flip else {})))
    out.append(dataclasses.replace(out[9], gray=True))  # (KS 5, jittered)
    if S <= min(sw for sw, _ in SHAPES):  # no horizontal pass: the scalar path of the vertical pass at any S
        out.append(cpu_ref.ViewParams(out_size=S, crop_top=1, crop_left=2, crop_h=h - 3, crop_w=S, flip=True, blur=True,
                                      ksize=7, sigma=1.7, **JITTER))
    out.append(cpu_ref.ViewParams(out_size=S, crop_top=0, crop_left=0, crop_h=h // 2, crop_w=w // 2, blur=True, ksize=9,
                                  sigma=1.9, **JITTER))
    out.append(cpu_ref.ViewParams(out_size=S, crop_top=h - h // 3, crop_left=w - w // 2, crop_h=h // 3, crop_w=w // 2,
                                  flip=True, blur=True, ksize=9, sigma=1.9, solarize=True))
    return out


@functools.lru_cache(maxsize=None)
def _oracle_images(S: int):
    """[image][view] -> the oracle's augmented PIL image (computed once per size)."""
    res = []
    for jpg, (w, h) in zip(_jpegs(), SHAPES):
        dec = cpu_ref.decode_rgb(jpg)
        res.append([cpu_ref.augment_image(dec, p) for p in _slot(S, w, h)])
    return res


def _run(device, S: int, out_code: int, max_s: str | None):
    """Every case of size S through one fresh context (max_s: DINO_VFINAL_MAX_S while it is created)."""
    jpegs = _jpegs()
    records = [_slot(S, w, h) for w, h in SHAPES]
    nv, B = len(records[0]), len(jpegs)
    cfg = DINOAugConfig(global_crop_size=S, local_crop_size=S, n_global_crops=nv, n_local_crops=0)
    old = os.environ.get("DINO_VFINAL_MAX_S")
    try:
        if max_s is not None:
            os.environ["DINO_VFINAL_MAX_S"] = max_s
        eng = IngestEngine(device, max_batch=B, max_views=nv, max_crop_size=S)
    finally:
        if old is None:
            os.environ.pop("DINO_VFINAL_MAX_S", None)
        else:
            os.environ["DINO_VFINAL_MAX_S"] = old
    buf, off = pack_jpegs(list(jpegs), pin=False)
    info = eng.decode(buf.to(device), off.to(device), B).cpu().numpy()
    assert (info[:, 0] == 0).all(), info
    recs = np.stack([params_to_record(p) for slot in records for p in slot])
    views = eng.augment(make_aug_config(cfg, S, S, out_code), params_to_device(recs, device))
    torch.cuda.synchronize()
    info = eng.batch_info(torch.empty(B, 4, dtype=torch.int32, device=device)).cpu().numpy()
    assert (info[:, 0] == 0).all(), info
    views = [v.cpu() for v in views]
    eng.close()
    return records, views


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


@pytest.mark.parametrize("S", SIZES)
def test_vfinal_routes_and_oracle(gpu_device, S):
    cfg0 = DINOAugConfig()
    dtypes = [(OUT_BF16, torch.bfloat16), (OUT_FP32, torch.float32)] + ([(OUT_FP8_E4M3, torch.float8_e4m3fn)] if S == 96 else [])
    ref_imgs = _oracle_images(S)
    bad_a, bad_b, nblur = [], [], 0
    for code, td in dtypes:
        records, fused = _run(gpu_device, S, code, None)
        _, split = _run(gpu_device, S, code, "0")
        for b, slot in enumerate(records):
            for v, p in enumerate(slot):
                got, two = fused[v][b], split[v][b]
                assert got.dtype == td and two.dtype == td
                if not torch.equal(_bits(got), _bits(two)):  # check A
                    bad_a.append((str(td), b, v, p.ksize, int((_bits(got) != _bits(two)).sum())))
                ref = cpu_ref.to_tensor_normalized(ref_imgs[b][v], cfg0.mean, cfg0.std, td).float()
                diff = (ref - got.float()).abs()
                nd, mx = int((diff > 0).sum()), float(diff.max())
                if p.blur:  # check B
                    nblur += 1
                    print(f"S={S} {td} image {b} view {v} ks {p.ksize}: {nd} of {diff.numel()} differ, max {mx:.6f}")
                    if mx > ONE_LEVEL + ULP[td] or nd > 0.005 * diff.numel():
                        bad_b.append((str(td), b, v, p.ksize, nd, mx))
                elif nd:
                    bad_b.append((str(td), b, v, 0, nd, mx))
    assert nblur > 0
    assert not bad_a, f"S={S}: k_vfinal differs from k_vert + k_final (dtype, image, view, ks, n): {bad_a[:12]}"
    assert not bad_b, f"S={S}: views off the oracle (dtype, image, view, ks, n, max): {bad_b[:12]}"


def _fma32(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """float32 fma: the product of two float32 is exact in float64; the sum is rounded to odd
    there (from its exact TwoSum error), so that the final rounding to float32 is the only one."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _sep_blur_u8(img: np.ndarray, k1: np.ndarray) -> np.ndarray:
    """final_compute_sep's order on a u8 [H, W, 3] image: h = fma(w[c], px[c], h) over the row
    taps from 0, acc = fma(w[a], h(y + a), acc) over the rows from 0, rint, clamp."""
    ks, pad = len(k1), len(k1) // 2
    x = np.pad(img.astype(np.float32), ((pad, pad), (pad, pad), (0, 0)), mode="reflect")
    H, W = img.shape[:2]
    hrow = np.zeros((H + 2 * pad, W, 3), np.float32)
    for c in range(ks):
        hrow = _fma32(np.full_like(hrow, k1[c]), x[:, c:c + W], hrow)
    acc = np.zeros((H, W, 3), np.float32)
    for a in range(ks):
        acc = _fma32(np.full_like(acc, k1[a]), hrow[a:a + H], acc)
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def test_host_separable_order_within_bound():
    n = 0
    for S in SIZES:
        for jpg, (w, h) in zip(_jpegs(), SHAPES):
            dec = cpu_ref.decode_rgb(jpg)
            for v, p in enumerate(_slot(S, w, h)):
                if not p.blur or p.ksize > 9:
                    continue
                ref = np.asarray(cpu_ref.augment_image(dec, dataclasses.replace(p, solarize=False)))
                pre = np.asarray(cpu_ref.augment_image(dec, dataclasses.replace(p, blur=False, solarize=False)))
                got = _sep_blur_u8(pre, cpu_ref.gaussian_kernel1d(p.ksize, p.sigma).numpy())
                d = np.abs(ref.astype(np.int32) - got.astype(np.int32))
                assert d.max() <= 1 and (d > 0).mean() <= 0.005, (S, w, h, v, p.ksize, int(d.max()), float((d > 0).mean()))
                n += 1
    assert n >= 4 * len(SIZES) * len(SHAPES)

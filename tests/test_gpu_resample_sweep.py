"""GPU: the resample kernels against Pillow, bit for bit, at every tile shape of k_hresize
(first and last crop width of each, tests/helpers.py), at view sizes from 30 to the ABI's
limit of 1024 (both sides of the fused / unfused boundary at 128, slices wider than the
workgroup at 518 and 1024), on degenerate crops, and on content whose bicubic sums leave
[0, 255] at both ends (tests/resample_cases.py; test_resample_shapes_cpu.py checks that the
cases are what they claim).  Inputs are raw RGB containers, so the pixels are exact."""

from __future__ import annotations

import io

import numpy as np
import pytest
import torch
from PIL import Image

from dataloader_amd import fallback
from dataloader_amd.config import DINOAugConfig
from dataloader_amd.engine import IngestEngine, pack_jpegs, params_to_device
from dataloader_amd.params import OUT_BF16, OUT_FP32, make_aug_config
from dataloader_amd.synthetic import textured_rgb
from oracle import cpu_ref
from tests import resample_cases as rc
from tests.helpers import SWEEP_SIZES, params_to_record
from tests.test_gpu_parity import _check_views

pytestmark = pytest.mark.gpu


def _engine_for(gpu_device, images, S, nv):
    """Raw containers of the images decoded into an engine whose workspaces are sized by the
    probe (decode bytes, and the augment bound of nv views of size S per image)."""
    B = len(images)
    cfg = DINOAugConfig(global_crop_size=S, local_crop_size=S, n_global_crops=nv, n_local_crops=0)
    eng = IngestEngine(gpu_device, max_batch=B, max_views=nv, max_crop_size=S)
    buf, off = pack_jpegs([fallback.raw_container(im) for im in images], pin=False)
    raw = np.ones(B, np.uint8)
    pinfo, ws, aws = fallback.probe(buf.data_ptr(), off.numpy(), B, 0, make_aug_config(cfg, S, S, OUT_FP32), raw)
    assert (pinfo[:, 0] == 0).all(), pinfo
    eng.reserve(ws, aws)
    info = eng.decode(buf.to(gpu_device), off.to(gpu_device), B, raw_mask=torch.from_numpy(raw).to(gpu_device))
    info = info.cpu().numpy()
    assert (info[:, 0] == 0).all(), info
    assert [(int(w), int(h)) for w, h in info[:, 1:3]] == [(im.shape[1], im.shape[0]) for im in images]
    return eng, cfg


def _augment(eng, cfg, S, records, out_code, device):
    recs = np.stack([params_to_record(p) for slot in records for p in slot])
    views = eng.augment(make_aug_config(cfg, S, S, out_code), params_to_device(recs, device))
    torch.cuda.synchronize()
    info = eng.batch_info(torch.empty(len(records), 4, dtype=torch.int32, device=device)).cpu().numpy()
    assert (info[:, 0] == 0).all(), info  # (no view left out for want of scratch)
    return views


@pytest.mark.parametrize("S", SWEEP_SIZES)
def test_resize_sweep_bit_exact(gpu_device, emu, S):
    """Every resize-only case of tests/resample_cases.py, fp32 (and bf16 at 224), bit-exact.
    (The 31 x 4001 crop of the height sweep at S = 30 is the one that found Pillow's
    vertical-pass-first rule, resample_vfirst; test_vertical_pass_first_crops pins it.)"""
    cfg0 = DINOAugConfig()
    cases = rc.resize_cases(emu, S)
    nv = rc.MAX_VIEWS if S <= 256 else 8  # (fewer spare views to render at 3 S^2 floats each)
    images, records, keep = rc.pack_cases(cases, nv)
    eng, cfg = _engine_for(gpu_device, images, S, nv)
    dtypes = [(OUT_FP32, torch.float32)] + ([(OUT_BF16, torch.bfloat16)] if S == 224 else [])
    outs = [(_augment(eng, cfg, S, records, code, gpu_device), td) for code, td in dtypes]
    eng.close()
    pil = {}
    bad, n = [], 0
    for b, (im, slot) in enumerate(zip(images, records)):
        dec = pil.setdefault(id(im), Image.fromarray(im, "RGB"))
        for v, p in enumerate(slot):
            if not keep[b][v]:
                continue
            n += 1
            for views, td in outs:
                ref = cpu_ref.augment_one(b"", p, cfg0.mean, cfg0.std, out_dtype=td, decoded=dec)
                got = views[v][b].cpu()
                assert got.dtype == td
                if not torch.equal(ref, got):
                    d = (ref.float() - got.float()).abs()
                    bad.append((im.shape[1], im.shape[0], p.crop_left, p.crop_top, p.crop_w, p.crop_h, p.flip,
                                str(td), int((d > 0).sum()), float(d.max())))
    assert n == sum(len(r) for _, r in cases)
    assert not bad, f"S={S}: {len(bad)} of {n} views differ (W, H, left, top, cw, ch, flip, dtype, n, max): {bad[:12]}"
    # constant images: exactly the normalised 255 / 0 everywhere (the >= side of the clip)
    views = outs[0][0]
    mean, std = np.asarray(cfg0.mean, np.float32), np.asarray(cfg0.std, np.float32)
    for b, im in enumerate(images):
        if im.min() == im.max() and im.shape[0] == 24:
            level = torch.from_numpy(np.asarray(im[0, 0], np.float32)).div(255)
            want = ((level - torch.from_numpy(mean)) / torch.from_numpy(std)).view(3, 1, 1).expand(3, S, S)
            for v in range(3):
                assert torch.equal(views[v][b].cpu(), want), (S, b, v)


@pytest.mark.parametrize("S", [30, 32, 132])
def test_vertical_pass_first_crops(gpu_device, S):
    """Crops over 100 times as high as wide whose height shrinks: Pillow runs the vertical pass
    first, and so does k_rcoeffs (resample_vfirst), ahead of the scalar fused (30), the word
    fused (32) and the unfused (132) vertical kernels, which then copy.  Both sides of the
    100 x rule, a view one row lower than the crop, and a square crop in the same launch."""
    rng = np.random.default_rng(3000 + S)
    W, H = 14, 1500
    images = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8), rng.integers(0, 2, size=(H, W, 3), dtype=np.uint8) * 255]
    crops = [(9, 1300), (12, 1201), (12, 1200), (1, S + 1), (14, 1500), (14, 14), (3, 301), (2, 1499)]
    records = [[cpu_ref.ViewParams(out_size=S, crop_top=(H - ch) if k & 1 else 0, crop_left=(W - cw) if k & 2 else 0,
                                   crop_h=ch, crop_w=cw, flip=bool(k & 4)) for k, (cw, ch) in enumerate(crops)]
               for _ in images]
    eng, cfg = _engine_for(gpu_device, images, S, len(crops))
    views = _augment(eng, cfg, S, records, OUT_FP32, gpu_device)
    eng.close()
    cfg0 = DINOAugConfig()
    for b, im in enumerate(images):
        dec = Image.fromarray(im, "RGB")
        for v, p in enumerate(records[b]):
            ref = cpu_ref.augment_one(b"", p, cfg0.mean, cfg0.std, out_dtype=torch.float32, decoded=dec)
            assert torch.equal(ref, views[v][b].cpu()), (S, b, p.crop_w, p.crop_h)


def _png(rgb: np.ndarray) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, format="PNG", compress_level=1)
    return buf.getvalue()


@pytest.mark.parametrize("S", [128, 132, 518, 1024])
def test_blur_and_jitter_at_new_view_sizes(gpu_device, S):
    """Full ColorJitter in four op orders, blur ksize 1, 9, 13 and 15 (pad 7, the largest the
    ABI admits) and a solarized view without blur, on textured content, at the largest fused
    view (128), the smallest unfused one (132), 518 (S % 4 != 0) and 1024: the rule of
    test_gpu_parity._check_views (bit-exact; blur within one level on <= 0.5 % of a view)."""
    rng = np.random.default_rng(2000 + S)
    W, H = S + S // 3 + 5, S + 9
    images = [textured_rgb(W, H, rng), textured_rgb(S // 2 + 3, S // 2 + 8, rng)]
    orders = [(3, 2, 1, 0), (1, 0, 2, 3), (0, 1, 2, 3), (2, 3, 0, 1)]
    records = []
    for b, im in enumerate(images):
        h, w, _ = im.shape
        slot = []
        for v, ks in enumerate([1, 9, 13, 15, 0]):
            cw, ch = [(w, h), (w - 7, h // 2), (w // 2 + 1, h - 3), (w - 1, h - 1), (w // 3, h // 3)][v]
            slot.append(cpu_ref.ViewParams(
                out_size=S, crop_top=(h - ch) // 2, crop_left=w - cw, crop_h=ch, crop_w=cw, flip=bool((b + v) & 1),
                jitter=True, order=orders[(b + v) % 4], brightness=[1.25, 0.8, 1.1, 0.6, 1.4][v],
                contrast=[0.7, 1.3, 0.9, 1.2, 0.6][v], saturation=[1.3, 0.5, 1.6, 0.9, 1.2][v],
                hue=[0.1, -0.07, 0.03, -0.2, 0.15][v], gray=False, blur=ks > 0,
                sigma=[0.4, 1.9, 2.6, 3.1, 1.0][v], ksize=max(ks, 1), solarize=ks == 0))
        records.append(slot)
    eng, cfg = _engine_for(gpu_device, images, S, 5)
    views = _augment(eng, cfg, S, records, OUT_FP32, gpu_device)
    eng.close()
    recs = np.stack([params_to_record(p) for slot in records for p in slot])
    cfg0 = DINOAugConfig()
    worst = _check_views([_png(im) for im in images], [v.cpu() for v in views], recs, 5, torch.float32, cfg0.mean, cfg0.std)
    print(f"S={S}: blur views differ on at most {worst:.4%} of their values")

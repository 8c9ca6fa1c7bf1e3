"""GPU: the vertical resample pass with 24-bit multiply-adds (csrc/resize.hpp tap_mad) against
Pillow, bit for bit, at the operand extremes: pixels 0 and 255 in every arrangement along y
(constant, checkerboard, row stripes of period 1 and 2) and noise; crops that downscale,
keep their height (no vertical pass), and upscale until a tap sits at or next to weight 1.0,
the largest coefficient; crops at the image's top and bottom edge; the word path of k_vfinal
(32, 96) and of k_vert + k_final (224) and the scalar path (30, S % 4 != 0); flip on and
off.  Tap counts per output row run from 2 (clipped at the crop's edge) to 13, odd and even,
so the unrolled tap loop's tail runs.  One decode-only batch (k_dhpass, k_dvpass) per
direction at the same extremes.  Inputs are raw RGB containers, so the pixels are exact."""

from __future__ import annotations

import numpy as np
import pytest
import torch
from PIL import Image

from dataloader_amd import fallback
from dataloader_amd.config import DINOAugConfig
from dataloader_amd.engine import IngestEngine, pack_jpegs
from dataloader_amd.params import OUT_FP32
from dataloader_amd.pipeline import resize_scratch_bound
from oracle import cpu_ref
from tests.helpers import dec_scratch_total
from tests.test_gpu_resample_sweep import _augment, _engine_for

pytestmark = pytest.mark.gpu

W, H = 144, 256


def _patterns(w: int, h: int) -> list[np.ndarray]:
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(24)
    planes = [np.zeros((h, w)), np.full((h, w), 255), ((xx + yy) & 1) * 255, (yy & 1) * 255, ((yy >> 1) & 1) * 255]
    imgs = [np.ascontiguousarray(np.repeat(p.astype(np.uint8)[:, :, None], 3, axis=2)) for p in planes]
    imgs.append(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
    return imgs


def _crop_heights(S: int) -> list[int]:
    """3x and 1.3x downscales (as far as a 256-row image allows), no vertical pass, and
    upscales down to a 2-row crop."""
    hs = [min(H, 3 * S), min(H, int(1.3 * S) + 1), S, max(2, S // 3 + 1), 5, 2]
    return sorted(set(hs), reverse=True)


@pytest.mark.parametrize("S", [96, 224, 32, 30])
def test_vertical_pass_extremes_bit_exact(gpu_device, S):
    images = _patterns(W, H)
    slot = []
    for k, ch in enumerate(_crop_heights(S)):
        for flip in (False, True):
            top = 0 if (k + flip) & 1 else H - ch  # the image's top edge, or its bottom edge
            cw = S if (k == 1 and S <= W) else W - 3 * k  # (one view without a horizontal pass)
            slot.append(cpu_ref.ViewParams(out_size=S, crop_top=top, crop_left=(W - cw) if flip else 0,
                                           crop_h=ch, crop_w=cw, flip=flip))
    records = [slot for _ in images]
    eng, cfg = _engine_for(gpu_device, images, S, len(slot))
    views = _augment(eng, cfg, S, records, OUT_FP32, gpu_device)
    eng.close()
    cfg0 = DINOAugConfig()
    bad = []
    for b, im in enumerate(images):
        dec = Image.fromarray(im, "RGB")
        for v, p in enumerate(slot):
            ref = cpu_ref.augment_one(b"", p, cfg0.mean, cfg0.std, out_dtype=torch.float32, decoded=dec)
            got = views[v][b].cpu()
            if not torch.equal(ref, got):
                bad.append((b, p.crop_top, p.crop_w, p.crop_h, p.flip, int((ref != got).sum())))
    assert not bad, f"S={S}: {len(bad)} views differ (image, top, cw, ch, flip, n): {bad[:12]}"


@pytest.mark.parametrize("w,h,ow,oh", [(200, 255, 66, 85), (24, 9, 96, 36), (96, 255, 96, 85)])
def test_decode_only_extremes_bit_exact(gpu_device, w, h, ow, oh):
    """k_dhpass + k_dvpass: a 3x downscale, a 4x upscale of a 9-row image, and a vertical pass
    alone (straight from the decoded image)."""
    images = _patterns(w, h)
    B = len(images)
    cfg0 = DINOAugConfig()
    eng = IngestEngine(gpu_device, max_batch=B, max_views=1, max_crop_size=max(ow, oh))
    buf, off = pack_jpegs([fallback.raw_container(im) for im in images], pin=False)
    raw = np.ones(B, np.uint8)
    pinfo, ws, _ = fallback.probe(buf.data_ptr(), off.numpy(), B, 0, raw_mask=raw)
    assert (pinfo[:, 0] == 0).all(), pinfo
    eng.reserve(ws, B * resize_scratch_bound(w, h, ow, oh))
    info = eng.decode(buf.to(gpu_device), off.to(gpu_device), B, raw_mask=torch.from_numpy(raw).to(gpu_device))
    assert (info.cpu().numpy()[:, 0] == 0).all()
    out = eng.resize_batch(ow, oh, cfg0.mean, cfg0.std, OUT_FP32)
    torch.cuda.synchronize()
    info = eng.batch_info(torch.empty(B, 4, dtype=torch.int32, device=gpu_device)).cpu().numpy()
    assert (info[:, 0] == 0).all(), info
    out = out.cpu()
    eng.close()
    for b, im in enumerate(images):
        ref = cpu_ref.to_tensor_normalized(Image.fromarray(im, "RGB").resize((ow, oh), Image.BICUBIC),
                                           cfg0.mean, cfg0.std, torch.float32)
        assert torch.equal(ref, out[b]), (b, int((ref != out[b]).sum()))


def test_decode_only_greedy_no_cascade(gpu_device, emu):
    """k_dplan's greedy branch: a 256 x 8192 image needs 8192 x 64 x 3 = 1 572 864 bytes of
    horizontal-pass rows, more than the engine's default augment workspace (4 x (32 x 3 x 1024
    + 256 KiB) = 1 441 792 bytes), so the batch does not fit.  The tall image alone is
    reported DINO_IMG_NO_SPACE (3) and comes out as zeros; the small images around it (under
    40 KB each) are placed and resized bit for bit.  With the workspace reserved to the exact
    sum of the images' dec_scratch totals, the batch fits and all four are bit-exact."""
    OW = OH = 64
    rng = np.random.default_rng(64)
    shapes = [(96, 64), (256, 8192), (96, 64), (64, 96)]  # (w, h)
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for w, h in shapes]
    B = len(images)
    cfg0 = DINOAugConfig()
    refs = [cpu_ref.to_tensor_normalized(Image.fromarray(im, "RGB").resize((OW, OH), Image.BICUBIC),
                                         cfg0.mean, cfg0.std, torch.float32) for im in images]
    eng = IngestEngine(gpu_device, max_batch=B, max_views=1, max_crop_size=32)
    buf, off = pack_jpegs([fallback.raw_container(im) for im in images], pin=False)
    raw = np.ones(B, np.uint8)
    pinfo, ws, _ = fallback.probe(buf.data_ptr(), off.numpy(), B, 0, raw_mask=raw)
    assert (pinfo[:, 0] == 0).all(), pinfo
    eng.reserve(ws, 0)  # the augment workspace keeps its default size
    assert eng.workspace_sizes()[1] == 1441792
    info = eng.decode(buf.to(gpu_device), off.to(gpu_device), B, raw_mask=torch.from_numpy(raw).to(gpu_device))
    assert (info.cpu().numpy()[:, 0] == 0).all()

    def run():
        out = eng.resize_batch(OW, OH, cfg0.mean, cfg0.std, OUT_FP32)
        st = eng.batch_info(torch.empty(B, 4, dtype=torch.int32, device=gpu_device))
        torch.cuda.synchronize()
        return out.cpu(), st.cpu().numpy()[:, 0].tolist()

    out, status = run()
    assert status == [0, 3, 0, 0], status
    assert not out[1].any()
    for b in (0, 2, 3):
        assert torch.equal(refs[b], out[b]), (b, int((refs[b] != out[b]).sum()))
    eng.reserve(ws, sum(dec_scratch_total(emu, w, h, OW, OH) for w, h in shapes))
    out, status = run()
    eng.close()
    assert status == [0, 0, 0, 0], status
    for b in range(B):
        assert torch.equal(refs[b], out[b]), (b, int((refs[b] != out[b]).sum()))

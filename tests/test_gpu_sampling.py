"""GPU parity on the chroma samplings and colour markers outside Pillow's writer: the files of
``tests/sampling_cases.py`` through ``IngestEngine.decode``, one batch per group.

They reach what no Pillow-written file does: k_color's generic per-pixel path (Cb and Cr at
different samplings, an upsampled luma plane) on narrow and on 2305-wide images, the
h1v2-fancy and integer-box upsamplers, and the speculative Huffman kernels (k_huff1 alone,
k_huff3, k_huff2 across segments, one restart interval per lane) and k_idct on MCUs of 4, 5,
6, 7, 8, 9 and 10 blocks, square or not.  Tolerance: none.  Where the oracle decodes a file the
status is 0 and every byte equals Pillow's; where it returns ``None`` the status is negative
and the views are zero.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from dataloader_amd.config import DINOAugConfig
from dataloader_amd.engine import IngestEngine, params_from_device
from dataloader_amd.params import OUT_BF16, VIEW_PARAMS_DTYPE, make_aug_config
from tests import sampling_cases as sc
from tests.test_gpu_parity import _check_views, _to_dev

pytestmark = pytest.mark.gpu


def _decode_group(dev, group, lane=None):
    """[(name, what, n)] for every file of the group that differs from the oracle."""
    cases, refs = sc.GROUPS[group](), sc.references(group)
    jpegs = [j for _, j in cases]
    eng = IngestEngine(dev, max_batch=len(jpegs), max_views=10, max_crop_size=224)
    if lane is not None:
        eng.set_prog_decoder(lane)
    d_bytes, d_off = _to_dev(jpegs, dev)
    info = eng.decode(d_bytes, d_off, len(jpegs)).cpu().numpy()
    bad = []
    for i, ((name, _), ref) in enumerate(zip(cases, refs)):
        st = int(info[i, 0])
        if ref is None:
            if st >= 0:
                bad.append((name, "reference rejects; status", st))
        elif st != 0:
            bad.append((name, "status", st))
        elif (int(info[i, 1]), int(info[i, 2])) != (ref.shape[1], ref.shape[0]):
            bad.append((name, "size", (int(info[i, 1]), int(info[i, 2]))))
        else:
            got = eng.copy_rgb(i, ref.shape[1], ref.shape[0]).cpu().numpy()
            if not np.array_equal(got, ref):
                bad.append((name, "bytes differing", int((got != ref).sum())))
    eng.close()
    return bad


@pytest.mark.parametrize("group", ["small", "wide", "route", "restart", "markers"])
def test_decode_group_bit_exact(gpu_device, group):
    if group == "route":  # the files still take the route their names say
        for name, j in sc.route_cases():
            assert sc.route_of(j) == name.split("_")[1], (name, sc.entropy_bytes(j))
    bad = _decode_group(gpu_device, group)
    assert not bad, f"{len(bad)} of {len(sc.GROUPS[group]())}: {bad}"


@pytest.mark.parametrize("lane", [False, True])
def test_progressive_samplings_bit_exact(gpu_device, lane):
    """Both settings of dino_ctx_set_prog_decoder; the lane decoder may hand an image to the
    wave decoder, the pixels are the same."""
    bad = _decode_group(gpu_device, "progressive", lane)
    assert not bad, bad


def test_rejected_files_give_zero_views(gpu_device):
    """Every file the oracle rejects, in one batch next to a good one: negative status, all
    views zero (the reference zero-fills)."""
    rejected = [(name, j) for g in sc.GROUPS for (name, j), ref in zip(sc.GROUPS[g](), sc.references(g)) if ref is None]
    assert len(rejected) >= 3 * len(sc.SMALL_SIZES) + 3
    good = dict(sc.small_cases())["s440_70x50"]
    jpegs = [j for _, j in rejected] + [good]
    cfg = DINOAugConfig(global_crop_size=32, local_crop_size=16, n_local_crops=2)
    eng = IngestEngine(gpu_device, max_batch=len(jpegs), max_views=cfg.n_views, max_crop_size=32)
    d_bytes, d_off = _to_dev(jpegs, gpu_device)
    views, info = eng.run_batch(d_bytes, d_off, len(jpegs), make_aug_config(cfg, 32, 16, OUT_BF16), seed=3, batch_index=0)
    torch.cuda.synchronize()
    st = info[:, 0].cpu().numpy()
    bad = [(name, int(st[i])) for i, (name, _) in enumerate(rejected) if st[i] >= 0]
    bad += [(name, "view", v) for i, (name, _) in enumerate(rejected) for v in range(cfg.n_views)
            if torch.count_nonzero(views[v][i].float()) != 0]
    assert st[-1] == 0 and all(torch.count_nonzero(v[-1].float()) > 0 for v in views)
    eng.close()
    assert not bad, bad


def test_augment_parity_on_unusual_mcus(gpu_device):
    """4:4:0 and 10-block 640x480 files through run_batch at the default config (2 x 224 +
    8 x 96): k_plan's decode workspace for these MCU shapes next to the views' scratch, every
    view against the oracle's replay of its record."""
    files = dict(sc.route_cases())
    jpegs = [files["s440_huff1_640x480"], files["s410_huff1_640x480"]]
    cfg = DINOAugConfig()
    B = len(jpegs)
    eng = IngestEngine(gpu_device, max_batch=B, max_views=cfg.n_views, max_crop_size=224)
    d_bytes, d_off = _to_dev(jpegs, gpu_device)
    params = torch.empty(B * cfg.n_views * VIEW_PARAMS_DTYPE.itemsize, dtype=torch.uint8, device=gpu_device)
    views, info = eng.run_batch(d_bytes, d_off, B, make_aug_config(cfg, 224, 96, OUT_BF16), seed=77, batch_index=1,
                                params_out=params)
    torch.cuda.synchronize()
    assert (info[:, 0].cpu().numpy() == 0).all(), info
    _check_views(jpegs, views, params_from_device(params), cfg.n_views, torch.bfloat16, cfg.mean, cfg.std)
    eng.close()

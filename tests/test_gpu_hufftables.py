"""GPU parity on Huffman table shapes no encoder in the suite emits: the files of
``tests/hufftable_cases.py`` through ``IngestEngine.decode``, one batch per group.

They reach what Annex K and optimal tables leave idle: tables whose every code is longer than
the lookahead (kLookBits 11, kDcLookBits 9, kPLookBits 9, kLLookBits 8: every symbol through
huff_slow_bits / lane_slow, no lookahead pair), codes exactly at the lookahead length and one
past it, the 17-bit bad code, lanes that are slow to synchronise (k_huff1's in-segment rounds,
k_huff3, k_huff2 across segments, one restart interval per lane), tables shared between
components or under ids 2 and 3, and tables libjpeg rejects.  Tolerance: none.  Where the oracle
decodes a file the status is 0 and every byte equals Pillow's; where it returns ``None`` the
status is negative and the views are zero.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from dataloader_amd.config import DINOAugConfig
from dataloader_amd.engine import IngestEngine, params_from_device
from dataloader_amd.params import OUT_BF16, VIEW_PARAMS_DTYPE, make_aug_config
from oracle import cpu_ref
from tests import hufftable_cases as hc
from tests.test_gpu_parity import _check_views, _jpeg_zoo, _to_dev

pytestmark = pytest.mark.gpu


def _differences(eng, info, cases, refs, ncomp=3):
    """[(name, what, n)] for every file of the decoded batch that differs from the oracle."""
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
        elif ncomp == 4 and int(info[i, 3]) != 4:
            bad.append((name, "info", info[i].tolist()))
        else:
            got = eng.copy_rgb(i, ref.shape[1], ref.shape[0]).cpu().numpy()
            if not np.array_equal(got, ref):
                bad.append((name, "bytes differing", int((got != ref).sum())))
    return bad


def _decode_group(dev, group, lane=None, four=False):
    cases, refs = hc.GROUPS[group](), hc.references(group)
    jpegs = [j for _, j in cases]
    eng = IngestEngine(dev, max_batch=len(jpegs), max_views=10, max_crop_size=224)
    if four:
        eng.set_four_component(True)
    if lane is not None:
        eng.set_prog_decoder(lane)
    d_bytes, d_off = _to_dev(jpegs, dev)
    info = eng.decode(d_bytes, d_off, len(jpegs)).cpu().numpy()
    bad = _differences(eng, info, cases, refs, 4 if four else 3)
    eng.close()
    return bad


@pytest.mark.parametrize("group", ["small", "route", "rejected"])
def test_decode_group_bit_exact(gpu_device, group):
    if group == "route":  # the files still take the route their names say
        for name, j in hc.route_cases():
            assert hc.route_of(j) == "huff" + name.split("_huff")[1][0], name
    bad = _decode_group(gpu_device, group)
    assert not bad, f"{len(bad)} of {len(hc.GROUPS[group]())}: {bad}"


@pytest.mark.parametrize("lane", [False, True])
def test_progressive_shapes_bit_exact(gpu_device, lane):
    """Both settings of dino_ctx_set_prog_decoder: the wave decoder's 9-bit lookahead and the
    lane decoder's 8-bit LDS rows with their eight slow lengths."""
    bad = _decode_group(gpu_device, "progressive", lane)
    assert not bad, bad


@pytest.mark.parametrize("lane", [False, True])
def test_four_component_shapes_bit_exact(gpu_device, lane):
    bad = _decode_group(gpu_device, "four_component", lane, four=True)
    assert not bad, bad


def test_rejected_tables_give_zero_views(gpu_device):
    """Every file the oracle rejects, in one batch next to the valid file they were made from:
    negative status and ten all-zero views (the reference zero-fills)."""
    refs = hc.references("rejected")
    rejected = [(name, j) for (name, j), ref in zip(hc.rejected_cases(), refs) if ref is None]
    assert len(rejected) >= len(hc.REJECT_USED) + 1
    jpegs = [j for _, j in rejected] + [hc.rejected_cases()[0][1]]
    cfg = DINOAugConfig(global_crop_size=32, local_crop_size=16)
    assert cfg.n_views == 10
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


@pytest.fixture(scope="module")
def mixed_batch():
    """shaped / Annex K / shaped / ...: every Pillow-written file of the parity zoo up to 1024x768
    (k_huff1 and k_huff3 items) between two shaped files, so that a work item that kept the
    previous item's LDS tables, or its skip / value lookahead overlay, decodes with the wrong
    ones."""
    shaped = [c for c in hc.small_cases() if "_70x50" in c[0] and c[0].split("_")[0] not in ("shared", "ids23")]
    shaped = shaped[::3] + hc.route_cases()[:3]
    zoo = _jpeg_zoo()
    default = [(f"zoo{i}", zoo[i]) for i in (*range(0, 12), 21, 22, 23, 27, 28, 30)]
    cases = []
    for k, d in enumerate(default):
        cases += [shaped[(2 * k) % len(shaped)], d]
    cases.append(shaped[(2 * len(default)) % len(shaped)])
    refs = [np.asarray(cpu_ref.decode_rgb(j)) for _, j in cases]
    return cases, refs


def test_mixed_batch_twice_on_one_engine(gpu_device, mixed_batch):
    cases, refs = mixed_batch
    assert [n.startswith("zoo") for n, _ in cases] == [bool(i & 1) for i in range(len(cases))]
    jpegs = [j for _, j in cases]
    eng = IngestEngine(gpu_device, max_batch=len(jpegs), max_views=10, max_crop_size=224)
    d_bytes, d_off = _to_dev(jpegs, gpu_device)
    for run in range(2):
        info = eng.decode(d_bytes, d_off, len(jpegs)).cpu().numpy()
        bad = _differences(eng, info, cases, refs)
        assert not bad, (run, bad)
    eng.close()


def test_augment_parity_on_slow_tables(gpu_device):
    """A k_huff3 and a k_huff2 file through run_batch at the default config (2 x 224 + 8 x 96):
    the coefficients reach k_idct and the resampler; every view against the oracle's replay of
    its record."""
    files = dict(hc.route_cases())
    jpegs = [files["inverted_huff3_320x240"], files["all16_huff2_400x320"]]
    cfg = DINOAugConfig()
    B = len(jpegs)
    eng = IngestEngine(gpu_device, max_batch=B, max_views=cfg.n_views, max_crop_size=224)
    d_bytes, d_off = _to_dev(jpegs, gpu_device)
    params = torch.empty(B * cfg.n_views * VIEW_PARAMS_DTYPE.itemsize, dtype=torch.uint8, device=gpu_device)
    views, info = eng.run_batch(d_bytes, d_off, B, make_aug_config(cfg, 224, 96, OUT_BF16), seed=78, batch_index=1,
                                params_out=params)
    torch.cuda.synchronize()
    assert (info[:, 0].cpu().numpy() == 0).all(), info
    _check_views(jpegs, views, params_from_device(params), cfg.n_views, torch.bfloat16, cfg.mean, cfg.std)
    eng.close()

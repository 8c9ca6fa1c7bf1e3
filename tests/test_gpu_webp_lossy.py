"""Lossy WebP on the device (``webp="device", webp_forms="all"``): the files of
tests/webp_lossy_cases.py against Pillow bit for bit, damaged files among sound ones, the option
off, a mixed batch through the backend on both routes."""

import numpy as np
import pytest
import torch

from dataloader_amd import fallback
from dataloader_amd.engine import IngestEngine
from dataloader_amd.synthetic import make_jpeg
from dataloader_amd.tario import spans_of
from tests import png_cases as pc
from tests import webp_cases as lossless
from tests import webp_lossy_cases as wc
from tests.test_gpu_parity import _to_dev
from tests.test_gpu_png import _run_backend

pytestmark = pytest.mark.gpu

CASES = wc.cases()


def _decode(dev, files, forms=True):
    eng = IngestEngine(dev, max_batch=len(files), max_views=10, max_crop_size=224)
    eng.set_webp(True)
    eng.set_webp_forms(forms)
    ptrs, lens, _keep = spans_of(files)
    form, ws = fallback.probe_webp_forms(ptrs, lens)
    eng.reserve(int(ws.sum()) + (1 << 20), 0)
    d_bytes, d_off = _to_dev(files, dev)
    return eng, form, eng.decode(d_bytes, d_off, len(files)).cpu().numpy()


def test_case_list_bit_exact_with_pillow(gpu_device):
    """Every case and fixture in one batch, with two damaged files Pillow raises on between sound ones."""
    broken = [d[1] for d in wc.damaged() if d[0] in ("mixed_m4_cut4", "noise_q100_17x33_flip1063")]
    assert len(broken) == 2 and all(pc.pillow_rgb(b) is None for b in broken)
    files = [c[1] for c in CASES]
    files[2:2] = [broken[0]]
    files[9:9] = [broken[1]]
    eng, form, info = _decode(gpu_device, files)
    assert form[2, 0] == 1 and form[9, 0] == 1, "the damage must lie where only the decode finds it"
    bad = []
    for i, data in enumerate(files):
        ref = pc.pillow_rgb(data)
        want = 1 if form[i, 0] == 0 else (0 if ref is not None else -1)
        if int(info[i, 0]) != want:
            bad.append((i, "status", int(info[i, 0]), want))
        elif want == 0:
            got = eng.copy_rgb(i, ref.shape[1], ref.shape[0]).cpu().numpy()
            if tuple(info[i, 1:3]) != ref.shape[1::-1] or not np.array_equal(got, ref):
                bad.append((i, int((got != ref).sum())))
    eng.close()
    assert not bad, bad


def test_option_off_keeps_every_lossy_file_a_hand_over(gpu_device):
    files = [c[1] for c in CASES]
    ptrs, lens, _keep = spans_of(files)
    assert (fallback.probe_webp(ptrs, lens)[0][:, 0] == 1).all()
    eng, _, info = _decode(gpu_device, files, forms=False)
    eng.close()
    assert (info[:, 0] == 1).all(), info[:, 0]


def test_mixed_batch_through_the_backend(gpu_device):
    """B = 16 of JPEGs, a lossless WebP and four lossy ones: webp_forms="all" gives the views of
    webp="host" bit for bit on both routes; the lossy files move from host_decoded to webp_device."""
    by = {c[0]: c[1] for c in CASES}
    uniq = [make_jpeg(160 + 8 * s, 120 + 4 * s, s) for s in range(5)]
    B, nb = 16, 3
    batches = [[uniq[(k + i) % 5] for i in range(B)] for k in range(nb)]
    lossy = {1: "mixed_m4", 6: "noise_q5_50x83", 9: "seg4_50x83", 14: "simple_50x83"}
    for i, n in lossy.items():
        batches[1][i] = by[n]
    batches[1][4] = {c[0]: c[1] for c in lossless.cases()}["gradient_m6"]
    (side, st), (direct, std) = (_run_backend(batches, r, webp="device", webp_forms="all") for r in ("side", "device"))
    (host, sth), (plain, stp) = _run_backend(batches, "side", webp="host"), _run_backend(batches, "side", webp="device")
    assert st["webp_device"] == 5 and st["webp_host"] == 0 and st["host_decoded"] == 0 and st["side_decoded"] == 5, st
    assert std["webp_device"] == 5 and std["host_decoded"] == 0, std
    assert stp["webp_device"] == 1 and stp["webp_host"] == 4 and stp["host_decoded"] == 4, stp
    assert sth["webp_device"] == 0 and sth["webp_host"] == 5 and sth["host_decoded"] == 5, sth
    for k in range(nb):
        for name in side[k]:
            assert torch.equal(side[k][name], host[k][name]) and torch.equal(direct[k][name], host[k][name]), (k, name)
            assert torch.equal(plain[k][name], host[k][name]), (k, name)
    for name in side[1]:
        assert all(side[1][name][i].any() for i in lossy), name

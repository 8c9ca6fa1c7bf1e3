"""Lossless WebP on the device (``webp="device"``): the files of tests/webp_cases.py against Pillow
bit for bit, damaged files among sound ones, a mixed batch on both routes and under every mode."""

import numpy as np
import pytest
import torch

from dataloader_amd import fallback
from dataloader_amd.engine import IngestEngine
from dataloader_amd.synthetic import make_jpeg
from dataloader_amd.tario import spans_of
from tests import png_cases as pc
from tests import webp_cases as wc
from tests.test_gpu_parity import _to_dev
from tests.test_gpu_png import _run_backend

pytestmark = pytest.mark.gpu

CASES = wc.cases()


def _decode(dev, files, on=True):
    eng = IngestEngine(dev, max_batch=len(files), max_views=10, max_crop_size=224)
    eng.set_webp(on)
    ptrs, lens, _keep = spans_of(files)
    form, ws = fallback.probe_webp(ptrs, lens)
    eng.reserve(int(ws.sum()) + (1 << 20), 0)
    d_bytes, d_off = _to_dev(files, dev)
    return eng, form, eng.decode(d_bytes, d_off, len(files)).cpu().numpy()


def test_case_list_bit_exact_with_pillow(gpu_device):
    """Every case in one batch, with two files damaged past their prologue between sound ones."""
    broken = [d for d in wc.damaged() if d[0] in ("gradient_m3_cut700", "gradient_m0_flip12")]  # (Pillow raises on both)
    files = [c[1] for c in CASES]
    files[2:2] = [broken[0][1]]
    files[9:9] = [broken[1][1]]
    eng, form, info = _decode(gpu_device, files)
    assert form[2, 0] == 2 and form[9, 0] == 2, "the damage must lie where only the decode finds it"
    bad = []
    for i, data in enumerate(files):
        ref = pc.pillow_rgb(data)
        want = {0: -1, 1: 1, 2: 0 if ref is not None else -1}[int(form[i, 0])]
        if int(info[i, 0]) != want:
            bad.append((i, "status", int(info[i, 0]), want))
        elif want == 0:
            got = eng.copy_rgb(i, ref.shape[1], ref.shape[0]).cpu().numpy()
            if tuple(info[i, 1:3]) != ref.shape[1::-1] or not np.array_equal(got, ref):
                bad.append((i, int((got != ref).sum())))
    eng.close()
    assert not bad, bad


def test_option_off_leaves_every_webp_corrupt(gpu_device):
    eng, _, info = _decode(gpu_device, [c[1] for c in CASES], on=False)
    eng.close()
    assert (info[:, 0] == -1).all(), info[:, 0]


def test_mixed_batch_through_the_backend(gpu_device):
    """B = 16 of JPEGs, a PNG, lossless and lossy WebPs: webp="device" gives the views of
    webp="host" bit for bit on both routes; "off" gives zeros for the WebPs and the views of a
    run without the option everywhere else."""
    by = {c[0]: c[1] for c in CASES}
    uniq = [make_jpeg(160 + 8 * s, 120 + 4 * s, s) for s in range(5)]
    B, nb = 16, 3
    batches = [[uniq[(k + i) % 5] for i in range(B)] for k in range(nb)]
    webps = {1: "gradient_m6", 4: "colours16_19", 6: "lossy", 9: "groups_128x96", 12: "rgba_exact", 14: "flat_70x130"}
    for i, n in webps.items():
        batches[1][i] = by[n]
    batches[1][3] = {c[0]: c[1] for c in pc.cases()}["palette"]
    (side, st), (direct, _) = (_run_backend(batches, r, png="device", webp="device") for r in ("side", "device"))
    (host, sth), (off, sto) = _run_backend(batches, "side", png="device", webp="host"), _run_backend(batches, "side", png="device", webp="off")
    plain, _ = _run_backend(batches, "side", png="device")
    assert st["webp_device"] == 5 and st["webp_host"] == 1 and st["host_decoded"] == 1 and st["side_decoded"] == 6, st
    assert sth["webp_device"] == 0 and sth["webp_host"] == 6 and sth["host_decoded"] == 6, sth
    assert sto["webp_device"] == 0 and sto["webp_host"] == 0 and sto["host_decoded"] == 0, sto
    for k in range(nb):
        for name in side[k]:
            assert torch.equal(side[k][name], direct[k][name]) and torch.equal(side[k][name], host[k][name]), (k, name)
            assert torch.equal(off[k][name], plain[k][name]), (k, name)
    for name in side[1]:
        for i in range(B):
            if i in webps:
                assert side[1][name][i].any() and not off[1][name][i].any(), (name, i)
            else:
                assert torch.equal(side[1][name][i], off[1][name][i]), (name, i)

"""PNG bit depths 1 / 2 / 4 / 16 and Adam7 on the device (``png_forms="all"``): the files of
tests/png_forms_cases.py against Pillow bit for bit; the option off; a mixed batch on both routes."""

import numpy as np
import pytest
import torch

from dataloader_amd import fallback
from dataloader_amd.engine import IngestEngine
from dataloader_amd.synthetic import make_jpeg
from dataloader_amd.tario import spans_of
from tests import png_cases as pc
from tests import png_forms_cases as fc
from tests.test_gpu_parity import _to_dev
from tests.test_gpu_png import _run_backend
from tests.test_png_forms_cpu import model_decode

pytestmark = pytest.mark.gpu

CASES = fc.cases()
FILES = [c[1] for c in CASES]


def _engine(dev, forms):
    eng = IngestEngine(dev, max_batch=len(FILES), max_views=10, max_crop_size=224)
    eng.set_png(True)
    if forms:
        eng.set_png_forms(True)
    ptrs, lens, _keep = spans_of(FILES)
    eng.reserve(int(fallback.probe_png_forms(ptrs, lens)[1].sum()) + (1 << 20), 0)
    return eng


def test_case_list_twice_bit_exact_with_pillow(gpu_device):
    eng = _engine(gpu_device, True)
    d_bytes, d_off = _to_dev(FILES, gpu_device)
    bad = []
    for rnd in range(2):
        info = eng.decode(d_bytes, d_off, len(FILES)).cpu().numpy()
        for i, (name, data, expect) in enumerate(CASES):
            m = model_decode(data)[0]
            want = int(m[0]) if m[3] else 1  # (a file the option does not take stays declined)
            if int(info[i, 0]) != want:
                bad.append((rnd, name, "status", int(info[i, 0]), "model", want))
            elif expect == "dev":
                ref = pc.pillow_rgb(data)
                got = eng.copy_rgb(i, ref.shape[1], ref.shape[0]).cpu().numpy()
                if tuple(info[i, 1:3]) != ref.shape[1::-1] or not np.array_equal(got, ref):
                    bad.append((rnd, name, int((got != ref).sum())))
    eng.close()
    assert not bad, bad[:20]


def test_option_off_declines_every_form(gpu_device):
    eng = _engine(gpu_device, False)
    d_bytes, d_off = _to_dev(FILES, gpu_device)
    info = eng.decode(d_bytes, d_off, len(FILES)).cpu().numpy()
    eng.close()
    assert (info[:, 0] == 1).all(), info[:, 0]


def test_mixed_batch_through_the_backend(gpu_device):
    """B = 16 of JPEGs, plain and extended PNGs and an APNG: png_forms="all" gives the views of
    png="host" bit for bit on both routes and moves the extended files to png_device."""
    by = {c[0]: c[1] for c in CASES}
    plain = {c[0]: c[1] for c in pc.cases()}
    uniq = [make_jpeg(160 + 8 * s, 120 + 4 * s, s) for s in range(5)]
    B, nb = 16, 3
    batches = [[uniq[(k + i) % 5] for i in range(B)] for k in range(nb)]
    ext = {1: "a7_c2d8_33x70", 3: "c0d16_70x65", 5: "a7_c3d4_130x5", 8: "c3d2_70x65", 10: "a7_c6d16_13x17",
           12: "gray16_every_value", 15: "c0d1_filter5"}
    for i, n in ext.items():
        batches[1][i] = by[n]
    for i, n in {2: "zlib_300x200", 7: "palette", 13: "apng"}.items():
        batches[1][i] = plain[n]
    (side, st), (direct, _) = (_run_backend(batches, r, png="device", png_forms="all") for r in ("side", "device"))
    (host, _), (off, sto) = _run_backend(batches, "side", png="host"), _run_backend(batches, "side", png="device")
    # filter5 is taken by the device (status -1: zeros, no container comes back from the side pool); the APNG is Pillow's
    assert st["png_device"] == 9 and st["png_host"] == 1 and st["host_decoded"] == 1 and st["side_decoded"] == 8, st
    assert sto["png_device"] == 2 and sto["png_host"] == 8 and sto["host_decoded"] == 8, sto
    for k in range(nb):
        for name in side[k]:
            for other in (direct, host, off):
                assert torch.equal(side[k][name], other[k][name]), (k, name)
    assert all(side[1][name][i].any() for name in side[1] for i in ext if ext[i] != "c0d1_filter5")

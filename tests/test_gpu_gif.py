"""GIF on the device (``gif="device"``): the files of tests/gif_cases.py against Pillow bit for bit,
the option off, a mixed batch decoded twice on one context, and the backend under every mode."""

from pathlib import Path

import numpy as np
import pytest
import torch

from dataloader_amd import fallback
from dataloader_amd.engine import IngestEngine
from dataloader_amd.synthetic import make_jpeg
from dataloader_amd.tario import spans_of
from tests import gif_cases as gc
from tests import png_cases as pc
from tests.test_gpu_parity import _to_dev
from tests.test_gpu_png import _run_backend

pytestmark = pytest.mark.gpu

CASES = gc.cases()
WANT = {"dev": 0, "corrupt": -1, "declined": 1, "none": -1}


def _engine(dev, files, on=True):
    eng = IngestEngine(dev, max_batch=len(files), max_views=10, max_crop_size=224)
    eng.set_gif(on)
    ptrs, lens, _keep = spans_of(files)
    eng.reserve(int(fallback.probe_gif(ptrs, lens)[1].sum()) + (64 << 20), 0)
    return eng


def _check(eng, dev, files, expect):
    d_bytes, d_off = _to_dev(files, dev)
    info = eng.decode(d_bytes, d_off, len(files)).cpu().numpy()
    bad = []
    for i, (data, want) in enumerate(zip(files, expect)):
        if int(info[i, 0]) != want:
            bad.append((i, "status", int(info[i, 0]), want))
        elif want == 0 and data[:2] != b"\xff\xd8":  # (the JPEGs: tests/test_gpu_parity.py)
            ref = pc.pillow_rgb(data)
            got = eng.copy_rgb(i, ref.shape[1], ref.shape[0]).cpu().numpy()
            if tuple(info[i, 1:3]) != ref.shape[1::-1] or not np.array_equal(got, ref):
                bad.append((i, "pixels", int((got != ref).sum())))
    return bad


def test_case_list_bit_exact_with_pillow(gpu_device):
    """Every case in one batch, the corrupt and declined ones between sound ones."""
    files = [c[1] for c in CASES]
    eng = _engine(gpu_device, files)
    bad = _check(eng, gpu_device, files, [WANT[c[2]] for c in CASES])
    eng.close()
    assert not bad, [(CASES[b[0]][0],) + b[1:] for b in bad]


def test_option_off_leaves_every_gif_corrupt(gpu_device):
    files = [c[1] for c in CASES]
    eng = _engine(gpu_device, files, on=False)
    d_bytes, d_off = _to_dev(files, gpu_device)
    info = eng.decode(d_bytes, d_off, len(files)).cpu().numpy()
    eng.close()
    assert (info[:, 0] == -1).all(), info[:, 0]


def test_mixed_batch_twice_on_one_context(gpu_device):
    """Baseline JPEG, progressive JPEG, a PNG and GIFs, decoded twice on one context: a table
    entry or a stream left over from the first pass would show in the second."""
    by = {c[0]: c[1] for c in CASES}
    prog = (Path(__file__).resolve().parent / "golden" / "prog_640x480.jpg").read_bytes()
    png = {c[0]: c[1] for c in pc.cases()}["palette"]
    names = ["noise256_96x80", "flat_200x100", "early_end_code", "lace_pillow_37x50", "deferred_clear", "kwkwk_chain"]
    files = [make_jpeg(64, 48, 2), by[names[0]], prog, png] + [by[n] for n in names[1:]]
    eng = _engine(gpu_device, files)
    eng.set_png(True)
    want = [0, 0, 0, 0, 0, -1, 0, 0, 0]
    for _ in range(2):
        bad = _check(eng, gpu_device, files, want)
        assert not bad, bad
    eng.close()


def test_backend_modes(gpu_device):
    """B = 16 from a host list source, a batch with GIFs between two plain ones: gif="device" gives
    the views of gif="host" bit for bit on the side route and on multiscan_route="device"; the
    counts are right; gif="off" gives zeros for the GIFs and the same views elsewhere."""
    by = {c[0]: c[1] for c in CASES}
    gifs = {1: "noise256_96x80", 4: "flat_200x100", 6: "no_table", 9: "lace_pillow_37x50", 12: "animation3", 14: "sub_screen_frame"}
    uniq = [make_jpeg(160 + 8 * s, 120 + 4 * s, s) for s in range(5)]
    B, nb = 16, 3
    batches = [[uniq[(k + i) % 5] for i in range(B)] for k in range(nb)]
    for i, n in gifs.items():
        batches[1][i] = by[n]
    (side, st), (direct, _) = (_run_backend(batches, r, gif="device") for r in ("side", "device"))
    (host, sth), (off, sto) = _run_backend(batches, "side", gif="host"), _run_backend(batches, "side")
    assert st["gif_device"] == 4 and st["gif_host"] == 2 and st["host_decoded"] == 2 and st["side_decoded"] == 4, st
    assert sth["gif_device"] == 0 and sth["gif_host"] == 6 and sth["host_decoded"] == 6, sth
    assert sto["gif_device"] == 0 and sto["gif_host"] == 0 and sto["host_decoded"] == 0, sto
    for k in range(nb):
        for name in side[k]:
            assert torch.equal(side[k][name], direct[k][name]) and torch.equal(side[k][name], host[k][name]), (k, name)
            for i in range(B):
                if k == 1 and i in gifs:
                    assert side[k][name][i].any() and not off[k][name][i].any(), (name, i)
                else:
                    assert torch.equal(side[k][name][i], off[k][name][i]), (k, name, i)

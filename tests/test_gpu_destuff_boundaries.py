"""GPU: k_destuff_count / k_destuff_write on the files of tests/destuff_cases.py: FF 00, RSTn,
a fill byte before a stuffed 0xFF, fill runs of 3 and 4100 before RSTn, and EOI, each with its
0xFF at offset -2, -1, 0 and +1 from a chunk, a tile and the first two 32 KiB part boundaries,
at leads 0, 1 and 15 (EOI and a lone trailing 0xFF on a part's first byte: all 16); scans cut
short whose last part holds no byte; bytes after EOI.

One decode per lead over an exact-size buffer.  For every file, bit for bit against the plain
reference destuffer of that module: ent_len, n_rst, terminated and rst_bad of the descriptor
(dino_debug_region 0, field offsets from the emulator build's offsetof), the destuffed bytes and
the 64 zero bytes after them (region 8), the restart offsets (region 9); an accepted file's
pixels equal Pillow's decode of the unshifted file (which test_destuff_cases_cpu.py holds equal
to Pillow's decode of the file itself); a rejected file has status TRUNCATED."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from dataloader_amd.config import DINOAugConfig
from dataloader_amd.engine import IngestEngine, pack_jpegs
from dataloader_amd.params import OUT_FP32, make_aug_config
from tests import destuff_cases as dc

pytestmark = pytest.mark.gpu

FIELDS = ("status", "scan_off", "scan_len", "ent_len", "n_rst", "terminated", "rst_bad", "sizeof")


@pytest.fixture(scope="module")
def layout(emu):
    out = np.zeros(len(FIELDS), np.int32)
    emu.emu_desc_layout(out.ctypes.data_as(ctypes.c_void_p))
    return {k: int(v) for k, v in zip(FIELDS, out)}


def _to_dev(entries, device):
    buf, off = pack_jpegs(entries, pin=False)
    d_bytes = buf.to(device)[: int(off[-1])].clone()  # exact size: no slack after the last image
    assert d_bytes.data_ptr() % 16 == 0
    return d_bytes, off.to(device)


@pytest.mark.parametrize("lead", dc.LEADS16)
def test_destuff_at_boundaries(gpu_device, layout, lead):
    cases = dc.cases_of_lead(lead)
    entries, positions = dc.batch_of_lead(lead)
    pixels = dc.base_pixels()
    eng = IngestEngine(gpu_device, max_batch=len(entries), max_views=1, max_crop_size=32)
    d_bytes, d_off = _to_dev(entries, gpu_device)
    info = eng.decode(d_bytes, d_off, len(entries)).cpu().numpy()
    bad = []
    for c, i in zip(cases, positions):
        assert info[i - 1, 0] < 0  # the dummy entry in front
        ref = dc.ref_destuff(c.scan)
        desc = eng.debug_region(i, 0, layout["sizeof"]).cpu().numpy()
        f = {k: int(desc[layout[k]:layout[k] + 4].view(np.int32)[0]) for k in FIELDS[:-1]}
        want = {"status": c.status, "scan_off": dc.scan_offset(c.jpeg), "scan_len": len(c.scan),
                "ent_len": len(ref.data), "n_rst": len(ref.rst), "terminated": int(ref.terminated), "rst_bad": 0}
        if f != want or info[i, 0] != c.status:
            bad.append((c.name, "descriptor", {k: (f[k], want[k]) for k in f if f[k] != want[k]}))
            continue
        if c.status != 0:
            continue
        n = len(ref.data)
        got = eng.debug_region(i, 8, n + 64).cpu().numpy()
        if got[:n].tobytes() != ref.data:
            first = int(np.flatnonzero(got[:n] != np.frombuffer(ref.data, np.uint8))[0])
            bad.append((c.name, "bytes", first))
        if got[n:].any():
            bad.append((c.name, "zero pad", int(np.flatnonzero(got[n:])[0])))
        rst = eng.debug_region(i, 9, 4 * len(ref.rst) + 4).cpu().numpy()[:4 * len(ref.rst)].view(np.int32)
        if tuple(int(x) for x in rst) != ref.rst:
            bad.append((c.name, "restart offsets", rst.tolist()))
        want_px = pixels[c.base]
        rgb = eng.copy_rgb(i, want_px.shape[1], want_px.shape[0]).cpu().numpy()
        if (int(info[i, 1]), int(info[i, 2])) != want_px.shape[1::-1] or not np.array_equal(rgb, want_px):
            bad.append((c.name, "pixels", int((rgb != want_px).sum())))
    eng.close()
    assert not bad, f"lead {lead}: {len(bad)} of {len(cases)} files differ: {bad[:8]}"


def test_rejected_file_gives_zero_views(gpu_device):
    """An unterminated scan whose last part holds no byte, through dino_run_batch: TRUNCATED, every
    view zero; the accepted file beside it is not."""
    cases = {c.name: c for c in dc.cases_of_lead(0)}
    cut, good = cases["cut_part1_n-15_lead0"], cases["ffd9_part1+0_lead0"]
    entries = []
    for c in (cut, good):
        entries += [b"\0" * (-(sum(map(len, entries)) + dc.scan_offset(c.jpeg)) % 16), c.jpeg]
    cfg = DINOAugConfig(global_crop_size=32, local_crop_size=16, n_local_crops=2)
    eng = IngestEngine(gpu_device, max_batch=len(entries), max_views=cfg.n_views, max_crop_size=32)
    d_bytes, d_off = _to_dev(entries, gpu_device)
    views, info = eng.run_batch(d_bytes, d_off, len(entries), make_aug_config(cfg, 32, 16, OUT_FP32), seed=3,
                                batch_index=0)
    torch.cuda.synchronize()
    st = info[:, 0].cpu().numpy()
    assert st[1] == dc.TRUNCATED and st[3] == 0, st
    for v in views:
        assert torch.count_nonzero(v[1]) == 0
        assert torch.count_nonzero(v[3]) > 0
    eng.close()

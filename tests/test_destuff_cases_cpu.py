"""CPU: the files of tests/destuff_cases.py are what they claim to be.

For every file: its pattern's 0xFF is at the stated scan index (the boundary's index for the
file's lead plus the offset); Pillow decodes it to the pixels of the unshifted base file, or
raises where the file is a rejected one; and the plain reference destuffer of that module
agrees with the emulator's model_destuff (bytes, zero pad, restart offsets, terminated, no
restart marker out of sequence).  Every (boundary, offset, pattern, lead) must be there: a
missing one fails, nothing is skipped."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from oracle import cpu_ref
from tests import destuff_cases as dc

P = ctypes.c_void_p


def emu_destuff(emu, scan: bytes):
    emu.emu_destuff.restype = ctypes.c_int64
    buf = np.frombuffer(scan, np.uint8)
    out = np.full(len(scan) + 96, 0xAA, np.uint8)
    rst = np.zeros(64, np.int32)
    info = np.zeros(4, np.int32)
    n = emu.emu_destuff(buf.ctypes.data_as(P), len(scan), out.ctypes.data_as(P), ctypes.c_int64(out.size),
                        rst.ctypes.data_as(P), rst.size, info.ctypes.data_as(P))
    assert n <= out.size and info[1] <= rst.size
    return out[:n].tobytes(), tuple(int(x) for x in rst[:info[1]]), [int(x) for x in info]


def test_every_target_is_attained():
    got = [c.key for c in dc.all_cases() if c.key]
    assert len(got) == len(set(got))
    assert set(got) == dc.target_keys()
    names = {c.name for c in dc.all_cases()}
    for p in (1, 2):
        assert all(f"lone_ff_part{p}_lead{lead}" in names for lead in dc.LEADS16)
        for lead in dc.LEADS3:
            for d in {-16, -15, -lead, -lead + 1}:
                assert f"cut_part{p}_n{d:+d}_lead{lead}" in names
    assert all(f"junk_{b}_lead{lead}" in names for b in ("mid", "mid2") for lead in dc.LEADS3)
    assert len(dc.all_cases()) <= 700 and max(len(c.jpeg) for c in dc.all_cases()) <= 92 * 1024


def test_reference_destuffer_on_hand_made_scans():
    r = dc.ref_destuff
    assert r(b"") == dc.Destuffed(b"", (), 0, False, False)
    assert r(b"ab\xff\x00c\xff\xd9zz") == dc.Destuffed(b"ab\xffc", (), 5, True, False)
    assert r(b"a\xff\xff\xff\x00b\xff\xff\xd0c\xff\xd1\xff\xff\xd9") == dc.Destuffed(b"a\xffbc", (3, 4), 13, True, False)
    assert r(b"a\xff\xd1b") == dc.Destuffed(b"ab", (1,), 4, False, True)
    assert r(b"ab\xff") == dc.Destuffed(b"ab", (), 2, False, False)
    assert r(b"ab\xff\xff\xff") == dc.Destuffed(b"ab", (), 4, False, False)
    assert r(b"\xff\xc4") == dc.Destuffed(b"", (), 0, True, False)


@pytest.mark.parametrize("lead", dc.LEADS16)
def test_cases_of_lead(emu, lead):
    pixels = dc.base_pixels()
    entries, positions = dc.batch_of_lead(lead)
    starts = np.concatenate([[0], np.cumsum([len(e) for e in entries])])
    cases = dc.cases_of_lead(lead)
    assert len(cases) >= 18
    for c, pos in zip(cases, positions):
        off = dc.scan_offset(c.jpeg)
        scan = c.jpeg[off:]
        assert (int(starts[pos]) + off) % 16 == lead, c.name
        # the pattern, where the name says
        if c.key:
            kind, offset, _, klead = c.key
            assert klead == lead and c.index == dc.BOUNDARIES[kind] - lead + offset, c.name
        if c.at:
            assert scan[c.index:c.index + len(c.at)] == c.at, c.name
            assert scan[c.index - c.run + 1:c.index + 1] == b"\xff" * c.run and scan[c.index - c.run] != 0xFF, c.name
        # the reference destuffer: the terminator's index, and the emulator's model
        ref = dc.ref_destuff(scan)
        e_bytes, e_rst, (e_len, e_nrst, e_term, e_bad) = emu_destuff(emu, scan)
        assert e_len == len(ref.data) and e_bytes[:e_len] == ref.data, c.name
        assert len(e_bytes) == (e_len + 15) // 16 * 16 + 64 and not any(e_bytes[e_len:]), c.name
        assert (e_rst, e_nrst, bool(e_term), e_bad) == (ref.rst, len(ref.rst), ref.terminated, 0), c.name
        assert not ref.rst_bad, c.name
        b = dc.bases()[c.base]
        img = cpu_ref.decode_rgb(c.jpeg)
        if c.status == 0:
            assert ref.terminated and ref.term == (c.index if c.at == b"\xff\xd9" else len(scan) - 2), c.name
            assert ref.data == dc.ref_destuff(b.scan).data and len(ref.rst) == len(b.rsts), c.name
            assert img is not None and np.array_equal(np.asarray(img), pixels[c.base]), c.name
        else:
            assert not ref.terminated and ref.term == c.index and img is None, c.name

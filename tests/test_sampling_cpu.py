"""Chroma samplings and colour markers outside Pillow's writer, through the host emulator
(the device's parser, Huffman, IDCT and colour code on the CPU) and the host probe.

Every file of ``tests/sampling_cases.py`` decodes in the sequential mode and in a speculative
mode; return value and pixels follow ``oracle.cpu_ref.decode_rgb`` on the same bytes: an image
-> 0 and identical pixels (bit-exact, no tolerance), ``None`` -> a negative status and nothing
written.  ``dino_probe`` reports the status the decode reports.
"""

from __future__ import annotations

import numpy as np
import pytest

from dataloader_amd import fallback
from dataloader_amd.engine import pack_jpegs
from tests import sampling_cases as sc
from tests.helpers import emu_decode

# the speculative mode's lane count: 64 on the small files, 300 on the wide and large ones
SPEC_LANES = {"small": 64, "wide": 300, "route": 300, "restart": 64, "progressive": 64, "markers": 64}


def _check(emu, group, mode, lanes):
    bad = []
    for (name, j), ref in zip(sc.GROUPS[group](), sc.references(group)):
        r, out, _ = emu_decode(emu, j, mode, lanes)
        if ref is None:
            if not (r < 0 and not out.any()):
                bad.append((name, "reference rejects; status", r, "bytes set", int(np.count_nonzero(out))))
        elif r != 0:
            bad.append((name, "status", r))
        elif out.shape != ref.shape:
            bad.append((name, "shape", out.shape, ref.shape))
        elif not np.array_equal(out, ref):
            bad.append((name, int((out != ref).sum())))
    assert not bad, f"{len(bad)} of {len(sc.GROUPS[group]())}: {bad}"


@pytest.mark.parametrize("group", list(sc.GROUPS))
def test_sequential_decode_matches_oracle(emu, group):
    _check(emu, group, 0, 1)


@pytest.mark.parametrize("group", list(sc.GROUPS))
def test_speculative_decode_matches_oracle(emu, group):
    _check(emu, group, 1, SPEC_LANES[group])


@pytest.mark.parametrize("group", list(sc.GROUPS))
def test_probe_reports_the_decode_status(emu, group):
    """``dino_probe`` (the host pre-screen of the same parser): 0 with the reference's size where
    the reference decodes, negative where it zero-fills, and the emulator's decode status."""
    cases = sc.GROUPS[group]()
    buf, off = pack_jpegs([j for _, j in cases], pin=False)
    info, _, _ = fallback.probe(buf.data_ptr(), off.numpy(), len(cases), 0)
    bad = []
    for i, ((name, j), ref) in enumerate(zip(cases, sc.references(group))):
        r = emu_decode(emu, j, 0, 1)[0]
        st = int(info[i, 0])
        if st != r or (ref is None) != (st < 0):
            bad.append((name, "probe", st, "decode", r, "reference", "rejects" if ref is None else "decodes"))
        elif ref is not None and (int(info[i, 1]), int(info[i, 2])) != (ref.shape[1], ref.shape[0]):
            bad.append((name, "size", int(info[i, 1]), int(info[i, 2])))
    assert not bad, bad


def test_rejected_files_are_the_known_ones():
    """The only non-pixel expectations: the layouts libjpeg refuses (more than ten blocks per
    MCU in an interleaved scan, a fractional upsampling ratio) and the "JFIF" APP0 / "Adobe"
    APP14 segments shorter than the version field that Pillow's APP handler reads."""
    rejected = {name for g in sc.GROUPS for (name, _), ref in zip(sc.GROUPS[g](), sc.references(g)) if ref is None}
    want = {f"{lay}_{w}x{h}" for lay in sc.REJECTED_LAYOUTS for (w, h) in sc.SMALL_SIZES}
    want |= {"b12_70x50_simple"}
    want |= {f"{m}_len{n}_{ids}_{s}" for s in ("444", "420") for n in (4, 5, 6)
             for m, ids in (("app0", "rgbids"), ("adobe0", "nojfif"), ("adobe1", "rgbids")) if (m, n) != ("adobe0", 4)
             and (m, n) != ("adobe1", 4)}
    assert rejected == want


def test_route_files_clear_their_thresholds():
    """Each route file's destuffed entropy bytes (and, as they are smaller than the file, the
    file's length) against the lane-plan thresholds, with a margin of 4 %."""
    for name, j in sc.route_cases():
        route = name.split("_")[1]
        n = sc.entropy_bytes(j)
        assert sc.route_of(j) == route, (name, n)
        if route == "huff1":
            assert len(j) <= sc.HUFF1_MAX_BYTES, (name, len(j))
        elif route == "huff3":
            assert n > 1.04 * sc.HUFF1_MAX_BYTES and len(j) <= sc.SEGMENT_BYTES, (name, n, len(j))
        else:
            assert n > 1.03 * sc.SEGMENT_BYTES and len(j) > sc.SEGMENT_BYTES, (name, n, len(j))
    for name, j in sc.restart_cases()[-4:]:
        assert sc.entropy_bytes(j) > sc.HUFF1_MAX_BYTES, name

"""The header walk (``parse_jpeg``, ``prog_walk``) on the files of ``tests/header_cases.py``:
metadata segments, header bytes on the 4096-byte prefix boundary of k_parse, and markers and
lengths on which libjpeg's ``read_markers`` and Pillow's marker loop are stricter or laxer than a
plain segment walk.

For every case, with no tolerance: the declared expectation is what ``oracle.cpu_ref.decode_rgb``
does with the bytes (an image with the stated pixels, or ``None``); ``dino_probe``'s status is 0
where the reference decodes and negative where it raises; the host emulator gives Pillow's pixels
where the reference decodes and a negative status with nothing written where it raises.
"""

from __future__ import annotations

import warnings

import numpy as np
import pytest

from dataloader_amd import fallback
from dataloader_amd.engine import pack_jpegs
from oracle import cpu_ref
from tests import header_cases as hc
from tests.helpers import emu_decode


@pytest.fixture(scope="module")
def pillow():
    """[the oracle's decode of every case]: an array or ``None``."""
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (Pillow warns about the malformed MPF segments it then ignores)
        for c in hc.cases():
            img = cpu_ref.decode_rgb(c.data)
            out.append(None if img is None else np.asarray(img))
    return out


def test_declarations_are_what_pillow_does(pillow):
    refs = hc.references()
    bad = []
    for c, got in zip(hc.cases(), pillow):
        assert c.expect in ("decodes", "raises"), c.name
        if (got is None) != (c.expect == "raises"):
            bad.append((c.name, "declared", c.expect, "Pillow", "raises" if got is None else "decodes"))
        elif got is not None and not np.array_equal(got, refs[c.pixels_of]):
            bad.append((c.name, "pixels differ from", c.pixels_of))
    assert not bad, bad


def test_probe_status_sign_follows_pillow(pillow):
    cases = hc.cases()
    buf, off = pack_jpegs([c.data for c in cases], pin=False)
    info, _, _ = fallback.probe(buf.data_ptr(), off.numpy(), len(cases), 0)
    bad = []
    for i, (c, ref) in enumerate(zip(cases, pillow)):
        st = int(info[i, 0])
        if (ref is None and st >= 0) or (ref is not None and st != 0):
            bad.append((c.name, "probe", st, "reference", "raises" if ref is None else "decodes"))
        elif ref is not None and (int(info[i, 1]), int(info[i, 2])) != (ref.shape[1], ref.shape[0]):
            bad.append((c.name, "size", int(info[i, 1]), int(info[i, 2])))
    assert not bad, f"{len(bad)} of {len(cases)}: {bad}"


@pytest.mark.parametrize("mode,lanes", [(0, 1), (1, 64)])
def test_emulator_matches_pillow(emu, pillow, mode, lanes):
    bad = []
    for c, ref in zip(hc.cases(), pillow):
        r, out, _ = emu_decode(emu, c.data, mode, lanes)
        if ref is None:
            if not (r < 0 and not out.any()):
                bad.append((c.name, "reference raises; status", r, "bytes set", int(np.count_nonzero(out))))
        elif r != 0:
            bad.append((c.name, "status", r))
        elif out.shape != ref.shape or not np.array_equal(out, ref):
            bad.append((c.name, "pixels"))
    assert not bad, f"{len(bad)} of {len(hc.cases())}: {bad}"


# ---- the cases are what they claim -----------------------------------------------------------
def _walk(jpeg: bytes):
    """[(marker, offset of FF, offset after the segment)] up to the first SOS, by a plain segment
    walk of its own (the family (b) files are well-formed)."""
    out, pos = [], 2
    while True:
        assert jpeg[pos] == 0xFF and jpeg[pos + 1] not in (0x00, 0xFF), pos
        n = int.from_bytes(jpeg[pos + 2:pos + 4], "big")
        out.append((jpeg[pos + 1], pos, pos + 2 + n))
        if jpeg[pos + 1] == 0xDA:
            return out
        pos += 2 + n


def test_boundary_cases_sit_on_the_boundary():
    """Every family (b) file has the named byte at the stated offset, found by a walk that does
    not use the builder's layout: a change of an encoder cannot move the cases off 4096."""
    markers = {"sos": (0xDA,), "dht": (0xC4,), "dqt": (0xDB,), "sof": (0xC0, 0xC2)}
    seen = set()
    for c in hc.boundary_cases():
        what, target = c.at
        segs = _walk(c.data)
        if what == "length":
            assert len(c.data) == target, c.name
            assert segs[-1][2] < target, c.name  # the scan header lies inside the prefix
            seen.add((what, target))
            continue
        tag, part = what.split("_")
        a, e = next((a, e) for m, a, e in segs if m in markers[tag])
        want = {"ff": a, "len": a + 2, "mid": (a + e) // 2, "last": e - 1, "end": e}[part]
        assert want == target, (c.name, want)
        if part == "ff":
            assert c.data[target] == 0xFF and c.data[target + 1] in markers[tag], c.name
        if what == "sos_last":
            assert segs[-1][2] == target + 1, c.name  # scan_off
        seen.add((what, target))
    whats = set(hc.boundary_bytes(hc.bases()["b420"]))
    assert whats == {"sos_ff", "sos_len", "sos_last", "dht_ff", "dht_len", "dht_mid", "dqt_ff", "dqt_len", "dqt_mid",
                     "sof_ff", "sof_len", "sof_mid", "sof_end"}
    assert seen == {(w, t) for w in whats for t in hc.BOUNDARY_OFFSETS} | {("length", t) for t in (4095, 4096, 4097)}
    assert len(hc.boundary_cases()) == 2 * len(seen)
    scan_offs = {_walk(c.data)[-1][2] for c in hc.boundary_cases() if c.at[0] == "sos_last"}
    assert scan_offs == {4095, 4096, 4097, 4098}


def test_metadata_cases_are_under_and_over_the_prefix():
    """Family (a): the first SOS header ends before byte 4096 in the ``_under`` files and after it
    in the ``_over`` files; every item has an ``_over`` file and every small item both."""
    by_name = {c.name: c for c in hc.metadata_cases()}
    for name, segs, _ in hc.metadata_items():
        over = by_name[f"{name}_over"].data
        assert _walk(over)[-1][1] > hc.PREFIX, name
        if len(segs) < 3000:
            assert _walk(by_name[f"{name}_under"].data)[-1][2] < hc.PREFIX, name
    assert sum(c.pixels_of == "prog" for c in hc.metadata_cases()) >= 2
    # the long items: what a photograph's header carries
    assert len(by_name["icc_three_full_over"].data) > 190_000 and len(by_name["com_65533_over"].data) > 65_000


def test_every_family_has_its_cases():
    """Nothing is filtered out: the counts follow from the lists; every row of the marker table
    stands at every place that applies."""
    b = hc.bases()
    items = hc.marker_items(b["b420"])
    names = {c.name for c in hc.marker_cases()}
    for name, _, _, _ in items:
        for where, base in (("app0", "b420"), ("dqt_sof", "b420"), ("sof_sos", "b420"), ("scans", "k1")):
            assert f"{name}_{where}_{base}" in names, (name, where)
    assert len(hc.marker_cases()) == 4 * len(items) + 6 + 2 * len(b) + 2 + 2
    assert {c.expect for c in hc.cases()} == {"decodes", "raises"}
    assert len(hc.cases()) == len(hc.metadata_cases()) + len(hc.boundary_cases()) + len(hc.marker_cases())
    # between two scans only libjpeg decides: TEM decodes there and nowhere before the first SOS
    expect = {c.name: c.expect for c in hc.cases()}
    assert expect["tem_scans_k1"] == "decodes" and expect["tem_app0_b420"] == "raises"
    # the three multi-scan layouts really are multi-scan
    assert sum(m == 0xDA for m, _, _ in hc.layout(b["k1"])) == 3
    assert sum(m == 0xDA for m, _, _ in hc.layout(b["prog"])) >= 3 and hc.sof_marker(b["prog"]) == 0xC2

"""Huffman table shapes no encoder in the suite emits (``tests/hufftable_cases.py``) through the
host emulator and the host probe, and the properties that make those files worth decoding on
the device: their tables have the intended lengths, the route files are on their routes, the
bad-code files hold bad codes, the rejected files are the ones expected.

Every file decodes in the sequential mode and in a speculative mode; return value and pixels
follow ``oracle.cpu_ref.decode_rgb`` on the same bytes: an image -> 0 and identical pixels
(bit-exact, no tolerance), ``None`` -> a negative status and nothing written.
"""

from __future__ import annotations

import hashlib

import numpy as np
import pytest

from dataloader_amd import fallback
from dataloader_amd.engine import pack_jpegs
from tests import cmyk_cases as cc
from tests import hufftable_cases as hc
from tests import sampling_cases as sc
from tests.helpers import emu_decode

THREE_COMPONENT_GROUPS = [g for g in hc.GROUPS if g != "four_component"]
SPEC_LANES = {"small": 64, "route": 300, "progressive": 64, "rejected": 64}

# sha256 of the writer's output before it took table_hook / share_tables / table_ids /
# bad_code_every: the defaults change no byte
PARENT_HASHES = {
    "s440_70x50": "9b5c56b0bfc48eaedcfe6c86e260c49f6cf86d91d27a3f864125fc5dbe805c0b",
    "s440_70x50_ri3": "274889bcb353fa3a401d2a14374cecb3d4324d24675593145c6fbb45e80d2cd4",
    "s411_70x50_deep": "fc1cd1c1a3a8fe0bfa01163791d3ab5d56be4142360fe4658901ca0fe5fb765a",
    "ycck_10blk_70x50": "43130f8834cd55245b103cdffa6c3fb8162d4aa782c6b82ecb0354026a51b3f0",
}


def test_default_writer_output_is_unchanged():
    files = {**dict(sc.small_cases()), **dict(sc.restart_cases()), **dict(sc.progressive_cases()), **cc.cases()}
    got = {name: hashlib.sha256(files[name]).hexdigest() for name in PARENT_HASHES}
    assert got == PARENT_HASHES


def _check(emu, group, mode, lanes):
    bad = []
    for (name, j), ref in zip(hc.GROUPS[group](), hc.references(group)):
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
    assert not bad, f"{len(bad)} of {len(hc.GROUPS[group]())}: {bad}"


@pytest.mark.parametrize("group", THREE_COMPONENT_GROUPS)
def test_sequential_decode_matches_oracle(emu, group):
    _check(emu, group, 0, 1)


@pytest.mark.parametrize("group", THREE_COMPONENT_GROUPS)
def test_speculative_decode_matches_oracle(emu, group):
    _check(emu, group, 1, SPEC_LANES[group])


def test_four_component_model_matches_oracle():
    """The four-component files go through the host model of the coefficient-buffer path with
    the option on (it has the one, sequential, mode)."""
    emu4 = cc.build_emu4()
    for (name, j), ref in zip(hc.four_component_cases(), hc.references("four_component")):
        st, got = cc.emu4_decode(emu4, j, 70, 50)
        assert ref is not None and st == 0 and np.array_equal(got, ref), name


@pytest.mark.parametrize("group", list(hc.GROUPS))
def test_probe_reports_the_decode_status(emu, group):
    """``dino_probe``: the emulator's decode status, 0 with the reference's size where the
    reference decodes and negative where it zero-fills; a four-component file is status 1 of
    kind 3 (decodable with the option on)."""
    cases = hc.GROUPS[group]()
    buf, off = pack_jpegs([j for _, j in cases], pin=False)
    info, _, _ = fallback.probe(buf.data_ptr(), off.numpy(), len(cases), 0)
    bad = []
    for i, ((name, j), ref) in enumerate(zip(cases, hc.references(group))):
        st = int(info[i, 0])
        if group == "four_component":
            if (st, int(info[i, 1]), int(info[i, 2]), int(info[i, 3])) != (1, 70, 50, 3):
                bad.append((name, info[i].tolist()))
            continue
        r = emu_decode(emu, j, 0, 1)[0]
        if st != r or (ref is None) != (st < 0):
            bad.append((name, "probe", st, "decode", r, "reference", "rejects" if ref is None else "decodes"))
        elif ref is not None and (int(info[i, 1]), int(info[i, 2])) != (ref.shape[1], ref.shape[0]):
            bad.append((name, "size", int(info[i, 1]), int(info[i, 2])))
    assert not bad, bad


# ---- the cases are what they claim -----------------------------------------------------
def _dht_histograms(jpeg: bytes):
    """[(class, id, [number of codes of length 1..16])] of every DHT table of the file, scans
    after the first included (a marker walk of its own: not the code under test)."""
    out, pos = [], 2
    while pos + 4 <= len(jpeg):
        assert jpeg[pos] == 0xFF, pos
        m = jpeg[pos + 1]
        if m == 0xD9:
            break
        n = int.from_bytes(jpeg[pos + 2:pos + 4], "big")
        if m == 0xC4:
            q = pos + 4
            while q < pos + 2 + n:
                bits = list(jpeg[q + 1:q + 17])
                out.append((jpeg[q] >> 4, jpeg[q] & 15, bits))
                q += 17 + sum(bits)
        pos += 2 + n
        if m == 0xDA:  # entropy data: up to the next marker that is neither stuffing nor RSTn
            while not (jpeg[pos] == 0xFF and jpeg[pos + 1] != 0 and not 0xD0 <= jpeg[pos + 1] <= 0xD7):
                pos += 1
    return out


def _shaped_cases():
    for group in ("small", "route", "progressive", "four_component"):
        for name, j in hc.GROUPS[group]():
            yield group, name, j, hc.meta(name)


def test_tables_have_the_intended_length_histogram():
    """all(L): n codes of L bits; cliff / revcliff (k, L): one code each of 1..k bits, the rest at
    L; 16 in place of L only where the table cannot hold its symbols, only for the shapes the
    case list names, and exactly where the hook recorded it.  Each of those shapes still has
    tables at its own L (the fallback did not swallow the shape)."""
    bad, own_level, checked = [], set(), 0
    for _, name, j, m in _shaped_cases():
        shape = m["shape"]
        if shape[0] not in ("all", "cliff", "revcliff"):
            continue
        fell_tables = 0
        for tc, th, bits in _dht_histograms(j):
            n = sum(bits)
            k, L = (0, shape[1]) if shape[0] == "all" else (shape[1], shape[2])
            fell = n - k > (1 << (L - k)) - 1
            want = [0] * 16
            for ln in range(1, min(k, n) + 1):
                want[ln - 1] = 1
            if n > k:
                want[(16 if fell else L) - 1] += n - k
                if not fell:
                    own_level.add(shape)
            fell_tables += fell
            checked += 1
            if bits != want:
                bad.append((name, tc, th, bits, want))
        if fell_tables and shape not in hc.MAY_FALL_BACK:
            bad.append((name, "fell back to 16"))
        if fell_tables != len(m["fallbacks"]):
            bad.append((name, "fallbacks", fell_tables, m["fallbacks"]))
    assert not bad, bad
    assert checked >= 6 * 4 * (len(hc.SHAPES) - 2)  # six tables a colour file
    assert own_level >= {s for s in hc.SHAPES if s[0] != "optimal" and s[0] != "inverted"}


def test_inverted_tables_put_the_longest_code_on_the_most_frequent_symbol():
    """The inverted AC tables of a route file reach past the 11-bit lookahead, and the entropy
    data is more than twice that of the same image under the writer's optimal tables, which
    stays on k_huff1."""
    files = dict(hc.route_cases())
    j = files["inverted_huff3_320x240"]
    assert max(ln + 1 for tc, _, bits in _dht_histograms(j) if tc == 1 for ln in range(16) if bits[ln]) > 11
    plain = hc.jw.encode(hc._route_image(320, 240), hc.ONE_SCAN, samp=hc.S444, quality=hc.ROUTE_QUALITY)
    assert sc.route_of(plain) == "huff1" and sc.entropy_bytes(j) > 2 * sc.entropy_bytes(plain)


def test_route_files_clear_their_thresholds(capsys):
    """Destuffed entropy bytes against the lane-plan thresholds with the margins of
    test_sampling_cpu (4 % past k_huff1's limit, 3 % past one segment)."""
    cases = hc.route_cases()
    assert len(cases) == 2 * len(hc.ROUTE_SHAPES) + 1
    with capsys.disabled():
        for name, j in cases:
            print(f"\n  {name}: {sc.entropy_bytes(j)} entropy bytes, {len(j)} file bytes, {sc.route_of(j)}", end="")
    for name, j in cases:
        route = name.split("_huff")[1][0]
        n = sc.entropy_bytes(j)
        assert sc.route_of(j) == "huff" + route, (name, n)
        if route == "3":
            assert n > 1.04 * sc.HUFF1_MAX_BYTES and len(j) <= sc.SEGMENT_BYTES, (name, n, len(j))
        else:
            assert n > 1.03 * sc.SEGMENT_BYTES and len(j) > sc.SEGMENT_BYTES, (name, n, len(j))
        assert len(j) < 400 * 1024, (name, len(j))
    assert b"\xff\xdd" in cases[-1][1] and cases[-1][1].count(b"\xff\xd0") >= 3


def test_bad_code_files_hold_bad_codes():
    """The writer's count, and the bytes: 17 one-bits put at least one stuffed FF (FF 00) into
    the entropy data whatever the bit phase."""
    names = [n for g, n, _, _ in _shaped_cases() if n.startswith("bad")]
    assert len(names) == 2 * 3 * 4 + 3
    files = dict(hc.small_cases())
    for n in names:
        count = hc.meta(n)["bad_codes"]
        assert count >= 1, n
        assert files[n].count(b"\xff\x00") >= 1, n
        if n.startswith("bad1_"):  # every symbol 0: at least one (EOB or a zero DC difference) in most blocks
            twin = hc.meta(n.replace("bad1_", "bad5_"))["bad_codes"]
            assert count >= 5 * twin, (n, count, twin)
    assert all(hc.meta(n)["bad_codes"] == 0 for _, n, _, _ in _shaped_cases() if not n.startswith("bad"))


REJECTED = {"oversub_dc0_70x50", "oversub_ac1_70x50", "allones_dc1_70x50", "allones_ac0_70x50", "dc16_dc0_70x50",
            "dc16_dc2_70x50", "sum257_ac0_70x50", "sum257_dc1_70x50",
            # libjpeg checks the count total when it reads a DHT; the code assignment and the DC
            # values only for tables a scan uses: the other unused-table files decode
            "sum257_unused_ac3_70x50", "sum257_unused_dc3_70x50"}


def test_rejected_files_are_the_known_ones():
    rejected = {name for g in hc.GROUPS for (name, _), ref in zip(hc.GROUPS[g](), hc.references(g)) if ref is None}
    assert rejected == REJECTED
    decoded = {name for (name, _), ref in zip(hc.rejected_cases(), hc.references("rejected")) if ref is not None}
    assert decoded == {"valid_70x50", "oversub_unused_ac3_70x50", "allones_unused_dc3_70x50", "dc16_unused_dc3_70x50"}
    # the unused tables change no pixel
    refs = dict(zip((n for n, _ in hc.rejected_cases()), hc.references("rejected")))
    assert all(np.array_equal(refs[n], refs["valid_70x50"]) for n in decoded)


def test_every_group_has_its_cases():
    """Nothing is filtered out: the counts follow from the case lists."""
    per_image = len(hc.SHAPES) - 1 + 2 * 3 + 2 * len(hc.BAD_CODE_SHAPES)
    assert len(hc.small_cases()) == 4 * per_image + len(hc.SHAPES) - 1 + len(hc.BAD_CODE_SHAPES)
    assert len(hc.progressive_cases()) == 2 * len(hc.PROGRESSIVE_SHAPES)
    assert len(hc.four_component_cases()) == 4
    assert len(hc.rejected_cases()) == 1 + len(hc.REJECT_USED) + len(hc.REJECT_UNUSED)
    names = [n for g in hc.GROUPS for n, _ in hc.GROUPS[g]()]
    assert len(set(names)) == len(names)

"""CPU: which 32 KiB part of a scan writes and which completes the descriptor in k_destuff_write
(csrc/plan.hpp ds_part_role, through the emulator).

Part p of an image covers scan indices [p 32768 - lead, (p + 1) 32768 - lead); E is the first
terminating marker's index, n (the scan's length) when there is none.  Swept over every lead,
lengths around one and two parts and every E within 17 bytes of a part boundary:

  * exactly one part finalises (ent_len, n_rst, terminated, TRUNCATED, the zero pad);
  * the parts that write cover [0, min(E, n)) with no gap and no overlap;
  * every part before the finaliser lies wholly below E, so that the finaliser's output offset,
    the sum of their counts, is the stream's length up to its own bytes; no part after it writes.

The condition this function replaced is restated below in Python: it left two families of
inputs without a finaliser, so their descriptors kept whatever ent_len they held with status OK
(a terminator on a part's first byte, p >= 1: for a valid file (scan_len - 2 + lead) % 32768 == 0)
or were never marked TRUNCATED (an unterminated scan with n + lead <= 32768 p < n + 16, whose last
part holds no byte)."""

from __future__ import annotations

import ctypes

import numpy as np

PART = 32768
LENGTHS = sorted({1, 15, 16, 17, *range(PART - 40, PART + 41), *range(2 * PART - 40, 2 * PART + 41)})


def _sweep(emu):
    emu.emu_ds_parts.restype = ctypes.c_int
    for lead in range(16):
        for n in LENGTHS:
            items = emu.emu_ds_parts(n)
            assert items == max(1, -(-(n + 16) // PART))
            near = {p * PART - lead + d for p in range(items + 1) for d in range(-17, 18)}
            for E in sorted({n} | {e for e in near if 0 <= e < n}):
                yield lead, n, E, items


def _roles(emu, lead, n, E, items):
    out = np.zeros(2 * items, np.uint8)
    emu.emu_ds_part_roles(lead, n, E, items, out.ctypes.data_as(ctypes.c_void_p))
    return [(bool(out[2 * p]), bool(out[2 * p + 1])) for p in range(items)]


def _parent_roles(lead, n, E, items):
    """The condition before ds_part_role: `last` was looked at only by a part that ran."""
    out = []
    for part in range(items):
        k0 = part * PART - lead
        k1 = k0 + PART
        runs = k0 < E or part == 0
        last = (k0 <= E < k1) if E < n else part == items - 1
        out.append((runs, runs and last))
    return out


def _check(roles, lead, n, E):
    fin = [p for p, (_, f) in enumerate(roles) if f]
    assert len(fin) == 1, f"finalisers {fin}"
    at = 0  # the writers' ranges, clipped at E and n, tile [0, min(E, n))
    for p, (writes, _) in enumerate(roles):
        k0, k1 = max(p * PART - lead, 0), min((p + 1) * PART - lead, E, n)
        if writes and k1 > k0:
            assert k0 == at, f"part {p} starts at {k0}, covered up to {at}"
            at = k1
        if p < fin[0]:
            assert min((p + 1) * PART - lead, n) <= E, f"part {p} before the finaliser holds bytes at or after E"
        if p > fin[0]:
            assert not writes, f"part {p} after the finaliser writes"
    assert at == min(E, n), f"covered up to {at}"


def test_one_finaliser_and_a_tiling(emu):
    count = 0
    for lead, n, E, items in _sweep(emu):
        try:
            _check(_roles(emu, lead, n, E, items), lead, n, E)
        except AssertionError as e:
            raise AssertionError(f"lead {lead} n {n} E {E} parts {items}: {e}") from None
        count += 1
    assert count > 100000


def test_parent_condition_left_two_families_without_a_finaliser(emu):
    first_byte, empty_last, other = [], [], []
    for lead, n, E, items in _sweep(emu):
        fin = [p for p, (_, f) in enumerate(_parent_roles(lead, n, E, items)) if f]
        assert len(fin) <= 1
        if fin:
            continue
        if E < n and E + lead >= PART and (E + lead) % PART == 0:
            first_byte.append((lead, n, E))
        elif E == n and n + lead <= (items - 1) * PART < n + 16:
            empty_last.append((lead, n, E))
        else:
            other.append((lead, n, E))
    assert not other, other[:5]
    # both families are there, at every lead that allows them, and ds_part_role closes them (the test above)
    assert {lead for lead, _, _ in first_byte} == set(range(16))
    assert {lead for lead, _, _ in empty_last} == set(range(16))
    # a valid file of the first family: EOI's 0xFF at E = scan_len - 2
    assert any(E == n - 2 for _, n, E in first_byte)
    # a lone trailing 0xFF there is the same hole
    assert any(E == n - 1 for _, n, E in first_byte)
    for lead, n, E in first_byte[:50] + empty_last[:50]:
        items = emu.emu_ds_parts(n)
        assert sum(f for _, f in _roles(emu, lead, n, E, items)) == 1

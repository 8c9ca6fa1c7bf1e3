"""Baseline JPEG files whose 0xFF patterns sit at chosen places relative to the boundaries of the
destuffing pass (TEST INFRASTRUCTURE ONLY; shared by test_destuff_cases_cpu.py and
test_gpu_destuff_boundaries.py).

k_destuff_count / k_destuff_write (csrc/kernels.hip) work on 16-byte chunks (chunk c covers scan
bytes [16 c - lead, 16 c - lead + 16), lead = the scan's address mod 16), tiles of 256 chunks
and parts of 8 tiles; every rule about a 0xFF byte looks at the byte after it, which may belong
to the next lane, tile or part.  Each file here puts the 0xFF of one pattern at boundary + offset
for one boundary (BOUNDARIES), one offset (OFFSETS) and one lead.

Bytes are moved in the two ways the format allows (B.1.1.2: any marker may be preceded by 0xFF
fill bytes): k fill bytes before an RSTn shift everything after them by k, fill bytes before EOI
move EOI.  Pillow decodes such a file to the pixels of the unshifted one, which
test_destuff_cases_cpu.py holds for every file.  One pattern steps outside the standard: FF FF 00,
a fill byte before a stuffed 0xFF, which libjpeg reads as one data 0xFF (jdhuff.c
jpeg_fill_bit_buffer skips 0xFFs after a 0xFF) and so must this decoder.

Nothing is stored in git: Pillow encodes seeded images of ``dataloader_amd.synthetic`` and the
cases are built once per process.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from dataloader_amd.synthetic import encode_jpeg, textured_rgb

CHUNK, TILE, PART = 16, 4096, 32768
# A chunk boundary between two waves of a tile (chunk 1344 = 21 x 64, not a tile's first), a tile
# boundary inside part 0, and the first two part boundaries.  A boundary's scan index is
# BOUNDARIES[kind] - lead.
BOUNDARIES = {"chunk": CHUNK * 1344, "tile": TILE * 6, "part1": PART, "part2": 2 * PART}
OFFSETS = (-2, -1, 0, 1)
LEADS3 = (0, 1, 15)
LEADS16 = tuple(range(16))
# patterns on the restart-interval file; the named 0xFF is the first byte of `at`
RST_PATTERNS = ("ff00", "ffdn", "ffff00", "run3", "run4100")
RUN = {"run3": 3, "run4100": 4100}
JUNK_BYTES = 40000
TRUNCATED = -2  # DINO_IMG_TRUNCATED


# ---- the reference destuffer ------------------------------------------------------------------
@dataclass(frozen=True)
class Destuffed:
    data: bytes        # the entropy-coded bytes without stuffing, fill bytes and markers
    rst: tuple         # per RSTn found: the offset in `data` at which the next interval starts
    term: int          # scan index of the 0xFF whose successor ended the scan; len(scan) if none
    terminated: bool   # a marker ended the scan (not the end of the bytes)
    rst_bad: bool      # an RSTn out of sequence


def ref_destuff(scan: bytes) -> Destuffed:
    """libjpeg's reading of a scan's bytes (jdhuff.c jpeg_fill_bit_buffer, jdmarker.c next_marker),
    one 0xFF at a time: after a 0xFF further 0xFFs are skipped; then 00 keeps one 0xFF as data,
    D0..D7 is a restart marker, anything else ends the scan; a 0xFF (or a run of them) with
    nothing after it is a scan cut short."""
    out, rst, bad, n, k = bytearray(), [], False, len(scan), 0
    while True:
        f = scan.find(b"\xff", k)
        if f < 0:
            out += scan[k:]
            return Destuffed(bytes(out), tuple(rst), n, False, bad)
        out += scan[k:f]
        j = f + 1
        while j < n and scan[j] == 0xFF:
            j += 1
        if j >= n:
            return Destuffed(bytes(out), tuple(rst), n - 1, False, bad)
        c = scan[j]
        if c == 0x00:
            out.append(0xFF)
        elif 0xD0 <= c <= 0xD7:
            bad |= (c & 7) != (len(rst) & 7)
            rst.append(len(out))
        else:
            return Destuffed(bytes(out), tuple(rst), j - 1, True, bad)
        k = j + 1


# ---- base files ---------------------------------------------------------------------------------
def scan_offset(jpeg: bytes) -> int:
    """Offset of the first entropy-coded byte of a one-scan file."""
    k = jpeg.index(b"\xff\xda")
    return k + 2 + int.from_bytes(jpeg[k + 2:k + 4], "big")


@dataclass(frozen=True)
class Base:
    name: str
    jpeg: bytes
    off: int       # scan_offset
    eoi: int       # scan index of EOI's 0xFF
    rsts: tuple    # scan indices of the RSTn markers' 0xFF
    ff00: tuple    # scan indices of the stuffed 0xFFs

    @property
    def head(self) -> bytes:
        return self.jpeg[:self.off]

    @property
    def scan(self) -> bytes:
        return self.jpeg[self.off:]


def _base(name: str, jpeg: bytes) -> Base:
    off = scan_offset(jpeg)
    scan = jpeg[off:]
    assert scan[-2:] == b"\xff\xd9"
    rsts, ff00, k = [], [], scan.find(b"\xff")
    while 0 <= k < len(scan) - 2:
        assert scan[k + 1] == 0x00 or 0xD0 <= scan[k + 1] <= 0xD7, "an encoder's scan: FF 00 and RSTn only"
        (ff00 if scan[k + 1] == 0x00 else rsts).append(k)
        k = scan.find(b"\xff", k + 2)
    return Base(name, jpeg, off, len(scan) - 2, tuple(rsts), tuple(ff00))


@functools.lru_cache(maxsize=None)
def bases() -> dict:
    """200 x 160 noisy quality-98 4:4:4 files of about 78 KB (two part boundaries inside the scan)
    with and without a restart interval of one MCU row, smaller ones of the same kind whose EOI is
    moved up to a boundary by fill bytes, and a 96 x 64 file of little data."""
    rng = np.random.default_rng(2101)
    big = textured_rgb(200, 160, rng, noise=30)
    out = [_base("big", encode_jpeg(big, quality=98, subsampling=0)),
           _base("big_ri", encode_jpeg(big, quality=98, subsampling=0, restart_mcus=25)),
           _base("small", encode_jpeg(textured_rgb(96, 64, rng), quality=85))]
    for name, (w, h) in (("low", (112, 72)), ("mid", (128, 96)), ("mid2", (160, 128))):
        out.append(_base(name, encode_jpeg(textured_rgb(w, h, rng, noise=30), quality=98, subsampling=0)))
    d = {b.name: b for b in out}
    assert d["big"].eoi > 2 * PART + 4200 and d["big_ri"].eoi > 2 * PART + 4200 and len(d["big_ri"].rsts) == 19
    assert d["small"].eoi < 4096 < BOUNDARIES["chunk"] - 4200 < d["low"].eoi < BOUNDARIES["chunk"] - 32
    assert BOUNDARIES["tile"] < d["mid"].eoi < PART - 32 and PART + 32 < d["mid2"].eoi < 2 * PART - 32
    return d


# ---- cases --------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    lead: int          # the scan's address mod 16 the file is made for
    jpeg: bytes
    base: str          # the unshifted file whose pixels an accepted file decodes to
    status: int        # 0, or TRUNCATED for a file Pillow rejects
    key: tuple = ()    # (boundary kind, offset, pattern, lead) of a target
    index: int = -1    # scan index of the pattern's 0xFF
    at: bytes = b""    # the scan's bytes from `index` on
    run: int = 0       # 0xFFs that end at `index` (a fill run's length; 1: no 0xFF before it)

    @property
    def scan(self) -> bytes:
        return self.jpeg[scan_offset(self.jpeg):]


def _insert(scan: bytes, edits) -> bytes:
    """`edits`: (scan index, count) pairs; count 0xFF bytes go in before each index."""
    out, prev = bytearray(), 0
    for at, count in sorted(edits):
        out += scan[prev:at] + b"\xff" * count
        prev = at
    return bytes(out + scan[prev:])


def _rst_case(b: Base, kind: str, off: int, pat: str, lead: int) -> Case:
    """The restart-interval file with `pat`'s 0xFF at BOUNDARIES[kind] - lead + off."""
    T = BOUNDARIES[kind] - lead + off
    key, name = (kind, off, pat, lead), f"{pat}_{kind}{off:+d}_lead{lead}"
    if pat in ("ff00", "ffff00"):
        # the last stuffed 0xFF at or before T, moved up to T by fill bytes before the RSTn ahead of it
        q = max(k for k in b.ff00 if k <= T and k > b.rsts[0])
        r = max(k for k in b.rsts if k < q)
        extra = 1 if pat == "ffff00" else 0  # one fill byte before the stuffed 0xFF itself
        scan = _insert(b.scan, [(r, T - q), (q, extra)])
        return Case(name, lead, b.head + scan, b.name, 0, key, T, b"\xff\xff\x00"[1 - extra:], 1)
    if pat == "ffdn":
        # the last RSTn at or before T, moved up by fill bytes before the RSTn ahead of it
        j = max(i for i in range(1, len(b.rsts)) if b.rsts[i] <= T)
        scan = _insert(b.scan, [(b.rsts[j - 1], T - b.rsts[j])])
        return Case(name, lead, b.head + scan, b.name, 0, key, T, bytes([0xFF, 0xD0 + j % 8]), 1)
    # a run of R fill bytes that ends at T, then RSTn
    R = RUN[pat]
    j = max(i for i in range(1, len(b.rsts)) if b.rsts[i] + R - 1 <= T)
    scan = _insert(b.scan, [(b.rsts[j - 1], T + 1 - R - b.rsts[j]), (b.rsts[j], R)])
    return Case(name, lead, b.head + scan, b.name, 0, key, T, bytes([0xFF, 0xFF, 0xD0 + j % 8]), R)


def _eoi_case(b: Base, kind: str, off: int, pat: str, lead: int) -> Case:
    """`b` with EOI's 0xFF moved up to BOUNDARIES[kind] - lead + off by fill bytes."""
    T = BOUNDARIES[kind] - lead + off
    assert b.eoi <= T
    scan = _insert(b.scan, [(b.eoi, T - b.eoi)])
    return Case(f"{pat}_{kind}{off:+d}_lead{lead}", lead, b.head + scan, b.name, 0, (kind, off, pat, lead), T,
                b"\xff\xd9", T - b.eoi + 1)


def _junk(rng) -> bytes:
    """JUNK_BYTES random bytes.  Chance alone gives 40 KB about 150 0xFFs but less than one FF 00, so
    every pair the destuffer knows is also written at 256 random places."""
    junk = rng.integers(0, 256, JUNK_BYTES, dtype=np.uint8)
    pairs = [0x00, 0xFF, 0xD9, 0xDA, 0xC4, *range(0xD0, 0xD8)]
    for k in rng.integers(0, JUNK_BYTES - 1, 256):
        junk[k], junk[k + 1] = 0xFF, pairs[int(rng.integers(len(pairs)))]
    data = junk.tobytes()
    assert all(data.count(bytes([0xFF, m])) for m in pairs)
    return data


def target_keys() -> set:
    """Every (boundary, offset, pattern, lead) that must be attained."""
    keys = {(kind, off, pat, lead) for kind in BOUNDARIES for off in OFFSETS for pat in RST_PATTERNS
            for lead in LEADS3}
    keys |= {(kind, off, "ffd9", lead) for kind in BOUNDARIES for off in OFFSETS for lead in LEADS16}
    keys |= {(kind, off, "ffd9_fill", lead) for kind in ("part1", "part2") for off in OFFSETS for lead in LEADS3}
    return keys


@functools.lru_cache(maxsize=None)
def all_cases() -> tuple:
    B = bases()
    rng = np.random.default_rng(2102)
    out = [Case(f"base_{b.name}_lead{lead}", lead, b.jpeg, b.name, 0) for b in B.values() for lead in LEADS3]
    # EOI: the file with the most data that still ends before the boundary; and the 96 x 64 file,
    # whose fill run then crosses whole tiles
    eoi_base = {"chunk": "low", "tile": "low", "part1": "mid", "part2": "mid2"}
    for kind in BOUNDARIES:
        for off in OFFSETS:
            out += [_rst_case(B["big_ri"], kind, off, pat, lead) for pat in RST_PATTERNS for lead in LEADS3]
            out += [_eoi_case(B[eoi_base[kind]], kind, off, "ffd9", lead) for lead in LEADS16]
            if kind.startswith("part"):
                out += [_eoi_case(B["small"], kind, off, "ffd9_fill", lead) for lead in LEADS3]
    for p in (1, 2):
        # a scan ending in a lone 0xFF on part p's first byte
        for lead in LEADS16:
            b = B["big_ri" if lead & 1 else "big"]
            scan = b.scan[:p * PART - lead] + b"\xff"
            out.append(Case(f"lone_ff_part{p}_lead{lead}", lead, b.head + scan, b.name, TRUNCATED,
                            index=p * PART - lead, at=b"\xff", run=2 if scan[-2] == 0xFF else 1))
        # a scan cut with no terminator whose last part holds none of its bytes: its length n has
        # n + lead <= p PART < n + 16; and the lengths either side of that window
        for lead in LEADS3:
            for n in sorted({p * PART - 16, p * PART - 15, p * PART - lead, p * PART - lead + 1}):
                b = next(b for b in (B["big"], B["big_ri"]) if b.scan[n - 1] != 0xFF)
                out.append(Case(f"cut_part{p}_n{n - p * PART:+d}_lead{lead}", lead, b.head + b.scan[:n], b.name,
                                TRUNCATED, index=n))
    # bytes after EOI (EOI in part 0, in part 1) must add nothing
    for name in ("mid", "mid2"):
        junk = _junk(rng)
        out +=[Case(f"junk_{name}_lead{lead}", lead, B[name].jpeg + junk, name, 0, index=B[name].eoi, at=b"\xff\xd9",
                     run=1) for lead in LEADS3]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def cases_of_lead(lead: int) -> list:
    return [c for c in all_cases() if c.lead == lead]


def batch_of_lead(lead: int):
    """The lead's files as one packed batch: before each file a dummy entry of 0..15 zero bytes (not a
    JPEG: status < 0) puts the file's scan at `lead` mod 16, given a buffer that starts on 16 bytes.
    Returns (entries, positions): entries[positions[i]] is cases_of_lead(lead)[i]'s file."""
    entries, positions, at = [], [], 0
    for c in cases_of_lead(lead):
        pad = (lead - at - scan_offset(c.jpeg)) % 16
        entries += [b"\0" * pad, c.jpeg]
        positions.append(len(entries) - 1)
        at += pad + len(c.jpeg)
    return entries, positions


@functools.lru_cache(maxsize=None)
def base_pixels() -> dict:
    """Pillow's decode of every unshifted base file (read-only arrays), computed once."""
    from oracle import cpu_ref
    out = {}
    for name, b in bases().items():
        arr = np.asarray(cpu_ref.decode_rgb(b.jpeg)).copy()
        arr.setflags(write=False)
        out[name] = arr
    return out

"""JPEG files whose Huffman tables have shapes no encoder in the suite emits (TEST
INFRASTRUCTURE ONLY; shared by test_hufftables_cpu.py and test_gpu_hufftables.py).

Pillow writes the Annex K tables and ``jpeg_writer.optimal_table`` builds tables from the
image's own statistics: both give the frequent symbols the short codes, so nearly every symbol
decodes through a lookahead entry, nearly every AC entry is a pair and speculative lanes
synchronise within a few symbols.  The decoder's lookaheads are fixed: kLookBits = 11 bits for
the AC tables, kDcLookBits = 9 for the DC tables, kPLookBits = 9 in the coefficient-buffer scan
decoders and kLLookBits = 8 in the lane decoder's LDS rows; longer codes go through
huff_slow_bits / lane_slow, which fake a zero after 17 bits when no code matches.

A *shape* maps the used symbols of a table, sorted by falling frequency, to code lengths:

  inverted        the optimal lengths handed out in reverse (the most frequent symbol gets the
                  longest code)
  all(L)          every symbol at L bits
  cliff(k, L)     unary codes (0, 10, 110, ...) for the k most frequent symbols, the rest at L
  revcliff(k, L)  the same lengths with the rarest symbols on the unary codes

A table of n symbols fits all(L) when n <= 2^L - 1 and cliff(k, L) when n - k <= 2^(L-k) - 1 (the
all-ones code stays unassigned); where it does not, the hook uses 16 in place of L and records
``(kind, slot, n)`` in the case's ``fallbacks``.  ``MAY_FALL_BACK`` names the shapes this may
happen to.

Every group returns ``[(name, jpeg_bytes)]``, built once per process; ``meta(name)`` gives the
case's shape, fallbacks and number of 17-bit bad codes.  The expectation for every file is
whatever ``oracle.cpu_ref.decode_rgb`` does with its bytes, as in ``sampling_cases``.
"""

from __future__ import annotations

import functools

import numpy as np

from dataloader_amd.synthetic import textured_rgb
from tests import cmyk_cases as cc
from tests import jpeg_writer as jw
from tests import sampling_cases as sc

S420 = ((2, 2), (1, 1), (1, 1))
S444 = ((1, 1), (1, 1), (1, 1))
SAMPLINGS = {"420": S420, "444": S444}
ONE_SCAN = [jw.scan((0, 1, 2))]
GRAY_SCAN = [jw.scan((0,))]

ALL_LENGTHS = (8, 9, 10, 11, 12, 16)
CLIFFS = ((3, 11), (3, 12), (1, 9), (1, 10), (7, 16), (3, 8), (3, 9))


def shape_name(shape) -> str:
    return shape[0] + "_".join(str(v) for v in shape[1:])


SHAPES = [("optimal",), ("inverted",)] + [("all", L) for L in ALL_LENGTHS] + [("cliff", k, L) for k, L in CLIFFS] \
    + [("revcliff", k, L) for k, L in CLIFFS]
# shapes whose L-bit level (31 codes) is smaller than the AC tables of the 70x50 files
MAY_FALL_BACK = {("cliff", 3, 8), ("revcliff", 3, 8)}


def shape_lengths(shape, n: int) -> tuple[list[int], bool]:
    """Code lengths of the n used symbols in order of falling frequency (not for "optimal" /
    "inverted", which come from the frequencies), and whether 16 stands in for L."""
    if shape[0] == "all":
        L = shape[1]
        fell = n > (1 << L) - 1
        return [16 if fell else L] * n, fell
    k, L = shape[1], shape[2]
    fell = n - k > (1 << (L - k)) - 1
    lens = list(range(1, k + 1))[:n] + [16 if fell else L] * max(0, n - k)
    return (lens[::-1] if shape[0] == "revcliff" else lens), fell


class TableHook:
    """``table_hook`` of ``jpeg_writer.encode`` for one shape; collects the fallbacks."""

    def __init__(self, shape):
        self.shape = shape
        self.fallbacks: list = []

    def __call__(self, kind, slot, freq):
        if self.shape[0] == "optimal":
            return jw.optimal_table(np.asarray(freq))
        used = sorted((s for s in range(256) if freq[s]), key=lambda s: (-freq[s], s))
        if self.shape[0] == "inverted":
            codes = jw.canonical_codes(*jw.optimal_table(np.asarray(freq)))
            lens = sorted((codes[s][1] for s in used), reverse=True)
        else:
            lens, fell = shape_lengths(self.shape, len(used))
            if fell:
                self.fallbacks.append((kind, slot, len(used)))
        bits = [lens.count(ln) for ln in range(1, 17)]
        vals = [s for ln in range(1, 17) for s, l in zip(used, lens) if l == ln]
        return bits, vals


_META: dict = {}


def meta(name: str) -> dict:
    """{"shape", "fallbacks", "bad_codes"} of a case built by one of the groups."""
    return _META[name]


def _encode(name, shape, img, scans, four: dict | None = None, **kw) -> tuple[str, bytes]:
    hook = TableHook(shape)
    report: dict = {}
    if four is not None:
        data = cc.encode4(img, scans, table_hook=hook, **four, **kw)
    else:
        data = jw.encode(img, scans, table_hook=None if shape == ("optimal",) else hook, report=report, **kw)
    _META[name] = {"shape": shape, "fallbacks": hook.fallbacks, "bad_codes": report.get("bad_codes", 0)}
    return name, data


BAD_CODE_SHAPES = (("optimal",), ("all", 16), ("cliff", 3, 12))
SMALL_SIZES = ((70, 50), (33, 17))


@functools.lru_cache(maxsize=None)
def small_cases():
    """Baseline single-scan files of every shape at 70x50 and 33x17, 4:2:0 and 4:4:4, and gray
    33x17; shared tables (one DC and one AC table for the three components), table ids 2 and 3
    (luma 2, both chroma components 3); every n-th symbol 0 as the 17-bit bad code."""
    rng = np.random.default_rng(1301)
    out = []
    for (w, h) in SMALL_SIZES:
        for sname, samp in SAMPLINGS.items():
            img = textured_rgb(w, h, rng)
            tail = f"{sname}_{w}x{h}"
            for shape in SHAPES[1:]:
                out.append(_encode(f"{shape_name(shape)}_{tail}", shape, img, ONE_SCAN, samp=samp))
            for shape in (("optimal",), ("inverted",), ("all", 12)):
                out.append(_encode(f"shared_{shape_name(shape)}_{tail}", shape, img, ONE_SCAN, samp=samp, share_tables=True))
                out.append(_encode(f"ids23_{shape_name(shape)}_{tail}", shape, img, ONE_SCAN, samp=samp, table_ids=(2, 3, 3)))
            for shape in BAD_CODE_SHAPES:
                for n in (1, 5):
                    out.append(_encode(f"bad{n}_{shape_name(shape)}_{tail}", shape, img, ONE_SCAN, samp=samp,
                                       bad_code_every=n))
    gray = textured_rgb(33, 17, rng)[..., 1].copy()
    for shape in SHAPES[1:]:
        out.append(_encode(f"{shape_name(shape)}_gray_33x17", shape, gray, GRAY_SCAN))
    for shape in BAD_CODE_SHAPES:
        out.append(_encode(f"bad5_{shape_name(shape)}_gray_33x17", shape, gray, GRAY_SCAN, bad_code_every=5))
    return out


# (w, h) of the 4:4:4 quality-90 textured files: the smallest of the ladder 320x240, 336x256, ...
# (16 wider, 16 taller each step) whose destuffed entropy bytes clear sc.HUFF1_MAX_BYTES by 4 %
# (k_huff3) and sc.SEGMENT_BYTES by 3 % (k_huff2)
ROUTE_SHAPES = (("inverted",), ("all", 16))
ROUTE_QUALITY = 90
ROUTE_SIZES = {
    "huff3": {("inverted",): (320, 240), ("all", 16): (320, 240)},
    "huff2": {("inverted",): (432, 352), ("all", 16): (400, 320)},
}


def _route_image(w, h):
    return textured_rgb(w, h, np.random.default_rng(1302))


@functools.lru_cache(maxsize=None)
def route_cases():
    """One k_huff3 and one k_huff2 file per route shape (names ``<shape>_<route>_<w>x<h>``) and a
    k_huff3 file with one restart interval per MCU row (one interval per lane)."""
    out = []
    for shape in ROUTE_SHAPES:
        for route in ("huff3", "huff2"):
            w, h = ROUTE_SIZES[route][shape]
            out.append(_encode(f"{shape_name(shape)}_{route}_{w}x{h}", shape, _route_image(w, h), ONE_SCAN, samp=S444,
                               quality=ROUTE_QUALITY))
    w, h = ROUTE_SIZES["huff3"][("inverted",)]
    out.append(_encode(f"inverted_huff3_{w}x{h}_ri{w // 8}", ("inverted",), _route_image(w, h), ONE_SCAN, samp=S444,
                       quality=ROUTE_QUALITY, restart=w // 8))
    return out


PROGRESSIVE_SHAPES = (("inverted",), ("all", 8), ("all", 9), ("all", 16), ("cliff", 3, 9), ("revcliff", 7, 16))


@functools.lru_cache(maxsize=None)
def progressive_cases():
    """70x50 4:2:0 under jpeg_simple_progression and the deep script; the AC tables hold the
    EOBRUN symbols."""
    rng = np.random.default_rng(1303)
    img = textured_rgb(70, 50, rng)
    out = []
    for shape in PROGRESSIVE_SHAPES:
        for sname, script in (("simple", jw.simple_progression()), ("deep", jw.deep_progression())):
            out.append(_encode(f"{shape_name(shape)}_70x50_{sname}", shape, img, script, samp=S420, progressive=True))
    return out


@functools.lru_cache(maxsize=None)
def four_component_cases():
    """One Adobe CMYK (1x1 components) and one YCCK (10 blocks per MCU) 70x50 file per shape;
    decoded with the four-component option on."""
    out = []
    for shape in (("all", 16), ("inverted",)):
        out.append(_encode(f"{shape_name(shape)}_cmyk_70x50", shape, cc.planes4(70, 50, 1304), cc.ONE_SCAN,
                           four={"adobe": 0}))
        out.append(_encode(f"{shape_name(shape)}_ycck_70x50", shape, cc.planes4(70, 50, 1305), cc.ONE_SCAN,
                           four={"adobe": 2, "samp": cc.S10}))
    return out


# ---- tables libjpeg rejects -------------------------------------------------------------
def dht_tables(jpeg: bytes) -> list[tuple[int, int, list[int], list[int]]]:
    """(class, id, BITS[16], HUFFVAL) of every table of every DHT segment before the first SOS."""
    out, pos = [], 2
    while jpeg[pos + 1] != 0xDA:
        n = int.from_bytes(jpeg[pos + 2:pos + 4], "big")
        if jpeg[pos + 1] == 0xC4:
            q, end = pos + 4, pos + 2 + n
            while q < end:
                bits = list(jpeg[q + 1:q + 17])
                out.append((jpeg[q] >> 4, jpeg[q] & 15, bits, list(jpeg[q + 17:q + 17 + sum(bits)])))
                q += 17 + sum(bits)
        pos += 2 + n
    return out


def with_tables(jpeg: bytes, replace: dict, extra: list = ()) -> bytes:
    """The file with table (class, id) -> (bits, vals) of ``replace`` in place of its own and the
    tables ``extra`` [(class, id, bits, vals)] in a DHT segment of their own before the SOS."""
    out, pos = bytearray(jpeg[:2]), 2
    while jpeg[pos + 1] != 0xDA:
        n = int.from_bytes(jpeg[pos + 2:pos + 4], "big")
        if jpeg[pos + 1] == 0xC4:
            body = bytearray()
            for tc, th, bits, vals in dht_tables(jpeg[:2] + jpeg[pos:pos + 2 + n] + b"\xff\xda"):
                bits, vals = replace.get((tc, th), (bits, vals))
                body += bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals)
            out += jw._seg(0xC4, bytes(body))
        else:
            out += jpeg[pos:pos + 2 + n]
        pos += 2 + n
    for tc, th, bits, vals in extra:
        out += jw._seg(0xC4, bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals))
    return bytes(out + jpeg[pos:])


def _bits(**counts) -> list[int]:
    return [counts.get(f"l{ln}", 0) for ln in range(1, 17)]


# one defect each (jdhuff.c jpeg_make_d_derived_tbl, jdmarker.c get_dht)
DEFECTS = {
    "oversub": (_bits(l1=1, l2=3), [0, 1, 2, 3]),            # 0, 10, 11, then a fourth 2-bit code
    "allones": (_bits(l1=1, l2=1, l3=2), [0, 1, 2, 3]),      # 0, 10, 110, 111
    "dc16": (_bits(l2=3, l3=1), [0, 16, 1, 2]),              # a legal code; value 16 is no DC category
    "sum257": (_bits(l15=2, l16=255), [v & 255 for v in range(257)]),
}
# (name, defect, class, id of the used table it replaces)
REJECT_USED = [("oversub_dc0", "oversub", 0, 0), ("oversub_ac1", "oversub", 1, 1), ("allones_dc1", "allones", 0, 1),
               ("allones_ac0", "allones", 1, 0), ("dc16_dc0", "dc16", 0, 0), ("dc16_dc2", "dc16", 0, 2),
               ("sum257_ac0", "sum257", 1, 0), ("sum257_dc1", "sum257", 0, 1)]
# the same defects in a table no scan references
REJECT_UNUSED = [("oversub_unused_ac3", "oversub", 1), ("allones_unused_dc3", "allones", 0),
                 ("dc16_unused_dc3", "dc16", 0), ("sum257_unused_ac3", "sum257", 1),
                 ("sum257_unused_dc3", "sum257", 0)]


@functools.lru_cache(maxsize=None)
def rejected_cases():
    """A valid 70x50 4:2:0 file (tables 0, 1, 2 of both classes) with one table made invalid."""
    rng = np.random.default_rng(1306)
    name, base = _encode("valid_70x50", ("optimal",), textured_rgb(70, 50, rng), ONE_SCAN, samp=S420)
    assert sorted((tc, th) for tc, th, _, _ in dht_tables(base)) == [(c, i) for c in (0, 1) for i in (0, 1, 2)]
    out = [(name, base)]
    for name, defect, tc, th in REJECT_USED:
        out.append((f"{name}_70x50", with_tables(base, {(tc, th): DEFECTS[defect]})))
    for name, defect, tc in REJECT_UNUSED:
        out.append((f"{name}_70x50", with_tables(base, {}, [(tc, 3, *DEFECTS[defect])])))
    for n, _ in out[1:]:
        _META[n] = {"shape": ("optimal",), "fallbacks": [], "bad_codes": 0}
    return out


GROUPS = {"small": small_cases, "route": route_cases, "progressive": progressive_cases,
          "four_component": four_component_cases, "rejected": rejected_cases}


@functools.lru_cache(maxsize=None)
def references(group: str):
    """The oracle's decode of every file of a group, computed once: a read-only H x W x 3
    array, or ``None`` where the reference zero-fills."""
    from oracle import cpu_ref
    out = []
    for _, j in GROUPS[group]():
        img = cpu_ref.decode_rgb(j)
        arr = None if img is None else np.asarray(img).copy()
        if arr is not None:
            arr.setflags(write=False)
        out.append(arr)
    return out


route_of = sc.route_of

"""Lossless WebP files of stream forms libwebp's encoder never emits (TEST INFRASTRUCTURE ONLY;
shared by test_vp8l_forms_cpu.py and test_gpu_vp8l_forms.py), built at import by
tests/vp8l_writer.py with a seeded generator.

``cases()`` -> [(name, bytes, expect)], expect "dev" (the device decodes it) or "declined" (more
groups than the table area holds: Pillow's); ``bad()`` -> [(name, bytes)], each a sound case with
one field damaged, one file per error rule of vp8l.hpp's header comment; ``record(name)`` is the
writer's record of what the file holds.  Every case names the one boundary it crosses and is the
smallest shape that still reaches it.  The expectation for pixels is always Pillow's.
"""

from __future__ import annotations

import functools

import numpy as np

from tests import vp8l_writer as vw
from tests.vp8l_writer import CROSS, GREEN, INDEX, PREDICTOR, Code, Stream
from tests.webp_cases import riff

_REC: dict = {}
BODY_ERRORS = ("bad_copy_before_first", "bad_copy_past_last", "bad_cut_one_bit")  # the prologue is sound: only the decode finds them


def record(name: str) -> dict:
    cases(), bad()
    return _REC[name]


def _words(r, n, alpha=None):
    v = r.integers(0, 1 << 32, n, dtype=np.uint64)
    if alpha is not None:
        v = (v & 0xFFFFFF) | (alpha << 24)
    return [int(x) for x in v]


def _lits(vals):
    return [("lit", int(v)) for v in vals]


def _green(vals):  # literals with a value in green alone (indices, modes)
    return [("lit", 0xFF000000 | (int(v) << 8)) for v in vals]


def _grid(w, h, vals, **kw):
    return Stream(w, h, _green(vals), **kw)


def _palette(cols, **kw):
    """The palette's stream: each colour as the difference to the one before."""
    d = [cols[0]] + [vw._sub(b, a) for a, b in zip(cols, cols[1:])]
    return Stream(len(cols), 1, _lits(d), **kw)


def _bundle(idx, w, h, bits):
    """Rows of w indices packed 1 << bits to a word's green, low bits first."""
    per, out = 8 >> bits, []
    for y in range(h):
        row = idx[y * w:(y + 1) * w]
        for x0 in range(0, w, 1 << bits):
            out.append(sum(int(v) << (per * k) for k, v in enumerate(row[x0:x0 + (1 << bits)])))
    return _green(out)


def _index(r, n, w, h, top=None):
    """(transform, main ops) of an n-colour palette with random indices below ``top``."""
    b = 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3
    idx = r.integers(0, top or n, w * h)
    return (INDEX, n, _palette(_words(r, n))), _bundle(idx, w, h, b)


def _sub_size(w, h, b):
    return (w + (1 << b) - 1) >> b, (h + (1 << b) - 1) >> b


def _pred(r, w, h, b=2, modes=None, **kw):
    bw, bh = _sub_size(w, h, b)
    m = modes if modes is not None else r.integers(0, 16, bw * bh)
    return (PREDICTOR, b, _grid(bw, bh, m, **kw))


def _cross(r, w, h, b=2, mult=None):
    bw, bh = _sub_size(w, h, b)
    return (CROSS, b, Stream(bw, bh, _lits(mult if mult is not None else _words(r, bw * bh, 0xFF))))


def _ladder(n, syms):
    """Lengths 1, 2, ..., 14, 15, 15 over the 16 symbols ``syms`` of an alphabet of n."""
    out = [0] * n
    for k, s in enumerate(syms):
        out[s] = min(k + 1, 15)
    return out


def _in_slot(r, bits, slot, count):
    out = set()
    while len(out) < count:
        out.update(v for v in _words(r, 4096) if vw.cache_slot(v, bits) == slot)
    return sorted(out)[:count]


def _fit(build, want):
    """The first build(k), k = 0, 1, ..., whose stream's bit count mod 8 is ``want``."""
    for k in range(64):
        out = build(k)
        if out[1]["nbits"] % 8 == want:
            return out
    raise AssertionError("no stream of that length")


def _add(out, name, built, expect="dev"):
    payload, rec = built
    assert name not in _REC, name
    _REC[name] = rec
    out.append((name, riff(payload), expect))


def _bad_px():
    return _words(np.random.default_rng(7), 64)


def _bad_base():
    px = _bad_px()
    return _lits(px[:30]) + [("copy", 4, 2)] + _lits(px[:30])


def _one_bit_tail():
    return _fit(lambda k: vw.vp8l(8, 8, [(GREEN,)], _lits(_words(np.random.default_rng(50 + k), 64))), 1)


@functools.lru_cache(maxsize=None)
def cases():
    r = np.random.default_rng(2026)
    out: list = []
    add = functools.partial(_add, out)

    # --- transform orders ---
    add("only_predictor_9x7", vw.vp8l(9, 7, [_pred(r, 9, 7)], _lits(_words(r, 63))))
    add("only_cross_b9_7x5", vw.vp8l(7, 5, [_cross(r, 7, 5, 9)], _lits(_words(r, 35))))  # 35 pixels: a ragged last RGB store
    add("only_green_7x5", vw.vp8l(7, 5, [(GREEN,)], _lits(_words(r, 35))))
    for first, w in (("green", 300), ("green", 257), ("predictor", 257), ("predictor", 300)):
        for b, n in ((3, 2), (1, 16)) if (first == "green") == (w == 300) else ((2, 4), (0, 40)):
            t, ops = _index(r, n, w, 3)
            add(f"{first}_index_b{b}_{w}x3", vw.vp8l(w, 3, [(GREEN,) if first == "green" else _pred(r, w, 3), t], ops))
    t, ops = _index(r, 2, 5, 2)
    add("green_index_b3_5x2", vw.vp8l(5, 2, [(GREEN,), t], ops))
    t, ops = _index(r, 4, 5, 2)
    add("predictor_index_b2_5x2", vw.vp8l(5, 2, [_pred(r, 5, 2), t], ops))
    t, ops = _index(r, 4, 21, 9)
    add("order_cross_green_predictor_index", vw.vp8l(21, 9, [_cross(r, 21, 9), (GREEN,), _pred(r, 21, 9, 3), t], ops))
    t, ops = _index(r, 3, 21, 9)  # the predictor and cross-colour see the bundled width, 6
    add("order_green_index_predictor_cross", vw.vp8l(21, 9, [(GREEN,), t, _pred(r, 6, 9), _cross(r, 6, 9, 3)], ops))

    # --- predictor ---
    add("predictor_modes_16x16", vw.vp8l(16, 16, [_pred(r, 16, 16, 2, r.permutation(16))], _lits(_words(r, 256))))
    add("predictor_modes_8x66", vw.vp8l(8, 66, [_pred(r, 8, 66, 2, [(3 * k + 14) % 16 for k in range(34)])], _lits(_words(r, 528))))
    add("predictor_b9_5x5", vw.vp8l(5, 5, [_pred(r, 5, 5, 9, [5])], _lits(_words(r, 25))))
    add("predictor_w2", vw.vp8l(2, 6, [_pred(r, 2, 6, 2, [3, 10])], _lits(_words(r, 12))))
    add("predictor_w3", vw.vp8l(3, 6, [_pred(r, 3, 6, 2, [5, 9])], _lits(_words(r, 18))))
    ends = r.choice(np.array([0x00, 0xFF, 0x00, 0xFF, 0x80], np.uint64), (144, 4))  # channels of 0x00 and 0xFF neighbours
    target = [int(a << 24 | b << 16 | c << 8 | d) for a, b, c, d in ends]
    modes, clips = [11, 12, 13, 12, 13, 11, 13, 11, 12], set()
    res = vw.predictor_residuals(target, 12, 12, 2, modes, clips)
    built = vw.vp8l(12, 12, [_pred(r, 12, 12, 2, modes)], _lits(res))
    built[1]["clips"] = clips
    add("predictor_clip_both_ways", built)

    # --- cross-colour ---
    m = [0x80, 0x7F, 0xFF]
    mult = [0xFF000000 | m[k % 3] << 16 | m[(k // 3) % 3] << 8 | m[(k + k // 3) % 3] for k in range(9)]
    built = vw.vp8l(12, 12, [_cross(r, 12, 12, 2, mult)], _lits(_words(r, 144)))
    built[1]["multipliers"] = {(pos, (v >> (8 * pos)) & 255) for v in mult for pos in range(3)}
    add("cross_multipliers_b2", built)

    # --- colour cache ---
    px = _words(r, 40)
    add("cache1_main", vw.vp8l(8, 5, [], _lits(px[:6]) + [("cache", px[5]), ("slot", 0), ("slot", 1)] + _lits(px[9:38]) + [("cache", px[37]), ("slot", 0)],
                               cache_bits=1))
    top = _in_slot(r, 11, 2047, 2)
    add("cache11_symbol_2327", vw.vp8l(8, 5, [], _lits(px[:6] + top[:1]) + [("cache", top[0]), ("cache", px[2])] + _lits(px[:29] + top[1:]) + [("cache", top[1])],
                                       cache_bits=11))
    sub = _green([3, 7, 11, 2]) + [("cache", 0xFF000000 | 7 << 8), ("cache", 0xFF000000 | 3 << 8)]
    add("cache_in_predictor_image", vw.vp8l(9, 7, [(PREDICTOR, 2, Stream(3, 2, sub, cache_bits=11))], _lits(_words(r, 63))))
    cm = _words(r, 4, 0xFF)
    add("cache_in_cross_image", vw.vp8l(9, 7, [(CROSS, 2, Stream(3, 2, _lits(cm) + [("cache", cm[1]), ("cache", cm[3])], cache_bits=5))],
                                        _lits(_words(r, 63))))
    pal = _palette(_words(r, 5))
    pal.ops, pal.cache_bits = pal.ops[:3] + [("cache", pal.ops[1][1]), ("cache", pal.ops[2][1])], 6
    add("cache_in_palette", vw.vp8l(9, 5, [(INDEX, 5, pal)], _bundle(r.integers(0, 5, 45), 9, 5, 1)))
    ent = Stream(3, 2, _green([0, 1, 2]) + [("cache", 0xFF000000 | 1 << 8), ("cache", 0xFF000000), ("cache", 0xFF000000 | 2 << 8)], cache_bits=4)
    add("cache_in_entropy_image", vw.vp8l(9, 7, [], _lits(_words(r, 63)), meta=(2, [0, 1, 2, 1, 0, 2], ent)))
    same = _in_slot(r, 4, 9, 210)
    add("cache_collisions_210", vw.vp8l(16, 16, [], _lits(same) + [("cache", same[-1])] + _lits(_words(r, 45)), cache_bits=4))
    add("cache_after_copy_70", vw.vp8l(16, 10, [], _lits(px[:30]) + [("copy", 70, 120 + 30), ("cache", px[9]), ("cache", px[29])] + _lits(_words(r, 58)),
                                       cache_bits=10))
    ops = _lits(px[:20]) + [("cache", px[4]), ("copy", 9, 120 + 13), ("cache", px[15])] + _lits(_words(r, 29)) + [("cache", px[0])] + _lits(_words(r, 19))
    add("cache_with_groups", vw.vp8l(10, 8, [], ops, cache_bits=9, meta=(2, [0, 1, 2, 2, 1, 0], None)))

    # --- palette ---
    for n in (1, 2, 3, 4, 5, 16, 17, 256):
        t, ops = _index(r, n, 9, 5)
        add(f"palette_{n}", vw.vp8l(9, 5, [t], ops))
    for n, topv in ((3, 4), (5, 16), (17, 256)):  # indices past the palette: transparent black
        t, ops = _index(r, n, 9, 5, topv)
        add(f"palette_{n}_index_past_end", vw.vp8l(9, 5, [t], ops))

    # --- codes ---
    syms = [int(s) for s in r.permutation(250)[:16]]
    for a, name in enumerate(("green", "red", "blue", "alpha")):
        lad = [s << (8, 16, 0, 24)[a] for s in syms]
        ops = _lits([lad[k] for k in r.integers(0, 16, 44)] + lad[14:] + [lad[k] for k in r.integers(0, 16, 18)])
        add(f"code15_{name}", vw.vp8l(8, 8, [], ops, codes={(0, a): Code(280 if a == 0 else 256, _ladder(280 if a == 0 else 256, syms))}))
    dsyms = [int(s) for s in r.permutation(14)[:14]] + [14, 15]  # distance symbols 0..15: codes 1..192
    ops = _lits(_words(r, 80))
    for s in dsyms[::-1]:
        ops.append(("copy", 3, 1 + s if s < 4 else ((2 + (s & 1)) << ((s - 2) >> 1)) + 1))
    ops += _lits(_words(r, 12 * 12 - 80 - 48))
    add("code15_dist", vw.vp8l(12, 12, [], ops, codes={(0, 4): Code(40, _ladder(40, dsyms))}))
    add("one_symbol_everywhere_0bit", vw.vp8l(8, 8, [(GREEN,)], _lits([0xFF004D00] * 64)))
    g = _words(r, 64, 0xFF)
    ops = _lits([(v & 0xFF00FFFF) | 0x00330000 for v in g])
    add("simple_two_equal", vw.vp8l(8, 8, [], ops, codes={(0, 1): Code(256, simple=([0x33, 0x33], True))}))
    ops = _lits([(v & 0xFFFF00FF) | (v & 0x100) for v in g])
    add("simple_1bit", vw.vp8l(8, 8, [], ops, codes={(0, 0): Code(280, simple=([0, 1], False)), (0, 3): Code(256, simple=([0xFF], True))}))
    ops = _lits(g[:20]) + [("copy", 6, 7), ("copy", 5, 8)] + _lits(g[:33])  # codes 7 and 8: distance symbol 5
    add("simple_dist_one_outside", vw.vp8l(8, 8, [], ops, codes={(0, 4): Code(40, simple=([5, 200], True))}))
    ops = _lits([(v & 0xFF00FFFF) | ((v >> 8 & 255) << 16) for v in g])  # red as green
    lens = vw.limited_lengths(np.bincount([(o[1] >> 16) & 255 for o in ops], minlength=256).tolist())
    add("max_symbol_is_alphabet", vw.vp8l(8, 8, [], ops, codes={(0, 1): Code(256, lens, cl_syms=vw.cl_plain(lens), max_symbol=(256, 7))}))
    ops = _lits([(v & 0xFFFFFF00) | (v & 1) for v in g])
    add("max_symbol_2", vw.vp8l(8, 8, [], ops, codes={(0, 2): Code(256, [1, 1] + [0] * 254, cl_syms=[(1, 0), (1, 0)], max_symbol=(2, 0))}))
    ops = _lits(_words(r, 300))
    eight = [8] * 256
    add("repeat16_first_and_last", vw.vp8l(20, 15, [], ops, codes={(0, 3): Code(256, eight, cl_syms=[(16, 3)] * 42 + [(16, 1)],
                                                                                   cl_len=[int(k in (8, 16)) for k in range(19)])}))
    lens = [7] * 128 + [0] * 128  # 17: zeros up to the alphabet's end, in runs of 10 and a last one of 8
    ops7 = _lits([(v & 0xFF00FFFF) | (v >> 1 & 0x7F0000) for v in _words(r, 64)])
    add("repeat17_ends_alphabet", vw.vp8l(8, 8, [], ops7, codes={(0, 1): Code(256, lens, cl_syms=vw.cl_plain(lens[:128]) + [(17, 7)] * 12 + [(17, 5)])}))
    add("repeat18_ends_alphabet", vw.vp8l(8, 8, [], ops7, codes={(0, 1): Code(256, lens, cl_syms=vw.cl_plain(lens[:128]) + [(18, 117)])}))
    add("code_length_code_single", vw.vp8l(20, 15, [], ops, codes={(0, 2): Code(256, eight, cl_syms=vw.cl_plain(eight))}))

    # --- back-references ---
    tiles = [(x + y) % 3 for y in range(17) for x in range(16)]
    add("copy4096_dist1_64x65", vw.vp8l(64, 65, [], _lits(g[:1]) + [("copy", 4096, 2)] + _lits(_words(r, 63)), meta=(2, tiles, None)))
    ops = _lits(g[:3])
    for d in (2, 3):
        ops += [("copy", 3 * d + 2, 120 + d)]
    ops += _lits(_words(r, 47))
    for d in (63, 64, 65):
        ops += [("copy", 2 * d + 7, 120 + d)]
    ops += _lits(_words(r, 30 * 16 - 69 - 2 * 192 - 21))
    add("copy_overlapping_2_3_63_64_65", vw.vp8l(30, 16, [], ops))
    for w in (20, 5, 2):  # (5 wide: three codes point right of the pixel and clamp to 1; 2 wide: twelve)
        ops, pos = [], 0
        for code in sorted(range(1, 121), key=lambda c: vw.distance(c, w)):
            need = vw.distance(code, w) - pos
            ops += _lits(_words(r, max(0, need)))
            ops.append(("copy", 1, code))
            pos += max(0, need) + 1
        extra = -pos % w
        add(f"short_codes_all_{w}wide", vw.vp8l(w, (pos + extra) // w, [], ops + _lits(_words(r, extra))))
    add("copy_extra_bits_max_to_last_pixel", vw.vp8l(64, 64, [], _lits(g[:1]) + [("copy", 4000, 2), ("copy", 95, 120 + 3990)]))
    add("copy_in_predictor_image", vw.vp8l(20, 20, [(PREDICTOR, 2, Stream(5, 5, _green(r.integers(0, 16, 7)) + [("copy", 12, 120 + 6), ("copy", 6, 1)]))],
                                           _lits(_words(r, 400))))
    pal = _palette(_words(r, 12))
    pal.ops = pal.ops[:5] + [("copy", 7, 120 + 4)]
    add("copy_in_palette", vw.vp8l(9, 5, [(INDEX, 12, pal)], _bundle(r.integers(0, 12, 45), 9, 5, 1)))
    ent = Stream(5, 4, _green([0, 1, 2, 1, 3]) + [("copy", 10, 1), ("copy", 5, 120 + 14)])
    add("copy_in_entropy_image", vw.vp8l(20, 16, [], _lits(_words(r, 320)), meta=(2, [v >> 8 & 255 for v in vw.expand(ent)[0]], ent)))

    # --- groups ---
    add("groups_prefix_bits_2", vw.vp8l(9, 9, [], _lits(_words(r, 81)), meta=(2, [0, 3, 1, 2, 2, 0, 1, 3, 0], None)))
    add("groups_prefix_bits_9", vw.vp8l(9, 9, [], _lits(_words(r, 81)), meta=(9, [0], None)))
    flat = _lits([0xFF000000 | (x * 3 + y) << 8 | (x ^ y) for y in range(64) for x in range(64)])
    add("groups_at_cap_256_64x64", vw.vp8l(64, 64, [], flat, meta=(2, [int(v) for v in r.permutation(256)], None)))
    over = [int(v) for v in r.permutation(256)]
    over[over.index(255)] = 256
    add("groups_over_cap_257_64x64", vw.vp8l(64, 64, [], flat, meta=(2, over, None)), "declined")
    add("groups_sparse_5_4x4", vw.vp8l(4, 4, [], _lits(_words(r, 16)), meta=(2, [5], None)), "declined")

    # --- input ring ---
    add("ring_3k_payload", vw.vp8l(32, 30, [], _lits(_words(r, 960)), alpha=0))
    tail = lambda k: vw.vp8l(6, 4, [], _lits(_words(np.random.default_rng(k), 24)))  # noqa: E731
    for want, odd, name in ((0, 1, "tail_full_byte_pad"), (0, 0, "tail_full_byte_no_pad"), (1, 1, "tail_one_bit_pad"), (1, 0, "tail_one_bit_no_pad")):
        built = next(b for b in (_fit(lambda k, s=s: tail(100 * s + k), want) for s in range(40)) if len(b[0]) % 2 == odd)
        add(name, built)
    add("tail_one_bit_last_byte", _one_bit_tail())
    add("sound_base_of_bad_files", vw.vp8l(8, 8, [(GREEN,)], _bad_base(), cache_bits=3))
    add("sound_base_with_sub_image", vw.vp8l(8, 8, [(GREEN,), (PREDICTOR, 2, Stream(2, 2, _green([1, 2]) + [("copy", 2, 120 + 2)]))],
                                             _bad_base(), cache_bits=3))
    assert len({c[0] for c in out}) == len(out)
    return out


def ring_batch():
    """"ring_3k_payload" sixteen times with fillers that are no image between them, so that its
    payload (20 bytes into the file) starts at every offset mod 16 of the batch's buffer."""
    data = {c[0]: c[1] for c in cases()}["ring_3k_payload"]
    files, at = [], 0
    for k in range(16):
        pad = (k - 20 - at) % 16
        if pad:
            files.append(b"\xaa" * (pad + 32))
            at += pad + 32
        files.append(data)
        at += len(data)
    return files


@functools.lru_cache(maxsize=None)
def bad():
    """[(name, bytes)]: the case "sound_base_of_bad_files" (subtract-green, a 3-bit cache, one
    back-reference; or with a predictor sub-image added) with one field changed."""
    px = _bad_px()
    base = _bad_base()
    out: list = []

    def add(name, ops=base, tr=((GREEN,),), **kw):
        payload, rec = vw.vp8l(8, 8, list(tr), ops, **{"cache_bits": 3, **kw})
        _REC[name] = rec
        out.append((name, riff(payload)))

    add("bad_transform_twice", tr=((GREEN,), (GREEN,)))
    add("bad_cache_bits_0", cache_field=0)
    add("bad_cache_bits_12", cache_field=12)
    lens = [1, 1] + [0] * 38
    add("bad_simple_all_outside", codes={(0, 4): Code(40, simple=([40, 255], True), check=False)})
    add("bad_max_symbol_above_alphabet", codes={(0, 4): Code(40, lens, cl_syms=vw.cl_plain(lens), max_symbol=(41, 2))})
    add("bad_repeat_past_alphabet", codes={(0, 4): Code(40, lens, cl_syms=[(1, 0), (1, 0), (18, 28)])})  # 2 + 39 > 40
    add("bad_code_length_code_empty", codes={(0, 4): Code(40, lens, cl_len=[0] * 19)})
    add("bad_code_empty", codes={(0, 4): Code(40, [0] * 40, cl_syms=vw.cl_plain([0] * 40), cl_len=[1, 1] + [0] * 17, check=False)})
    add("bad_code_oversubscribed", codes={(0, 4): Code(40, [1, 1, 1] + [0] * 37, check=False)})
    add("bad_code_incomplete_two_symbols", codes={(0, 4): Code(40, [1, 2] + [0] * 38, check=False)})
    add("bad_copy_before_first", _lits(px[:30]) + [("copy", 4, 120 + 31)] + _lits(px[:30]), check=False)
    add("bad_copy_past_last", _lits(px[:30]) + [("copy", 35, 2)], check=False)
    sub = Stream(2, 2, _green([1, 2]) + [("copy", 2, 120 + 3)], check=False)
    add("bad_copy_before_first_in_sub_image", tr=((GREEN,), (PREDICTOR, 2, sub)))
    sub = Stream(2, 2, _green([1, 2]) + [("copy", 3, 1)], check=False)
    add("bad_copy_past_last_in_sub_image", tr=((GREEN,), (PREDICTOR, 2, sub)))
    payload, rec = _one_bit_tail()  # the case "tail_one_bit_last_byte" without its last byte
    _REC["bad_cut_one_bit"] = rec
    out.append(("bad_cut_one_bit", riff(payload[:-1])))
    return out

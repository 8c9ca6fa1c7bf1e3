"""Test-only VP8L (lossless WebP) bitstream writer: every choice an encoder makes is an argument.

libwebp's encoder writes a narrow part of the format: one transform order, a colour cache of at
most 10 bits and none in a sub-image, no predictor mode above 13, the code shapes its heuristics
pick.  Here the caller gives the transform list in any order, every sub-image as a script of its
own, the colour-cache bits of every stream, the entropy image, and each prefix code down to the
code-length code, the ``max_symbol`` field and the place of every repeat symbol.  Written from
the format specification ("WebP Lossless Bitstream Specification"); standard library and numpy
only, no project code.

A stream is a script of operations over ARGB words (alpha << 24 | red << 16 | green << 8 | blue):

  ("lit", argb)            a literal
  ("cache", argb)          a colour-cache reference to a colour the cache holds (the writer
                           tracks the cache: slot = 0x1e35a7bd * argb >> (32 - bits))
  ("slot", k)              a colour-cache reference to slot k, whatever it holds
  ("copy", length, code)   a back-reference; ``code`` is the distance code: 1..120 are the short
                           codes over the (dx, dy) map, above that the distance is code - 120

``expand`` is the plain sequential forward model of a script (the ARGB words it stands for, before
any inverse transform); ``vp8l`` writes a payload and returns it with a record of what it holds
(which transform order, modes, code shapes, distance codes ...), the evidence of the coverage test.
The oracle for pixels is Pillow, not this model.
"""

from __future__ import annotations

import heapq

PREDICTOR, CROSS, GREEN, INDEX = 0, 1, 2, 3
ALPHABETS = ("green", "red", "blue", "alpha", "dist")
CL_ORDER = [17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
# the 120 short distance codes as (dx, dy): distance = dx + dy * xsize, at least 1
DIST_MAP = [
    (0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3),
    (-1, 3), (3, 1), (-3, 1), (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1), (3, 3), (-3, 3),
    (2, 4), (-2, 4), (4, 2), (-4, 2), (0, 5), (3, 4), (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5), (5, 1), (-5, 1), (2, 5),
    (-2, 5), (5, 2), (-5, 2), (4, 4), (-4, 4), (3, 5), (-3, 5), (5, 3), (-5, 3), (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1),
    (2, 6), (-2, 6), (6, 2), (-6, 2), (4, 5), (-4, 5), (5, 4), (-5, 4), (3, 6), (-3, 6), (6, 3), (-6, 3), (0, 7), (7, 0), (1, 7),
    (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1), (4, 6), (-4, 6), (6, 4), (-6, 4), (2, 7), (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7),
    (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5), (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1), (8, 2), (6, 6), (-6, 6),
    (8, 3), (5, 7), (-5, 7), (7, 5), (-7, 5), (8, 4), (6, 7), (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6), (8, 7)]
assert len(DIST_MAP) == 120 and len(set(DIST_MAP)) == 120


class BitWriter:
    """LSB first, as every field of the format is read."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.nbits = 0

    def bits(self, v: int, n: int) -> None:
        assert 0 <= v < (1 << n) or n == 0, (v, n)
        self.acc |= v << self.n
        self.n += n
        self.nbits += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, n: int) -> None:  # a prefix code's bits go first bit first
        for i in range(n - 1, -1, -1):
            self.bits((code >> i) & 1, 1)

    def done(self) -> bytes:
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lengths) -> dict:
    """symbol -> (code, length) of the canonical code: shorter codes first, then by symbol."""
    cnt = [0] * 17
    for ln in lengths:
        cnt[ln] += 1
    cnt[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lengths):
        if ln:
            out[s] = (nxt[ln], ln)
            nxt[ln] += 1
    return out


def kraft(lengths) -> int:
    """Sum of 2^(15 - length) over the symbols: 2^15 for a complete code."""
    return sum(1 << (15 - ln) for ln in lengths if ln)


def limited_lengths(hist, limit: int = 15) -> list:
    """Huffman code lengths of a histogram, at most ``limit`` bits: counts are flattened (halved
    towards 1) until the tree fits.  One used symbol gets length 1 (a code read with no bits)."""
    used = [s for s, c in enumerate(hist) if c]
    out = [0] * len(hist)
    if len(used) == 1:
        out[used[0]] = 1
    counts = {s: hist[s] for s in used}
    while len(used) > 1:
        heap = [(c, s, (s,)) for s, c in counts.items()]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(depth.values()) <= limit:
            for s, d in depth.items():
                out[s] = d
            break
        counts = {s: (c + 1) // 2 for s, c in counts.items()}
    return out


def cl_plain(lengths) -> list:
    """Every length as its own code-length symbol (no repeats, trailing zeros included)."""
    return [(ln, 0) for ln in lengths]


def cl_runs(lengths) -> list:
    """Code-length symbols with repeats 16 / 17 / 18 wherever they apply (greedy); the length
    repeated by 16 before any non-zero length is 8."""
    out, i, n, prev = [], 0, len(lengths), 8
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            r = min(run, 138)
            out.append((18, r - 11) if r >= 11 else (17, r - 3))
            i += r
            continue
        if v == 0:
            out.append((0, 0))
            i += 1
            continue
        if v != prev:
            out.append((v, 0))
            prev, i, run = v, i + 1, run - 1
        if run >= 3:
            r = min(run, 6)
            out.append((16, r - 3))
            i += r
        elif run:
            out.append((v, 0))
            i += 1
    return out


CL_EXTRA = {16: (2, 3), 17: (3, 3), 18: (7, 11)}  # extra bits, repeat offset


class Code:
    """One prefix code over an alphabet of ``n`` symbols.

    Normal form: ``lengths`` (n of them); ``cl_syms`` = [(code-length symbol, extra value)]
    (default: ``cl_runs``), ``cl_len`` = the 19 lengths of the code-length code (default: from the
    symbols' histogram; one symbol used gives a code-length code of a single symbol), ``max_symbol``
    = None (the flag stays 0) or (count, f): the count of code-length symbols to read, written in
    2 + 2 f bits.  Simple form: ``simple`` = (symbols, wide): one or two symbols, the first of 8
    bits if ``wide`` else 1 bit; symbols at or above n are written as they are and count for nothing.
    ``check`` = False writes an over-subscribed, incomplete or empty code as it is."""

    def __init__(self, n, lengths=None, simple=None, cl_syms=None, cl_len=None, max_symbol=None, check=True):
        self.n, self.simple, self.max_symbol, self.check = n, simple, max_symbol, check
        if simple is not None:
            lengths = [0] * n
            for s in simple[0]:
                if s < n:
                    lengths[s] = 1
        self.lengths = list(lengths)
        assert len(self.lengths) == n
        self.nsyms = sum(1 for ln in self.lengths if ln)
        if check:
            assert self.nsyms >= 1 and (self.nsyms == 1 or kraft(self.lengths) == 1 << 15), "not a complete code"
        self.table = canonical(self.lengths) if self.nsyms > 1 and kraft(self.lengths) <= 1 << 15 else {}
        self.cl_syms = cl_syms if cl_syms is not None else cl_runs(self.lengths)
        hist = [0] * 19
        for s, _ in self.cl_syms:
            hist[s] += 1
        self.cl_len = list(cl_len) if cl_len is not None else limited_lengths(hist, 7)

    def write(self, bw: BitWriter) -> None:
        if self.simple is not None:
            syms, wide = self.simple
            bw.bits(1, 1)
            bw.bits(len(syms) - 1, 1)
            bw.bits(1 if wide else 0, 1)
            bw.bits(syms[0], 8 if wide else 1)
            if len(syms) == 2:
                bw.bits(syms[1], 8)
            return
        bw.bits(0, 1)
        nc = 19
        while nc > 4 and self.cl_len[CL_ORDER[nc - 1]] == 0:
            nc -= 1
        bw.bits(nc - 4, 4)
        for i in range(nc):
            bw.bits(self.cl_len[CL_ORDER[i]], 3)
        if self.max_symbol is None:
            bw.bits(0, 1)
        else:
            count, f = self.max_symbol
            bw.bits(1, 1)
            bw.bits(f, 3)
            bw.bits(count - 2, 2 + 2 * f)
        cl = canonical(self.cl_len) if sum(1 for ln in self.cl_len if ln) > 1 else {}
        for s, ev in self.cl_syms:
            if cl:
                bw.code(*cl[s])
            if s >= 16:
                bw.bits(ev, CL_EXTRA[s][0])

    def put(self, bw: BitWriter, s: int) -> None:
        if s in self.table:
            bw.code(*self.table[s])
        else:  # a code of one symbol is read with no bits; a damaged code is never reached
            assert not self.check or (self.nsyms == 1 and self.lengths[s]), (s, "not in the code")

    def facts(self) -> dict:
        """What the coverage test asks of a code."""
        f = {"n": self.n, "nsyms": self.nsyms, "maxlen": max(self.lengths), "simple": self.simple, "max_symbol": self.max_symbol}
        if self.simple is None:
            have, ends = 0, set()
            for s, ev in self.cl_syms:
                have += 1 if s < 16 else CL_EXTRA[s][1] + ev
                if s >= 16 and have == self.n:
                    ends.add(s)
            f.update(cl_first=self.cl_syms[0][0] if self.cl_syms else None, cl_ends=ends,
                     cl_single=sum(1 for ln in self.cl_len if ln) == 1, cl_count=len(self.cl_syms))
        return f


def auto_code(n: int, hist) -> Code:
    """A sound code for a histogram: the simple form where it fits, else Huffman lengths."""
    used = [s for s, c in enumerate(hist) if c]
    if not used:
        return Code(n, simple=([0], False))
    if len(used) <= 2 and used[-1] < 256:
        return Code(n, simple=(used, used[0] > 1))
    return Code(n, limited_lengths(list(hist) + [0] * (n - len(hist))))


def prefix(v: int):
    """(symbol, extra bits, extra value) of a length or a distance code v >= 1."""
    v -= 1
    if v < 4:
        return v, 0, 0
    hb = v.bit_length() - 1
    return 2 * hb + ((v >> (hb - 1)) & 1), hb - 1, v & ((1 << (hb - 1)) - 1)


def distance(code: int, xs: int) -> int:
    if code > 120:
        return code - 120
    dx, dy = DIST_MAP[code - 1]
    return max(1, dx + dy * xs)


def cache_slot(argb: int, bits: int) -> int:
    return ((0x1E35A7BD * argb) & 0xFFFFFFFF) >> (32 - bits)


class Stream:
    """An image stream: xs x ys ARGB words written as ``ops`` with a colour cache of ``cache_bits``
    (0: none).  ``codes``: {(group, alphabet 0..4): Code} for the codes not left to ``auto_code``.
    ``meta`` = (prefix bits, group index of every tile in row order, the entropy image's Stream or
    None for one of literals) gives the main image several groups; ``ngroups`` overrides the count
    of groups written.  ``cache_field`` overrides the 4-bit field alone (a damaged file);
    ``check`` = False lets a back-reference leave the image."""

    def __init__(self, xs, ys, ops, cache_bits=0, codes=None, meta=None, ngroups=None, cache_field=None, check=True):
        self.xs, self.ys, self.ops, self.cache_bits = xs, ys, list(ops), cache_bits
        self.codes, self.meta, self.ngroups, self.cache_field, self.check = dict(codes or {}), meta, ngroups, cache_field, check


def expand(st: Stream, rec: dict | None = None):
    """(ARGB words, tokens) of a stream's script.  A token: (position, green-alphabet symbol,
    [(alphabet, symbol, extra bits, extra value), ...] that follow it)."""
    total, bits = st.xs * st.ys, st.cache_bits
    px, toks, cache = [], [], [0] * (1 << bits)
    rec = {} if rec is None else rec
    note = lambda k, v: rec.setdefault(k, set()).add(v)  # noqa: E731
    run_slot, run_len, last_copy = -1, 0, 0
    for op in st.ops:
        pos = len(px)
        if op[0] == "lit":
            v = op[1]
            toks.append((pos, (v >> 8) & 255, [(1, (v >> 16) & 255, 0, 0), (2, v & 255, 0, 0), (3, v >> 24, 0, 0)]))
            px.append(v)
            if bits:
                s = cache_slot(v, bits)
                run_slot, run_len = s, run_len + 1 if s == run_slot else 1
            last_copy = 0
        elif op[0] in ("cache", "slot"):
            k = cache_slot(op[1], bits) if op[0] == "cache" else op[1]
            assert bits and k < (1 << bits) and (op[0] == "slot" or cache[k] == op[1]), (op, "not in the cache")
            toks.append((pos, 280 + k, []))
            px.append(cache[k])
            note("cache_sym", 280 + k)
            if k == run_slot:
                note("collide_run", run_len)
            if last_copy:
                note("cache_after_copy", last_copy)
            run_slot, run_len, last_copy = -1, 0, 0
        else:
            _, n, code = op
            ls, lb, lv = prefix(n)
            ds, db, dv = prefix(code)
            toks.append((pos, 256 + ls, [(0, None, lb, lv), (4, ds, db, dv)]))
            d = distance(code, st.xs)
            note("dist_code", code)
            note("len_extra", lb)
            note("dist_extra", db)
            if code <= 120 and sum(x * y for x, y in zip(DIST_MAP[code - 1], (1, st.xs))) < 1:
                note("dist_clamped", code)
            if d < n:
                note("overlap", d)
            if n >= 4096:
                note("copy4096_dist", d)
            if d > pos or n > total - pos:
                assert not st.check, (op, pos, "back-reference outside the image")
                note("copy_outside", "before" if d > pos else "past")
                break
            if pos + n == total:
                note("copy_to_end", n)
            for _ in range(n):
                px.append(px[-d])
            run_slot, run_len, last_copy = -1, 0, n
        for v in px[pos:]:
            if bits:
                cache[cache_slot(v, bits)] = v
    assert len(px) == total or not st.check, (len(px), total)
    return px, toks


def _write_stream(bw: BitWriter, st: Stream, main: bool, rec: dict, where: str) -> None:
    sub = rec.setdefault(where, {})
    px, toks = expand(st, sub)
    sub["cache_bits"] = st.cache_bits
    if not main:
        sub["greens"] = {(v >> 8) & 255 for v in px}
    field = st.cache_bits if st.cache_field is None else st.cache_field
    bw.bits(1 if (field or st.cache_field is not None) else 0, 1)
    if field or st.cache_field is not None:
        bw.bits(field, 4)
    ngroups, tile = 1, lambda x, y: 0  # noqa: E731
    if main:
        bw.bits(1 if st.meta else 0, 1)
        if st.meta:
            pb, idx, est = st.meta
            ew, eh = (st.xs + (1 << pb) - 1) >> pb, (st.ys + (1 << pb) - 1) >> pb
            assert len(idx) == ew * eh
            bw.bits(pb - 2, 3)
            est = est or Stream(ew, eh, [("lit", 0xFF000000 | (g << 8)) for g in idx])
            assert (est.xs, est.ys) == (ew, eh)
            assert [(v >> 8) & 0xFFFF for v in expand(est)[0]] == list(idx), "the entropy image's script is not the group list"
            _write_stream(bw, est, False, rec, "entropy")
            ngroups = max(idx) + 1
            tile = lambda x, y: idx[(y >> pb) * ew + (x >> pb)]  # noqa: E731
            sub["prefix_bits"] = pb
    ngroups = st.ngroups or ngroups
    sub["groups"] = ngroups
    sizes = [256 + 24 + ((1 << st.cache_bits) if st.cache_bits else 0), 256, 256, 256, 40]
    hist = [[[0] * n for n in sizes] for _ in range(ngroups)]
    grp = [tile(pos % st.xs, pos // st.xs) for pos, _, _ in toks]
    for g, (_, s0, rest) in zip(grp, toks):
        hist[g][0][s0] += 1
        for a, s, _, _ in rest:
            if s is not None:
                hist[g][a][s] += 1
    codes = [[st.codes.get((g, a)) or auto_code(sizes[a], hist[g][a]) for a in range(5)] for g in range(ngroups)]
    for g in range(ngroups):
        for a in range(5):
            assert codes[g][a].n == sizes[a]
            codes[g][a].write(bw)
            if g in grp or (g, a) in st.codes:
                sub.setdefault("codes", []).append((ALPHABETS[a], codes[g][a].facts()))
    sub["zero_bit_pixels"] = bool(toks) and all(codes[g][a].nsyms == 1 for g in set(grp) for a in range(5))
    sub["groups_used"] = len(set(grp))
    for g, (_, s0, rest) in zip(grp, toks):
        codes[g][0].put(bw, s0)
        for a, s, eb, ev in rest:
            if s is not None:
                codes[g][a].put(bw, s)
            bw.bits(ev, eb)


def vp8l(w: int, h: int, transforms, main_ops, *, alpha: int = 1, **kw):
    """(payload, record) of a w x h file.  ``transforms``, in stream order, any of
      (PREDICTOR, block bits, Stream)   the sub-image of modes (mode << 8) of its blocks
      (CROSS, block bits, Stream)       the sub-image of multipliers
      (GREEN,)
      (INDEX, colours, Stream)          the palette's colours x 1 stream, delta coded
    ``main_ops`` with ``kw`` make the main image's Stream (its width shrinks after an INDEX of
    at most 16 colours); the record's "nbits" is the stream's length in bits."""
    bw, rec = BitWriter(), {"transforms": [], "tbits": set()}
    bw.bits(0x2F, 8)
    bw.bits(w - 1, 14)
    bw.bits(h - 1, 14)
    bw.bits(alpha, 1)
    bw.bits(0, 3)
    xs = w
    for t in transforms:
        bw.bits(1, 1)
        bw.bits(t[0], 2)
        rec["transforms"].append(t[0])
        if t[0] in (PREDICTOR, CROSS):
            b = t[1]
            bw.bits(b - 2, 3)
            assert (t[2].xs, t[2].ys) == ((xs + (1 << b) - 1) >> b, (h + (1 << b) - 1) >> b), "sub-image size"
            _write_stream(bw, t[2], False, rec, "predictor" if t[0] == PREDICTOR else "cross")
            rec["tbits"].add((t[0], b))
        elif t[0] == INDEX:
            n = t[1]
            bw.bits(n - 1, 8)
            assert (t[2].xs, t[2].ys) == (n, 1)
            _write_stream(bw, t[2], False, rec, "palette")
            b = 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3
            xs = (xs + (1 << b) - 1) >> b
            rec["tbits"].add((INDEX, b))
            rec.setdefault("palette_sizes", set()).add(n)
    bw.bits(0, 1)
    _write_stream(bw, Stream(xs, h, main_ops, **kw), True, rec, "main")
    rec["nbits"] = bw.nbits
    out = bw.done()
    rec["bytes"] = len(out)
    return out, rec


# --- forward transforms: only so that residuals give the pixels a case wants ---
def _sub(a: int, b: int) -> int:  # per-channel difference mod 256
    return sum((((a >> s) - (b >> s)) & 255) << s for s in (0, 8, 16, 24))


def _avg2(a: int, b: int) -> int:
    return sum(((((a >> s) & 255) + ((b >> s) & 255)) >> 1) << s for s in (0, 8, 16, 24))


def _ch(v: int):
    return [(v >> s) & 255 for s in (0, 8, 16, 24)]


def predict(mode: int, L: int, T: int, TL: int, TR: int, clips: set | None = None) -> int:
    """The predictor of the specification; ``clips`` collects (mode, "low" / "high") where the
    clamp of modes 12 and 13 acts."""
    if mode in (0, 14, 15) or mode > 13:
        return 0xFF000000
    if mode <= 4:
        return (L, T, TR, TL)[mode - 1]
    if mode <= 10:
        return {5: _avg2(_avg2(L, TR), T), 6: _avg2(L, TL), 7: _avg2(L, T), 8: _avg2(TL, T), 9: _avg2(T, TR),
                10: _avg2(_avg2(L, TL), _avg2(T, TR))}[mode]
    l, t, tl = _ch(L), _ch(T), _ch(TL)
    if mode == 11:
        pl = sum(abs(a - b) for a, b in zip(t, tl))  # distance of L + T - TL to L
        pt = sum(abs(a - b) for a, b in zip(l, tl))
        if clips is not None:
            clips.add((11, "L" if pl < pt else "T"))
        return L if pl < pt else T
    out = 0
    for k in range(4):
        if mode == 12:
            v = l[k] + t[k] - tl[k]
        else:
            a = (l[k] + t[k]) >> 1
            v = a + int((a - tl[k]) / 2)  # the division rounds towards zero
        if clips is not None and not 0 <= v <= 255:
            clips.add((mode, "low" if v < 0 else "high"))
        out |= min(255, max(0, v)) << (8 * k)
    return out


def predictor_residuals(target, w: int, h: int, bits: int, modes, clips: set | None = None) -> list:
    """Residual ARGB words that a predictor transform of ``modes`` (one per block, row order)
    turns back into ``target`` (w * h words)."""
    bw_ = (w + (1 << bits) - 1) >> bits
    out = []
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if y == 0:
                p = 0xFF000000 if x == 0 else target[i - 1]
            elif x == 0:
                p = target[i - w]
            else:
                # the rightmost pixel's top-right is the next word in memory: its own row's first pixel
                p = predict(modes[(y >> bits) * bw_ + (x >> bits)], target[i - 1], target[i - w], target[i - w - 1],
                            target[i - w + 1], clips)
            out.append(_sub(target[i], p))
    return out

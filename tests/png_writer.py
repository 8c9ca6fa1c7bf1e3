"""Test-only PNG writer: every choice an encoder makes is an argument.

Pillow and zlib emit only what their encoders choose.  Here the caller picks the filter type of
every row, the deflate blocks (stored, fixed, or dynamic with given code lengths and a given
token sequence), the IDAT chunking, and any extra or damaged chunk.  Standard library and numpy
only.
"""

from __future__ import annotations

import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def chunk(cid: bytes, data: bytes = b"", crc: int | None = None) -> bytes:
    """One chunk; ``crc`` overrides the checksum (a damaged chunk)."""
    c = zlib.crc32(cid + data) & 0xFFFFFFFF if crc is None else crc
    return struct.pack(">I", len(data)) + cid + data + struct.pack(">I", c)


def ihdr(w: int, h: int, color: int, depth: int = 8, interlace: int = 0, comp: int = 0, filt: int = 0) -> bytes:
    return struct.pack(">IIBBBBB", w, h, depth, color, comp, filt, interlace)


def paeth(a: int, b: int, c: int) -> int:
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_rows(pix: np.ndarray, types) -> bytes:
    """Filtered scanlines of ``pix`` (H x W x C uint8); ``types[y]`` is row y's filter byte.  A
    type above 4 is written as it is, the row unfiltered (an invalid file)."""
    h, w, c = pix.shape
    rows = pix.reshape(h, w * c).astype(np.int32)
    out = bytearray()
    prev = np.zeros(w * c, np.int32)
    for y in range(h):
        t = int(types[y % len(types)])
        cur = rows[y]
        left = np.concatenate([np.zeros(c, np.int32), cur[:-c]]) if w * c > c else np.zeros(w * c, np.int32)
        ul = np.concatenate([np.zeros(c, np.int32), prev[:-c]]) if w * c > c else np.zeros(w * c, np.int32)
        if t == 1:
            f = cur - left
        elif t == 2:
            f = cur - prev
        elif t == 3:
            f = cur - ((left + prev) >> 1)
        elif t == 4:
            f = cur - np.array([paeth(int(a), int(b), int(cc)) for a, b, cc in zip(left, prev, ul)], np.int32)
        else:
            f = cur
        out.append(t)
        out += (f & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v: int, n: int) -> None:  # LSB first (header fields, extra bits)
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, n: int) -> None:  # Huffman codes go MSB first
        for i in range(n - 1, -1, -1):
            self.bits((code >> i) & 1, 1)

    def align(self) -> None:
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self) -> bytes:
        self.align()
        return bytes(self.out)


def canonical(lengths) -> dict:
    """symbol -> (code, length) of the canonical code (RFC 1951 3.2.2)."""
    cnt = [0] * 16
    for ln in lengths:
        cnt[ln] += 1
    cnt[0] = 0
    nxt = [0] * 17
    code = 0
    for b in range(1, 16):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lengths):
        if ln:
            out[s] = (nxt[ln], ln)
            nxt[ln] += 1
    return out


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


def len_sym(n: int):
    for i in range(28, -1, -1):
        if n >= LEN_BASE[i]:
            return 257 + i, LEN_EXTRA[i], n - LEN_BASE[i]
    raise ValueError(n)


def dist_sym(d: int):
    for i in range(29, -1, -1):
        if d >= DIST_BASE[i]:
            return i, DIST_EXTRA[i], d - DIST_BASE[i]
    raise ValueError(d)


def put_tokens(bw: BitWriter, tokens, ll: dict, dd: dict) -> None:
    """Tokens: an int literal, a (length, distance) match, or ("raw", code, nbits) for bits
    written as they are (an invalid code), or ("sym", s) for a bare literal/length symbol."""
    for t in tokens:
        if isinstance(t, (int, np.integer)):
            bw.code(*ll[int(t)])
        elif t[0] == "raw":
            bw.code(t[1], t[2])
        elif t[0] == "sym":
            bw.code(*ll[t[1]])
        elif t[0] == "dsym":  # a match with a bare distance symbol (30, 31: invalid)
            s, eb, ev = len_sym(t[1])
            bw.code(*ll[s])
            bw.bits(ev, eb)
            bw.code(*dd[t[2]])
        else:
            n, d = t
            s, eb, ev = len_sym(n)
            bw.code(*ll[s])
            bw.bits(ev, eb)
            s, eb, ev = dist_sym(d)
            bw.code(*dd[s])
            bw.bits(ev, eb)
    bw.code(*ll[256])


def cl_runs(lengths) -> list:
    """Code-length symbols for ``lengths`` with runs 16 / 17 / 18 wherever they apply (greedy),
    over the whole literal/length + distance sequence: runs cross the HLIT / HDIST boundary."""
    out = []
    i = 0
    n = len(lengths)
    while i < n:
        v = lengths[i]
        j = i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            r = min(run, 138)
            out.append((18, r - 11, 7) if r >= 11 else (17, r - 3, 3))
            i += r
        elif v != 0 and run >= 4:
            out.append((v, 0, 0))
            r = min(run - 1, 6)
            out.append((16, r - 3, 2))
            i += 1 + r
        else:
            out.append((v, 0, 0))
            i += 1
    return out


def block_stored(bw: BitWriter, data: bytes, final: bool, nlen: int | None = None) -> None:
    bw.bits(1 if final else 0, 1)
    bw.bits(0, 2)
    bw.align()
    n = len(data)
    bw.out += struct.pack("<HH", n, (n ^ 0xFFFF) if nlen is None else nlen) + data


def block_fixed(bw: BitWriter, tokens, final: bool) -> None:
    bw.bits(1 if final else 0, 1)
    bw.bits(1, 2)
    put_tokens(bw, tokens, canonical(FIXED_LL), canonical(FIXED_D + [5, 5]))


def block_dynamic(bw: BitWriter, tokens, ll_len, d_len, final: bool, cl_syms=None, cl_len=None) -> None:
    """Dynamic block with the given code lengths (HLIT = len(ll_len), HDIST = len(d_len)).
    ``cl_syms`` overrides the run-length coding of the lengths, ``cl_len`` the code-length code."""
    bw.bits(1 if final else 0, 1)
    bw.bits(2, 2)
    syms = cl_syms if cl_syms is not None else cl_runs(list(ll_len) + list(d_len))
    if cl_len is None:
        # a complete code over the used symbols: 2^nb - n of them one bit shorter than the rest
        used = sorted({s for s, _, _ in syms})
        if len(used) == 1:
            used.append((used[0] + 1) % 19)
        nb = (len(used) - 1).bit_length()
        short = (1 << nb) - len(used)
        cl_len = [0] * 19
        for k, s in enumerate(used):
            cl_len[s] = nb - 1 if k < short else nb
    cl = canonical(cl_len)
    hclen = 19
    while hclen > 4 and cl_len[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    bw.bits(len(ll_len) - 257, 5)
    bw.bits(len(d_len) - 1, 5)
    bw.bits(hclen - 4, 4)
    for i in range(hclen):
        bw.bits(cl_len[CL_ORDER[i]], 3)
    for s, ev, eb in syms:
        bw.code(*cl[s])
        bw.bits(ev, eb)
    put_tokens(bw, tokens, canonical(ll_len), canonical(d_len))


def expand(tokens) -> bytes:
    """The bytes a token sequence stands for (literals and matches only), given none before."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, (int, np.integer)):
            out.append(int(t))
        else:
            n, d = t
            for _ in range(n):
                out.append(out[-d])
    return bytes(out)


def zlib_wrap(deflate: bytes, data: bytes, cmf: int = 0x78, flg: int | None = None, adler: int | None = None) -> bytes:
    """zlib stream around raw deflate bytes; ``data`` is what they inflate to (for Adler-32)."""
    if flg is None:
        flg = 0x80
        flg += 31 - ((cmf << 8) + flg) % 31
    a = zlib.adler32(data) & 0xFFFFFFFF if adler is None else adler
    return bytes([cmf, flg]) + deflate + struct.pack(">I", a)


def split_idat(stream: bytes, sizes) -> list:
    """IDAT chunks of the given payload sizes (cycled; the rest in one last chunk when sizes end
    with None)."""
    out = []
    pos = 0
    k = 0
    while pos < len(stream) or (k < len(sizes) and sizes[k] == 0):
        s = sizes[k % len(sizes)] if sizes[-1] is not None or k < len(sizes) - 1 else None
        if s is None:
            s = len(stream) - pos
        out.append(chunk(b"IDAT", stream[pos:pos + s]))
        pos += s
        k += 1
        if k > 100000:
            break
    return out


def png(w: int, h: int, color: int, stream: bytes, idat_sizes=None, before=(), between=(), after=(), depth: int = 8,
        interlace: int = 0, plte: bytes | None = None, trns: bytes | None = None, iend: bool = True,
        ihdr_crc: int | None = None, signature: bytes = SIGNATURE, tail: bytes = b"") -> bytes:
    """A PNG file around the zlib stream ``stream``.  ``before`` / ``after``: whole chunks (bytes)
    before PLTE and after the IDAT run; ``between``: chunks put after the first IDAT chunk."""
    parts = [signature, chunk(b"IHDR", ihdr(w, h, color, depth, interlace), ihdr_crc)]
    parts += list(before)
    if plte is not None:
        parts.append(chunk(b"PLTE", plte))
    if trns is not None:
        parts.append(chunk(b"tRNS", trns))
    idats = split_idat(stream, idat_sizes) if idat_sizes else [chunk(b"IDAT", stream)]
    parts.append(idats[0])
    parts += list(between)
    parts += idats[1:]
    parts += list(after)
    if iend:
        parts.append(chunk(b"IEND"))
    return b"".join(parts) + tail


def simple(pix: np.ndarray, color: int, types=(0,), level: int = 6, **kw) -> bytes:
    """``pix`` (H x W x C) through zlib at ``level`` with the given row filters."""
    h, w, _ = pix.shape
    return png(w, h, color, zlib.compress(filter_rows(pix, types), level), **kw)

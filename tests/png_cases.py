"""PNG case list shared by tests/test_png_cpu.py (host model) and tests/test_gpu_png.py.

Each case is (name, file bytes, expectation): "dev" — the device decodes it (probe kind 4) to
Pillow's pixels; "raise" — kind 4 and Pillow raises (status -1 after the decode); "corrupt" —
Pillow raises at open (probe kind -1); "declined" — probe kind 5, Pillow decides.  The files are
the smallest at which each mechanism can go wrong; png_writer builds what no encoder emits.
"""

from __future__ import annotations

import functools
import io
import struct
import zlib

import numpy as np

from tests import png_writer as pw


def pillow_rgb(b: bytes):
    """np.asarray(Image.open(b).convert("RGB")), or None where Pillow raises (cpu.py:251-253)."""
    import warnings

    from PIL import Image
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (Pillow's advice to convert palette transparency to RGBA)
            return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
    except Exception:  # noqa: BLE001
        return None


def _pix(h, w, c, seed=0, coarse=False):
    rng = np.random.default_rng(seed + 1000 * h + 10 * w + c)
    p = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    return (p // 64 * 64).astype(np.uint8) if coarse else p


COLOR_OF = {1: 0, 2: 4, 3: 2, 4: 6}


def _wrap(w, h, color, deflate, raw, **kw):
    return pw.png(w, h, color, pw.zlib_wrap(deflate, raw), **kw)


def _complete(lens_used: dict, nsym: int, maxbits: int):
    """Code lengths over nsym symbols: the given ones, the remaining code space filled by unused
    symbols (from the top) so that the code is complete."""
    lens = [0] * nsym
    for s, ln in lens_used.items():
        lens[s] = ln
    left = (1 << maxbits) - sum(1 << (maxbits - ln) for ln in lens_used.values())
    assert left >= 0
    free = [s for s in range(nsym - 1, -1, -1) if s not in lens_used]
    ln = 1
    while left > 0:
        unit = 1 << (maxbits - ln)
        if unit <= left:
            lens[free.pop(0)] = ln
            left -= unit
        else:
            ln += 1
    return lens


def _crossing(ll_len, d_len) -> list:
    """Code-length symbols of pw.cl_runs whose run starts in the literal/length lengths and ends
    in the distance lengths."""
    out, i = [], 0
    for s, ev, _ in pw.cl_runs(list(ll_len) + list(d_len)):
        n = 1 if s < 16 else (3 + ev if s in (16, 17) else 11 + ev)
        if s >= 16 and i < len(ll_len) < i + n:
            out.append(s)
        i += n
    return out


@functools.lru_cache(maxsize=1)
def cases() -> list:
    out = []

    def add(name, b, exp):
        out.append((name, b, exp))

    # ---- filters: each type on every row incl. the first, widths / heights 1, bpp 1..4, band edges
    for bpp in (1, 2, 3, 4):
        for f in range(5):
            add(f"filter{f}_bpp{bpp}", pw.simple(_pix(3, 5, bpp, f), COLOR_OF[bpp], types=(f,)), "dev")
    add("width1", pw.simple(_pix(9, 1, 3), 2, types=(4, 3, 1, 2, 0)), "dev")
    add("height1", pw.simple(_pix(1, 9, 4), 6, types=(4,)), "dev")
    for rows in (63, 64, 65, 129):
        add(f"rows{rows}", pw.simple(_pix(rows, 3, 3, rows), 2, types=(3, 4)), "dev")
    add("alternate5", pw.simple(_pix(23, 17, 3), 2, types=(0, 1, 2, 3, 4)), "dev")
    tie = np.zeros((4, 6, 1), np.uint8)  # Paeth ties: pa == pb, pb == pc, all equal
    tie[0] = [[10], [20], [10], [20], [30], [30]]
    tie[1] = [[20], [10], [20], [10], [30], [40]]
    tie[2] = [[20], [20], [20], [20], [20], [20]]
    tie[3] = [[30], [10], [30], [10], [40], [20]]
    add("paeth_ties", pw.simple(tie, 0, types=(4,)), "dev")

    # ---- blocks
    pix = _pix(4, 4, 3)
    raw = pw.filter_rows(pix, (0,))
    bw = pw.BitWriter(); pw.block_stored(bw, b"", False); pw.block_stored(bw, raw, True)
    add("stored_empty_first", _wrap(4, 4, 2, bw.done(), raw), "dev")
    bw = pw.BitWriter(); pw.block_fixed(bw, list(raw[:5]), False); pw.block_stored(bw, raw[5:], True)
    add("stored_midbyte", _wrap(4, 4, 2, bw.done(), raw), "dev")
    bw = pw.BitWriter(); pw.block_fixed(bw, list(raw), True)
    add("fixed", _wrap(4, 4, 2, bw.done(), raw), "dev")
    bw = pw.BitWriter(); pw.block_fixed(bw, list(raw), False); pw.block_stored(bw, b"", True)
    add("final_empty", _wrap(4, 4, 2, bw.done(), raw), "dev")
    bw = pw.BitWriter()
    q = len(raw) // 5
    pw.block_stored(bw, raw[:q], False); pw.block_fixed(bw, list(raw[q:2 * q]), False)
    used = sorted(set(raw[2 * q:3 * q]) | {256})
    ll = _complete({s: 8 for s in used}, 286, 9) if len(used) <= 256 else None
    pw.block_dynamic(bw, list(raw[2 * q:3 * q]), ll, [1], False)
    pw.block_stored(bw, raw[3 * q:4 * q], False); pw.block_fixed(bw, list(raw[4 * q:]), True)
    add("five_blocks", _wrap(4, 4, 2, bw.done(), raw), "dev")
    big = _pix(128, 171, 3, 5)  # 128 x 514 = 65792 bytes: one stored block of 65535
    rawb = pw.filter_rows(big, (1,))
    bw = pw.BitWriter(); pw.block_stored(bw, rawb[:65535], False); pw.block_stored(bw, rawb[65535:], True)
    add("stored_65535", _wrap(171, 128, 2, bw.done(), rawb), "dev")

    # dynamic: one-code distance tree, matches of length 3 / 258, dist 1 with 258, dist < len with len % dist != 0
    # (every byte is 0..4, so whatever lands on a row's first byte is a valid filter type)
    toks = [0, 3, 1, 4, (258, 1), (3, 1), 1, 2, 3, 4, 0, (13, 5), (258, 7)]
    toks += [2] * (12 * 100 - len(pw.expand(toks)))
    body = pw.expand(toks)
    lits = {t for t in toks if isinstance(t, int)} | {256}
    lens_syms = {pw.len_sym(t[0])[0] for t in toks if not isinstance(t, int)}
    dist_syms = {pw.dist_sym(t[1])[0] for t in toks if not isinstance(t, int)}
    ll = _complete({s: 6 for s in sorted(lits | lens_syms)}, 286, 7)
    dl = _complete({s: 3 for s in sorted(dist_syms)}, 30, 4)
    bw = pw.BitWriter(); pw.block_dynamic(bw, toks, ll, dl, True)
    add("matches", _wrap(99, 12, 0, bw.done(), body), "dev")
    # a one-code distance tree (incomplete, allowed): every match at distance 1
    rawd = bytes([0]) + bytes([9]) * 403
    toksd = [0, 9, (258, 1), (144, 1)]
    assert pw.expand(toksd) == rawd
    ll = _complete({0: 2, 9: 2, 256: 2, 285: 3, pw.len_sym(144)[0]: 3}, 286, 3)
    bw = pw.BitWriter(); pw.block_dynamic(bw, toksd, ll, [1], True)
    add("one_code_dist", _wrap(403, 1, 0, bw.done(), rawd), "dev")
    # every literal/length symbol at 15 bits, and at the lookahead width (9) and one more (10)
    for width in (9, 10, 15):
        syms = list(range(0, 250)) + [256]
        lensw = _complete({s: width for s in syms}, 286, width)
        rawl = bytes([0]) + bytes(range(0, 250)) * 2
        bw = pw.BitWriter(); pw.block_dynamic(bw, list(rawl), lensw, [1], True)
        add(f"all_{width}bit", _wrap(500, 1, 0, bw.done(), rawl), "dev")
    # code-length runs 16 / 17 / 18 across the HLIT / HDIST boundary (cl_runs runs over both)
    llr = [0] * 257
    llr[0] = llr[1] = 2; llr[256] = 2
    llr += [3] * 2                     # 257, 258 at 3 bits: the run of 3s continues into the distances
    dlr = [3, 3, 3, 3, 3, 3, 3, 3]      # a complete 3-bit distance code
    # complete the literal code: 2+2+2 -> 3/4, + 2 x 1/8 = 1
    rawr = bytes([0, 1, 1, 0, 1, 0, 1, 0, 1])
    bw = pw.BitWriter(); pw.block_dynamic(bw, [0, 1, 1, 0, (4, 2), 1], llr, dlr, True)
    add("clrun_16_boundary", _wrap(8, 1, 0, bw.done(), rawr), "dev")
    assert _crossing(llr, dlr) == [16]
    # HLIT above 257 with trailing zero lengths that run on into leading zero distance lengths:
    # one zero run of 3..10 (symbol 17) and one of 11 or more (symbol 18) across the boundary
    for name, tail, lead, want in (("clrun_17_boundary", 5, 3, 17), ("clrun_18_boundary", 13, 4, 18)):
        llz = [2, 2] + [0] * 254 + [1] + [0] * tail
        dlz = [0] * lead + [1]          # one distance code (a single-code tree)
        assert _crossing(llz, dlz) == [want], (name, _crossing(llz, dlz))
        bw = pw.BitWriter(); pw.block_dynamic(bw, list(rawr), llz, dlz, True)
        add(name, _wrap(8, 1, 0, bw.done(), rawr), "dev")

    # ---- matches at distance 32768 and across the ring's wrap at 32 KiB and 64 KiB of output
    # (bytes 0..4 again: any of them is a valid filter byte)
    roww = bytes(np.random.default_rng(9).integers(0, 5, 200 * 901, dtype=np.uint8))
    toksw = list(roww[:32768]) + [(258, 32768)]
    done = pw.expand(toksw)
    toksw += list(roww[len(done):65536 - 100])  # literals up to 100 bytes short of 64 KiB
    toksw += [(258, 30000), (258, 32768), (200, 258), (258, 97)]
    done = pw.expand(toksw)
    toksw += list(roww[len(done):])
    done = pw.expand(toksw)
    assert len(done) == 200 * 901
    bw = pw.BitWriter(); pw.block_fixed(bw, toksw, True)
    add("ring_wrap", _wrap(300, 200, 2, bw.done(), bytes(done)), "dev")
    add("zlib_300x200", pw.simple(_pix(200, 300, 3, 4, coarse=True), 2, types=(0, 1, 2, 3, 4)), "dev")

    # ---- containers
    z = zlib.compress(pw.filter_rows(pix, (4, 1)))
    add("idat_every_byte", pw.png(4, 4, 2, z, idat_sizes=[1]), "dev")
    add("idat_zero_len", pw.png(4, 4, 2, z, idat_sizes=[0, 1, 0, 0, 2, None]), "dev")
    zb = zlib.compress(pw.filter_rows(_pix(30, 40, 3), (0,)), 0)
    add("idat_300_chunks", pw.png(40, 30, 2, zb, idat_sizes=[(len(zb) + 299) // 300]), "dev")
    anc = [pw.chunk(b"gAMA", struct.pack(">I", 45455)), pw.chunk(b"sRGB", b"\0"), pw.chunk(b"pHYs", b"\0" * 9)]
    add("ancillary_before", pw.png(4, 4, 2, z, before=anc), "dev")
    add("ancillary_between", pw.png(4, 4, 2, z, idat_sizes=[5, None], between=[pw.chunk(b"tIME", b"\0" * 7)]), "declined")
    add("ancillary_after", pw.png(4, 4, 2, z, after=[pw.chunk(b"tEXt", b"a\0b")]), "declined")
    add("trns_gray", pw.simple(_pix(3, 5, 1), 0, trns=b"\0\x07"), "dev")
    add("trns_rgb", pw.simple(pix, 2, trns=b"\0\x01\0\x02\0\x03"), "dev")
    idx = _pix(5, 7, 1, 3) % 6
    pal = bytes(_pix(1, 6, 3, 8).tobytes())
    add("palette", pw.simple(idx.astype(np.uint8), 3, plte=pal), "dev")
    add("palette_trns", pw.simple(idx.astype(np.uint8), 3, plte=pal, trns=bytes([0, 128, 255])), "dev")
    idx2 = idx.copy(); idx2[2, 2] = 200
    add("palette_short", pw.simple(idx2.astype(np.uint8), 3, plte=pal), "dev")
    add("palette_missing", pw.simple(idx.astype(np.uint8), 3), "declined")
    add("iccp", pw.png(4, 4, 2, z, before=[pw.chunk(b"iCCP", b"x\0\0" + zlib.compress(b"p" * 200))]), "declined")

    # ---- damaged files
    add("bad_signature", pw.png(4, 4, 2, z, signature=b"\x89PNG\r\n\x1a\x0b"), "corrupt")
    add("bad_ihdr_crc", pw.png(4, 4, 2, z, ihdr_crc=1), "corrupt")
    add("bad_plte_crc", pw.png(5, 7, 3, zlib.compress(pw.filter_rows(idx.astype(np.uint8), (0,))),
                               before=[pw.chunk(b"PLTE", pal, crc=7)]), "corrupt")
    add("bad_gama_crc", pw.png(4, 4, 2, z, before=[pw.chunk(b"gAMA", b"\0\0\xb1\x8f", crc=5)]), "corrupt")
    add("bad_idat_crc", pw.SIGNATURE + pw.chunk(b"IHDR", pw.ihdr(4, 4, 2)) + pw.chunk(b"IDAT", z, crc=3) + pw.chunk(b"IEND"), "dev")
    # the stream cut short: inside the Adler-32 Pillow still has every row; one byte more is the
    # first cut that takes the end of the last block away (pins Inflater::overrun)
    assert zlib.decompressobj().decompress(z[:-4]) == pw.filter_rows(pix, (4, 1))
    add("stream_short_1", pw.png(4, 4, 2, z[:-1]), "dev")
    add("stream_short_4", pw.png(4, 4, 2, z[:-4]), "dev")
    add("stream_short_5", pw.png(4, 4, 2, z[:-5]), "raise")
    bw = pw.BitWriter(); bw.bits(1, 1); bw.bits(3, 2)
    add("block_type_3", pw.png(4, 4, 2, pw.zlib_wrap(bw.done() + b"\0" * 20, raw)), "raise")
    # (a complete code has no unused pattern: the fixed code's length symbol 286 is the invalid one)
    bw = pw.BitWriter(); pw.block_fixed(bw, list(raw[:9]) + [("sym", 286)] + list(raw[9:]), True)
    add("invalid_code", pw.png(4, 4, 2, pw.zlib_wrap(bw.done(), raw)), "raise")
    bw = pw.BitWriter(); pw.block_fixed(bw, list(raw[:9]) + [("dsym", 3, 30)] + list(raw[12:]), True)
    add("invalid_dist_code", pw.png(4, 4, 2, pw.zlib_wrap(bw.done(), raw)), "raise")
    bw = pw.BitWriter(); pw.block_fixed(bw, [1, 2, 3, (3, 4)] + list(raw[6:]), True)
    add("dist_before_start", pw.png(4, 4, 2, pw.zlib_wrap(bw.done(), raw)), "raise")
    r5 = bytearray(raw); r5[13 * 2] = 5
    add("filter_byte_5", pw.png(4, 4, 2, zlib.compress(bytes(r5))), "raise")
    add("fdict", pw.png(4, 4, 2, bytes([0x78, 0xBB]) + z[2:]), "raise")
    add("bad_fcheck", pw.png(4, 4, 2, bytes([0x78, 0x9D]) + z[2:]), "raise")
    add("cm_7", pw.png(4, 4, 2, bytes([0x77, 0x9D]) + z[2:]), "raise")
    bw = pw.BitWriter(); pw.block_stored(bw, raw, True, nlen=0x1234)
    add("stored_nlen", pw.png(4, 4, 2, pw.zlib_wrap(bw.done(), raw)), "raise")
    add("data_after_stream", pw.png(4, 4, 2, z + b"garbage"), "dev")
    add("more_rows_than_h", pw.png(4, 4, 2, zlib.compress(raw + raw)), "dev")
    add("missing_iend", pw.png(4, 4, 2, z, iend=False), "dev")
    add("missing_iend_tail", pw.png(4, 4, 2, z, iend=False, tail=b"abcdefghijklmnop"), "declined")
    # a valid stream that ends after three of the four rows (Pillow keeps the rows)
    add("stream_ends_at_row_3", pw.png(4, 4, 2, zlib.compress(raw[:13 * 3])), "gap")
    add("adler_mismatch", pw.png(4, 4, 2, z[:-4] + b"\0\0\0\0"), "gap")  # post-stream

    # ---- declined flavours
    from PIL import Image
    for depth, color in ((1, 0), (2, 0), (4, 3), (16, 2)):
        im = Image.fromarray(_pix(6, 8, 3, depth))
        if color == 0:
            im = im.convert("L")
        bio = io.BytesIO()
        if depth == 16:
            Image.fromarray((_pix(6, 8, 1, 2).astype(np.uint16)[:, :, 0] * 257)).save(bio, "PNG")
        elif color == 3:
            im.quantize(16).save(bio, "PNG", bits=4)
        else:
            im.point(lambda v: v >> (8 - depth) << (8 - depth)).convert("1" if depth == 1 else "L").save(bio, "PNG", bits=depth)
        data = bio.getvalue()
        if depth == 2:  # (Pillow writes no 2-bit gray: the writer does)
            data = pw.png(8, 6, 0, zlib.compress(bytes([0, 0x1B, 0xE4] * 6)), depth=2)
        add(f"depth{depth}", data, "declined")
    add("adam7", pw.png(4, 4, 2, z, interlace=1), "declined")
    bio = io.BytesIO()
    Image.fromarray(_pix(5, 5, 3)).save(bio, "PNG", save_all=True, append_images=[Image.fromarray(_pix(5, 5, 3, 1))])
    add("apng", bio.getvalue(), "declined")
    return out

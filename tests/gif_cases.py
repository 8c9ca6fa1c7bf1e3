"""GIF files for tests/test_gif_cpu.py and tests/test_gpu_gif.py: written by Pillow where its
encoder can, packed by hand (``pack`` / ``gif_file``) where it cannot.

``cases()`` -> [(name, bytes, expect)] with expect "dev" (a context with ``gif`` on decodes it
and Pillow gives the same pixels), "corrupt" (it is the device's, and Pillow raises on the
stream: status -1), "declined" (a GIF Pillow decides) or "none" (Pillow raises at open: status -1)."""

import functools
import io
import struct

import numpy as np
from PIL import Image


def _save(a: np.ndarray, pal: np.ndarray, **kw) -> bytes:
    im = Image.fromarray(a.astype(np.uint8), "P")
    im.putpalette(pal.astype(np.uint8).tobytes())
    f = io.BytesIO()
    im.save(f, "GIF", **kw)
    return f.getvalue()


def pack(codes, bits: int, blocks=(255,)) -> bytes:
    """The codes as an LZW bit stream (the width grows with the codes since the last clear, 12 at
    most) cut into sub-blocks of the given lengths in turn, without the terminator."""
    clear, acc, nb, j, raw = 1 << bits, 0, 0, 0, bytearray()
    for c in codes:
        fill = min(4096, clear + 2 + max(0, j - 1))
        acc |= int(c) << nb
        nb += min(12, max(bits + 1, fill.bit_length()))
        while nb >= 8:
            raw.append(acc & 255)
            acc >>= 8
            nb -= 8
        j = 0 if c == clear else j + 1
    if nb:
        raw.append(acc)
    out, k = bytearray(), 0
    while raw:
        n = blocks[k % len(blocks)]
        out += bytes([len(raw[:n])]) + raw[:n]
        raw, k = raw[n:], k + 1
    return bytes(out)


def gif_file(w, h, bits, payload, gct=None, lct=None, lace=False, frame=None, ext=b"", end=b"\0;") -> bytes:
    """A one-image file around sub-blocks; tables as bytes of 3 x 2^k."""
    def flag(t):
        return 0 if t is None else 0x80 | ((len(t) // 3).bit_length() - 2)
    out = b"GIF89a" + struct.pack("<HHBBB", w, h, flag(gct), 0, 0) + (gct or b"") + ext
    out += b"," + struct.pack("<HHHHB", *(frame or (0, 0, w, h)), flag(lct) | (0x40 if lace else 0)) + (lct or b"")
    return out + bytes([bits]) + payload + end


def _literals(px, bits, every=100, lead=True, tail=True):
    """The indices as literal codes with a clear code every `every` codes (0: never)."""
    clear, codes = 1 << bits, []
    for i, v in enumerate(np.asarray(px).ravel().tolist()):
        if (lead and i == 0) or (every and i and i % every == 0):
            codes.append(clear)
        codes.append(v)
    return codes + ([clear + 1] if tail else [])


def _lace_order(h):
    return [y for s, d in ((0, 8), (4, 8), (2, 4), (1, 2)) for y in range(s, h, d)]


@functools.lru_cache(maxsize=None)
def cases():
    r = np.random.default_rng(3)
    pal = r.integers(0, 256, (256, 3))
    tab = pal.astype(np.uint8).tobytes()
    out = [("noise256_96x80", _save(r.integers(0, 256, (80, 96)), pal), "dev")]  # the table fills and clears: widths 9..12
    out.append(("flat_200x100", _save(np.full((100, 200), 5), pal), "dev"))      # KwKwK chains, long strings
    out += [(f"colours{n}_{w}x{h}", _save(r.integers(0, n, (h, w)), pal[:n]), "dev") for n, w, h in ((4, 21, 17), (16, 19, 23))]
    out += [(f"size_{w}x{h}", _save(r.integers(0, 8, (h, w)), pal), "dev") for w, h in ((1, 1), (1, 70), (70, 1), (63, 5), (64, 5), (65, 5))]
    y, x = np.mgrid[:50, :37]
    out.append(("lace_pillow_37x50", _save((x // 3 + y // 2) % 32, pal, interlace=True), "dev"))
    for h in (1, 2, 3, 4, 5, 6, 7, 8, 9, 50):
        a = r.integers(0, 256, (h, 5))
        out.append((f"lace_h{h}", gif_file(5, h, 8, pack(_literals(a[_lace_order(h)], 8), 8), gct=tab, lace=True), "dev"))
    out.append(("gif87a", _save(r.integers(0, 8, (9, 11)), pal), "dev"))
    assert out[-1][1][:6] == b"GIF87a"
    a, lct = r.integers(0, 4, (6, 7)), tab[300:312]
    out.append(("local_only", gif_file(7, 6, 2, pack(_literals(a, 2), 2), lct=lct), "dev"))
    out.append(("local_over_global", gif_file(7, 6, 2, pack(_literals(a, 2), 2), gct=tab[:24], lct=lct), "dev"))
    out.append(("transparency", _save(r.integers(0, 16, (12, 10)), pal[:16], transparency=3), "dev"))
    frames = [Image.fromarray(r.integers(0, 8, (14, 15)).astype(np.uint8), "P") for _ in range(3)]
    for im in frames:
        im.putpalette(tab)
    f = io.BytesIO()
    frames[0].save(f, "GIF", save_all=True, append_images=frames[1:], duration=40, loop=0)
    out.append(("animation3", f.getvalue(), "dev"))
    big = r.integers(0, 256, (50, 100))  # (from here on packed by hand) 5000 literals without a clear: the table fills and stays
    out.append(("deferred_clear", gif_file(100, 50, 8, pack(_literals(big, 8, every=0), 8), gct=tab), "dev"))
    small = r.integers(0, 8, (13, 31))
    for name, codes, blocks in (("clear_every_37", _literals(small, 3, every=36), (255,)),
                                ("no_leading_clear", _literals(small, 3, every=0, lead=False), (255,)),
                                ("no_end_code", _literals(small, 3, tail=False), (255,)),
                                ("surplus_pixels", _literals(np.concatenate([small.ravel(), small.ravel()[:99]]), 3), (255,)),
                                ("blocks_1_7_254", _literals(small, 3), (1, 7, 254))):
        out.append((name, gif_file(31, 13, 3, pack(codes, 3, blocks), gct=tab), "dev"))
    # KwKwK right after a clear, and a run that doubles: 0, then the entry being created, again and again
    out.append(("kwkwk_chain", gif_file(9, 5, 2, pack([4, 1] + list(range(6, 14)) + [5], 2), gct=tab), "dev"))
    out.append(("short_table", gif_file(31, 13, 3, pack(_literals(small, 3), 3), lct=tab[:12]), "dev"))  # indices 4..7: black
    comment = b"!\xfe\x05hello\0" + b"!\xff\x0bNETSCAPE2.0\x03\x01\0\0\0" + b"!\xf9\x04\x01\0\0\x02\0"
    out.append(("extensions_no_trailer", gif_file(31, 13, 3, pack(_literals(small, 3), 3), gct=tab, ext=comment, end=b"\0"), "dev"))
    # corrupt streams: Pillow raises
    cut = _literals(small, 3)
    out.append(("early_end_code", gif_file(31, 13, 3, pack(cut[:200] + [9], 3), gct=tab), "corrupt"))
    whole = gif_file(31, 13, 3, pack(cut, 3), gct=tab)
    out.append(("cut_mid_block", whole[:len(whole) - 80], "corrupt"))
    out.append(("cut_last_byte", whole[:-3], "corrupt"))  # the cut block holds every pixel: Pillow does not read it
    out.append(("code_above_next", gif_file(31, 13, 3, pack([8, 1, 2, 13] + cut[1:], 3), gct=tab), "corrupt"))
    # a GIF Pillow decides
    out.append(("sub_screen_frame", gif_file(31, 13, 3, pack(_literals(small[:12, :30], 3), 3), gct=tab, frame=(1, 1, 30, 12)), "declined"))
    out.append(("no_table", gif_file(31, 13, 3, pack(_literals(small, 3), 3)), "declined"))
    out.append(("code_size_9", gif_file(31, 13, 9, pack(_literals(small, 3), 3), gct=tab), "declined"))
    ramp = bytes(v for i in range(8) for v in (i, i, i))  # Pillow opens a gray-ramp table as "L"
    out += [(n, gif_file(31, 13, 3, pack(_literals(small, 3), 3), **kw), "declined")
            for n, kw in (("ramp_table", {"gct": ramp}), ("ramp_short_local", {"gct": tab, "lct": ramp[:12]}))]
    out.append(("zero_width", gif_file(0, 13, 3, pack(_literals(small, 3), 3), gct=tab), "none"))
    xmp = b"!\xff\x0bXMP DataXMP\x03abc\0"
    out.append(("xmp_extension", gif_file(31, 13, 3, pack(_literals(small, 3), 3), gct=tab, ext=xmp), "declined"))
    return out

"""WebP files for tests/test_webp_cpu.py and tests/test_gpu_webp.py, encoded by Pillow at test time.

``cases()`` -> [(name, bytes, expect)] with expect "dev" (a context with ``webp`` on decodes it),
"declined" (a WebP Pillow decides) or "none" (no WebP).  The "dev" files are the smallest that
cross each boundary of the decoder: every transform, bundling of 1 / 2 / 4 index bits, a colour
cache, several groups of codes, both kinds of distance code, more than 64 rows and more than
2 x 64 + 3 columns."""

import functools
import io

import numpy as np
from PIL import Image


def _enc(a: np.ndarray, **kw) -> bytes:
    f = io.BytesIO()
    Image.fromarray(a).save(f, "WEBP", lossless=True, **kw)
    return f.getvalue()


def _gradient(r, w, h):
    y, x = np.mgrid[:h, :w]
    return ((np.stack([x * 5 + y, y * 4, x + y * 3], -1) + r.integers(0, 6, (h, w, 3))) % 256).astype(np.uint8)


def _palette(r, w, h, n):
    return r.integers(0, 256, (n, 3)).astype(np.uint8)[r.integers(0, n, (h, w))]


def payload(b: bytes) -> bytearray:
    """The VP8L payload of a bare RIFF / WEBP / VP8L file."""
    assert b[12:16] == b"VP8L"
    return bytearray(b[20:20 + int.from_bytes(b[16:20], "little")])


def riff(p: bytes) -> bytes:
    """The bare file around a VP8L payload."""
    body = b"WEBPVP8L" + len(p).to_bytes(4, "little") + bytes(p) + b"\0" * (len(p) & 1)
    return b"RIFF" + len(body).to_bytes(4, "little") + body


@functools.lru_cache(maxsize=None)
def cases():
    r = np.random.default_rng(1)
    out = [(f"gradient_m{m}", _enc(_gradient(r, 37, 53), method=m), "dev") for m in (0, 3, 6)]
    out += [(f"colours{n}_{w}", _enc(_palette(r, w, h, n)), "dev") for n, w, h in ((4, 21, 17), (16, 19, 23), (200, 21, 40))]
    out.append(("colours2_9x5", _enc(_palette(r, 9, 5, 2)), "dev"))
    out.append(("flat_70x130", _enc(np.full((130, 70, 3), 77, np.uint8)), "dev"))
    g = r.integers(0, 256, (31, 29)).astype(np.uint8)
    out.append(("gray_noise", _enc(np.stack([g] * 3, -1)), "dev"))
    out.append(("rgba_exact", _enc(r.integers(0, 256, (23, 17, 4)).astype(np.uint8), exact=True), "dev"))
    out.append(("one_pixel", _enc(_gradient(r, 1, 1)), "dev"))
    out.append(("one_column", _enc(_gradient(r, 1, 33)), "dev"))
    icc = _enc(_gradient(r, 12, 9), icc_profile=b"not a real profile")
    out.append(("icc_vp8x", icc, "dev"))
    out.append(("wide_131x5", _enc(_gradient(r, 131, 5), method=4), "dev"))
    out.append(("rows65", _enc(_gradient(r, 20, 65), method=4), "dev"))
    out.append(("groups_128x96", _enc(_gradient(r, 128, 96), method=4), "dev"))
    tile = np.tile(r.integers(0, 256, (12, 24, 3)).astype(np.uint8), (3, 1, 1))  # matches 288 pixels back: no short code
    out += [(f"tiled_m{m}", _enc(tile, method=m), "dev") for m in (3, 4)]  # (method 3 gives it no transform at all)
    f = io.BytesIO()
    Image.fromarray(_gradient(r, 32, 24)).save(f, "WEBP", quality=80)
    out.append(("lossy", f.getvalue(), "declined"))
    out.append(("exif_vp8x", _enc(_gradient(r, 12, 9), exif=b"Exif\0\0II*\0\x08\0\0\0\0\0"), "declined"))
    anim = bytearray(icc)  # the VP8X file with its animation flag set
    assert anim[12:16] == b"VP8X"
    anim[20] |= 0x02
    out.append(("animation_flag", bytes(anim), "declined"))
    out.append(("riff_wave", b"RIFF\x04\0\0\0WAVE", "none"))
    return out


def damaged():
    """[(name, bytes)]: truncations and byte flips inside the VP8L payload of two of the files."""
    by = {c[0]: c[1] for c in cases()}
    out = []
    for name, cut in (("gradient_m3", 40), ("gradient_m3", 700), ("colours16_19", 9)):
        out.append((f"{name}_cut{cut}", riff(payload(by[name])[:-cut])))
    for name, at, x in (("gradient_m3", 6, 0x10), ("gradient_m3", 30, 0xFF), ("gradient_m3", 900, 0x01),
                        ("gradient_m0", 12, 0x80), ("colours16_19", 7, 0x04), ("flat_70x130", 8, 0x40),
                        ("gradient_m6", 200, 0x55), ("rows65", 1500, 0x08)):
        p = payload(by[name])
        p[at] ^= x
        out.append((f"{name}_flip{at}", riff(p)))
    return out

"""Lossy WebP files for tests/test_webp_lossy_cpu.py and tests/test_gpu_webp_lossy.py.

``cases()`` -> [(name, bytes, expect)] with expect "dev" (a context with ``webp_forms`` on decodes
it) or "declined" (Pillow decides it).  Encoded by Pillow at test time at the smallest shapes at
which each stage can go wrong (one pixel, one macroblock, crops on both axes with odd sides, a
4 x 6 macroblock frame with a full x + 2 y wavefront), plus the files of tests/golden/webp_lossy
(cwebp options Pillow's encoder does not have; README.md there lists the command lines)."""

import functools
import io
from pathlib import Path

import numpy as np
from PIL import Image

GOLDEN = Path(__file__).parent / "golden" / "webp_lossy"
SIZES = ((1, 1), (16, 16), (17, 33), (33, 17), (50, 83))


def _enc(a: np.ndarray, **kw) -> bytes:
    f = io.BytesIO()
    Image.fromarray(a).save(f, "WEBP", **kw)
    return f.getvalue()


def _noise(r, w, h):
    return r.integers(0, 256, (h, w, 3)).astype(np.uint8)


def mixed(r, w, h):
    """A gradient with a noise patch: 16x16-mode macroblocks beside 4x4-mode ones."""
    y, x = np.mgrid[:h, :w]
    a = (np.stack([x * 4 + y, y * 3, 255 - x * 2 - y], -1) % 256).astype(np.uint8)
    a[h // 3: 2 * (h // 3), w // 4: w // 4 + w // 2] = _noise(r, w // 2, h // 3)
    return a


def payload(b: bytes) -> bytearray:
    """The VP8 payload of a bare RIFF / WEBP / VP8 file."""
    assert b[12:16] == b"VP8 "
    return bytearray(b[20:20 + int.from_bytes(b[16:20], "little")])


def riff(p: bytes) -> bytes:
    """The bare file around a VP8 payload."""
    body = b"WEBPVP8 " + len(p).to_bytes(4, "little") + bytes(p) + b"\0" * (len(p) & 1)
    return b"RIFF" + len(body).to_bytes(4, "little") + body


@functools.lru_cache(maxsize=None)
def cases():
    r = np.random.default_rng(2)
    out = [(f"noise_q100_{w}x{h}", _enc(_noise(r, w, h), quality=100), "dev") for w, h in SIZES]
    out += [(f"noise_q5_{w}x{h}", _enc(_noise(r, w, h), quality=5), "dev") for w, h in SIZES[2:]]
    out += [(f"flat_{w}x{h}", _enc(np.full((h, w, 3), (90, 160, 40), np.uint8), quality=75), "dev") for w, h in SIZES[1:]]
    out += [(f"mixed_m{m}", _enc(mixed(r, 50, 83), quality=60, method=m), "dev") for m in (0, 4, 6)]
    half = np.full((83, 50, 3), 128, np.uint8)  # (methods below 3 code the skip flag, the token loop of the others does not)
    half[:20, :20] = _noise(r, 20, 20)
    out.append(("half_flat_m2", _enc(half, quality=75, method=2), "dev"))
    out.append(("mixed_q90_33x17", _enc(mixed(r, 33, 17), quality=90, method=4), "dev"))
    out.append(("icc_vp8x", _enc(mixed(r, 17, 33), quality=75, icc_profile=b"not a real profile"), "dev"))
    out += [(p.stem, p.read_bytes(), "dev") for p in sorted(GOLDEN.glob("*.webp"))]
    out.append(("alpha", _enc(r.integers(0, 256, (17, 33, 4)).astype(np.uint8), quality=75), "declined"))
    out.append(("exif_vp8x", _enc(mixed(r, 17, 33), quality=75, exif=b"Exif\0\0II*\0\x08\0\0\0\0\0"), "declined"))
    return out


def damaged():
    """[(name, bytes)]: byte flips inside the first partition and inside the token partition of two
    files, and the same files with the chunk cut short (sizes rewritten: the walk still verifies them)."""
    by = {c[0]: c[1] for c in cases()}
    out = []
    for name in ("mixed_m4", "noise_q100_17x33"):
        p = payload(by[name])
        first = int.from_bytes(p[:3], "little") >> 5
        for at, x in ((12, 0x40), (10 + first // 2, 0x08), (10 + first - 2, 0xFF), (10 + first + 5, 0x10),
                      (10 + first + (len(p) - 10 - first) // 2, 0x81), (len(p) - 3, 0x55)):
            q = bytearray(p)
            q[at] ^= x
            out.append((f"{name}_flip{at}", riff(q)))
        for cut in (4, (len(p) - 10 - first) // 2):
            out.append((f"{name}_cut{cut}", riff(p[:-cut])))
    return out

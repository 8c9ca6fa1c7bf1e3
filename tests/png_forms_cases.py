"""PNG files of bit depths 1, 2, 4, 16 and Adam7 for tests/test_png_forms_cpu.py and
tests/test_gpu_png_forms.py: (name, file bytes, expectation).  "dev": a context with png_forms on
decodes it to Pillow's pixels; "raise": it takes the file and Pillow raises (a filter byte of 5);
"declined": not a form it takes.  The filter types 0..4 cycle over the rows of every pass.
"""

from __future__ import annotations

import functools
import zlib

import numpy as np

from tests import png_writer as pw

ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]
# every valid (colour type, depth) pair a context without the option declines: units 1, 2, 3... 8
FORMS = [(0, 1), (0, 2), (0, 4), (3, 1), (3, 2), (3, 4), (0, 16), (4, 16), (2, 16), (6, 16)]
LACED = [(0, 8), (2, 8), (3, 4), (0, 1), (6, 16)]
LACED_SIZES = [(1, 1), (2, 1), (1, 2), (3, 5), (5, 3), (4, 4), (8, 8), (9, 9), (13, 17),  # each empty-pass pattern
               (33, 70),   # 133 pass rows: bands straddle passes
               (5, 140),   # pass 7 has 70 rows: a carry inside a pass
               (130, 5)]   # the widest band


def rows_of(samples: np.ndarray, depth: int) -> np.ndarray:
    """H x W x C samples -> H x row-bytes uint8 as PNG packs them (MSB first, 16 bits big-endian)."""
    h, w, c = samples.shape
    if depth == 16:
        return samples.astype(">u2").view(np.uint8).reshape(h, w * c * 2)
    if depth == 8:
        return samples.astype(np.uint8).reshape(h, w * c)
    bits = (samples.reshape(h, w * c, 1) >> np.arange(depth - 1, -1, -1)) & 1
    return np.packbits(bits.reshape(h, w * c * depth).astype(np.uint8), axis=1)


def build(w: int, h: int, color: int, depth: int, lace: int = 0, seed: int = 0, types=(0, 1, 2, 3, 4),
          samples: np.ndarray | None = None) -> bytes:
    c = pw.CHANNELS[color]
    u = max(1, c * depth // 8)
    if samples is None:
        samples = np.random.default_rng(seed + 7 * w + 131 * h + depth).integers(0, 1 << depth, (h, w, c))
    raw = b""
    for p, (x0, y0, dx, dy) in enumerate(ADAM7 if lace else [(0, 0, 1, 1)]):
        sub = samples[y0::dy, x0::dx]
        if sub.size:
            rows = rows_of(sub, depth)
            raw += pw.filter_rows(rows.reshape(rows.shape[0], -1, u), tuple(np.roll(types, -p)))
    plte = bytes(range(40, 40 + 3 * min(1 << depth, 10))) if color == 3 else None  # (depth 4: entries 10..15 are missing)
    return pw.png(w, h, color, zlib.compress(raw), depth=depth, interlace=lace, plte=plte)


@functools.lru_cache(maxsize=None)
def cases() -> list:
    out = []
    for color, depth in FORMS:
        for w, h in [(w, h) for w in (1, 3, 5, 7, 9, 70) for h in (1, 2, 65)]:  # row-end bits; the carry row across a band
            out.append((f"c{color}d{depth}_{w}x{h}", build(w, h, color, depth), "dev"))
        out.append((f"c{color}d{depth}_filter5", build(9, 4, color, depth, types=(1, 4, 5, 0)), "raise"))
    for color, depth in LACED:
        for w, h in LACED_SIZES:
            out.append((f"a7_c{color}d{depth}_{w}x{h}", build(w, h, color, depth, 1), "dev"))
        out.append((f"a7_c{color}d{depth}_filter5", build(9, 9, color, depth, 1, types=(2, 5)), "raise"))
    every = np.arange(65536).reshape(256, 256, 1)
    out.append(("gray16_every_value", build(256, 256, 0, 16, samples=every), "dev"))
    out.append(("rgb_depth4_invalid", build(5, 3, 2, 4), "declined"))
    return out

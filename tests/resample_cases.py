"""Hand-made crops that aim the resample kernels at their edges (shared by
test_resample_shapes_cpu.py, which checks that the cases are what they claim to be, and
test_gpu_resample_sweep.py, which runs them): every tile shape of k_hresize at its first and
last crop width, crop heights around the band and work-item sizes, degenerate crops, and
content that makes the bicubic sums overshoot both ends of the 8-bit clip.

A case is (rgb image [H, W, 3] u8, [ViewParams ...]); pack_cases lays the cases out as batch
slots of ``nv`` views each (a case with more records takes several slots of its image).
"""

from __future__ import annotations

import numpy as np

from oracle.cpu_ref import ViewParams
from tests.helpers import hresize_shape_table, hresize_tile, resample_sweep_widths, saturating_rgb

MAX_VIEWS = 32  # kMaxViews: views per image of one dino_augment call


def _plain(S, top, left, h, w, k):
    """Resize only (jitter, gray, blur, solarize off); every other record flipped."""
    return ViewParams(out_size=S, crop_top=top, crop_left=left, crop_h=h, crop_w=w, flip=bool((k >> 1) & 1))


def sweep_image_size(lib, S: int) -> tuple[int, int]:
    """(W, H) of the width sweep's image: as wide as the largest listed width; about 140 rows
    (8 bands of 16 rows + 1, and some room to move the crop), S rows where that is more."""
    return max(resample_sweep_widths(lib, S)), max(140, S)


def extra_widths(S: int) -> list[int]:
    """Widths inside the first shape that the boundary lists leave out: 2 and 3 px and wider
    upscales (hard edges upscaled overshoot most), S +- 1, and a 1.5 x downscale."""
    return [2, 3, S // 4 + 1, S // 2 + 1, S - 1, S + 1, S + S // 2 + 1]


def width_sweep_records(lib, S: int, W: int, H: int) -> list[ViewParams]:
    """One record per listed crop width, then one per extra width.  crop_left % 4 cycles through 0..3 (the staging
    loads' byte alignment), alternately near the image's left and right edge; crop_h cycles
    through {1, 7, R, R + 1, 8 R, 8 R + 1, S} for the width's own band height R (odd last row
    of a band, second work item, no vertical pass), at the bottom edge and at three other rows.
    The last record's crop ends at the image's last column and row."""
    recs = []
    widths = resample_sweep_widths(lib, S)
    for k, cw in enumerate(widths + extra_widths(S)):
        R = hresize_tile(lib, S, cw)[2] or 16  # (direct path: no bands)
        ch = min(H, [1, 7, R, R + 1, 8 * R, 8 * R + 1, S][k % 7])
        want = k % 4
        room = W - cw
        if room >= want:
            left = want if (k // 4) & 1 else room - ((room - want) % 4)
        else:
            left = room
        top = min(H - ch, [H - ch, 0, H // 4, H // 2][(k // 2) % 4])  # (the saturating image's four bands)
        recs.append(_plain(S, top, left, ch, cw, k))
    mid = widths[len(widths) // 2]
    R = hresize_tile(lib, S, mid)[2] or 16
    recs.append(_plain(S, H - (R + 1), W - mid, R + 1, mid, 0))
    return recs


def height_sweep_case(S: int, rng):
    """crop_w = S (no horizontal pass) and S + 1, crop_h over rows fewer / more than S."""
    hs = [1, 2, 3, S - 1, S + 1, 2 * S, 2 * S + 1] + ([1000, 4001] if S <= 224 else [])
    W, H = S + 4, max(hs)
    img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    recs = []
    for k, (cw, ch) in enumerate((cw, ch) for cw in (S, S + 1) for ch in hs):
        recs.append(_plain(S, (H - ch) if k & 1 else 0, min(k % 4, W - cw), ch, cw, k))
    return img, recs


def degenerate_cases(S: int, rng):
    """1 x 1, 1 x 5, 5 x 1, 2 x 2 and 3 x 2 crops (w x h), on noise and on 0/255 bits, and
    whole 1 x 1 and 2 x 3 images: one- to three-tap coefficient rows."""
    cases = []
    for img in (rng.integers(0, 256, size=(7, 9, 3), dtype=np.uint8),
                rng.integers(0, 2, size=(7, 9, 3), dtype=np.uint8) * 255):
        recs = []
        for k, (cw, ch) in enumerate([(1, 1), (1, 5), (5, 1), (2, 2), (3, 2)]):
            recs.append(_plain(S, (7 - ch) if k & 1 else k % 2, (9 - cw) if k & 2 else k % 3, ch, cw, k))
        cases.append((img, recs))
    cases.append((rng.integers(0, 256, size=(1, 1, 3), dtype=np.uint8), [_plain(S, 0, 0, 1, 1, 0)]))
    img = rng.integers(0, 256, size=(3, 2, 3), dtype=np.uint8)  # 2 wide, 3 high
    cases.append((img, [_plain(S, 0, 0, 3, 2, 0), _plain(S, 2, 1, 1, 1, 2), _plain(S, 1, 0, 2, 2, 1),
                        _plain(S, 0, 1, 3, 1, 3)]))
    return cases


def constant_widths(lib, S: int) -> list[int]:
    """Three widths for the all-255 / all-0 images: an upscale, a small downscale, and the
    first sliced shape's first width (for S > 256 every width is sliced: a wider one)."""
    table, _ = hresize_shape_table(lib, S)
    sliced = next(first for first, _, sw, R in table if R and sw < S and first > S + 3)
    return [S // 3 + 1, S + 3, sliced]


def constant_cases(lib, S: int):
    ws = constant_widths(lib, S)
    W, H = max(ws), 24
    cases = []
    for val in (255, 0):
        img = np.full((H, W, 3), val, np.uint8)
        cases.append((img, [_plain(S, 0 if k else H - 5, (W - cw) if k & 1 else 0, [5, 24, 17][k], cw, k)
                            for k, cw in enumerate(ws)]))
    return cases


def resize_cases(lib, S: int):
    """Every resize-only case of view size S.  The saturating width sweep comes last, so
    that the batch's last image holds the crop that ends at its last column and row."""
    rng = np.random.default_rng(1000 + S)
    W, H = sweep_image_size(lib, S)
    recs = width_sweep_records(lib, S, W, H)
    noise = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    cases = [height_sweep_case(S, rng), *degenerate_cases(S, rng), *constant_cases(lib, S),
             (noise, recs), (saturating_rgb(W, H, rng), recs)]
    return cases


def pack_cases(cases, nv: int = MAX_VIEWS):
    """-> (images, records [B][nv], keep [B][nv]): batch slots of nv views; a slot's spare
    views repeat its last record (keep False: rendered, not compared again)."""
    images, records, keep = [], [], []
    for img, recs in cases:
        for s in range(0, len(recs), nv):
            part = recs[s:s + nv]
            images.append(img)
            records.append(part + [part[-1]] * (nv - len(part)))
            keep.append([True] * len(part) + [False] * (nv - len(part)))
    return images, records, keep

"""CPU: every 8-bit resample coefficient fits the 24-bit signed multiply of the vertical
pass (csrc/resize.hpp tap_mad: |k| < 2^23).  Pillow's coefficient computation
(precompute_coeffs + normalize_coeffs_8bpc, as resample_coeffs_one states it) is restated
here in float64 and swept over input and output sizes and output positions: every position
of the small sizes, where taps are clipped at both image edges at once, and the edge and
some interior positions of the large ones, up to a 65535-pixel side and the 1024 view limit.
The restatement itself is tied to the kernels' own code through the host emulator."""

from __future__ import annotations

import numpy as np

from dataloader_amd.params import VIEW_PARAMS_DTYPE
from tests.helpers import emu_resized_crop

PRECISION_BITS = 22
LIMIT = 1 << 23


def _bicubic(x):
    x = np.abs(x)
    return np.where(x < 1.0, ((1.5 * x - 2.5) * x) * x + 1.0,
                    np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5, 0.0))


def coeffs(in_size: int, out_size: int, xx: np.ndarray):
    """(xmin, count, taps[len(xx), ksize]) of the output positions xx, in the operation order
    of resample_coeffs_one (float64 throughout, weights summed left to right)."""
    scale = float(np.float32(in_size)) / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    t = np.arange(ksize)
    w = _bicubic((t[None, :] + xmin[:, None] - center[:, None] + 0.5) * (1.0 / fs))
    w = np.where(t[None, :] < xmax[:, None], w, 0.0)
    ww = np.zeros(len(xx))
    for j in range(ksize):  # (np.sum adds pairwise: not Pillow's order)
        ww = ww + w[:, j]
    wn = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.where(wn < 0, -0.5 + wn * (1 << PRECISION_BITS), 0.5 + wn * (1 << PRECISION_BITS)).astype(np.int64)
    return xmin, xmax, k


def _positions(out_size: int, every: bool) -> np.ndarray:
    if every or out_size <= 64:
        return np.arange(out_size)
    mid = np.linspace(16, out_size - 17, 32).astype(np.int64)
    return np.unique(np.concatenate([np.arange(16), mid, np.arange(out_size - 16, out_size)]))


def test_restatement_matches_the_kernels_code(emu):
    """Rows and columns resampled with coeffs() equal the emulator's resized crop (the same
    resample_coeffs_one and the same sums as the kernels), upscaled and downscaled."""
    rng = np.random.default_rng(11)
    for (W, H, S) in [(37, 5, 16), (9, 90, 32), (200, 131, 30), (3, 2, 12)]:
        rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        rec = np.zeros((), VIEW_PARAMS_DTYPE)
        rec["out_size"], rec["crop_w"], rec["crop_h"] = S, W, H
        got = emu_resized_crop(emu, rgb, rec)

        def one_pass(src, n_in):  # along axis 1
            xmin, cnt, k = coeffs(n_in, S, np.arange(S))
            out = np.empty((src.shape[0], S, 3), np.uint8)
            for x in range(S):
                acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(
                    src[:, xmin[x]:xmin[x] + cnt[x]].astype(np.int64), k[x, :cnt[x]], axes=([1], [0]))
                out[:, x] = np.clip(acc >> PRECISION_BITS, 0, 255)
            return out

        tmp = one_pass(rgb, W)
        ref = one_pass(tmp.transpose(1, 0, 2), H).transpose(1, 0, 2)
        assert np.array_equal(ref, got), (W, H, S)


def test_every_tap_fits_24_bits():
    """|k| < 2^23 over the sweep; prints the largest magnitude and where it was found."""
    outs_all = list(range(1, 41)) + [96, 128, 224, 518, 1024]
    pairs = []
    for i in range(1, 321):  # small inputs: every position, every small output and the view sizes
        pairs += [(i, o, True) for o in outs_all if o <= 40 or i <= 64 or i % 16 == 1]
    big_in = [321, 480, 500, 640, 767, 1023, 1024, 1025, 1600, 2047, 4001, 4096, 9999, 16384, 32768, 65535]
    for i in big_in:  # large inputs: edges and a spread of interior phases
        pairs += [(i, o, False) for o in (1, 2, 3, 7, 30, 32, 96, 224, 518, 1023, 1024)]
    # scales just off 1 and just off small integers, where a tap sits at (or a hair off) weight 1
    for o in (30, 32, 96, 224, 1024):
        pairs += [(o + d, o, False) for d in (-3, -2, -1, 1, 2, 3) if o + d > 0]
        pairs += [(m * o + d, o, False) for m in (2, 3, 4) for d in (-1, 0, 1)]
    worst = (0, None)
    for i, o, every in pairs:
        xx = _positions(o, every)
        _, _, k = coeffs(i, o, xx)
        m = int(np.abs(k).max())
        if m > worst[0]:
            r = int(np.abs(k).max(axis=1).argmax())
            worst = (m, (i, o, int(xx[r])))
    m, at = worst
    print(f"largest |k| = {m} = {m / (1 << PRECISION_BITS):.4f} x 2^22 at (in, out, position) = {at}; "
          f"{len(pairs)} size pairs")
    assert m >= 1 << PRECISION_BITS  # (the sweep reaches weight 1.0)
    assert m < LIMIT, worst

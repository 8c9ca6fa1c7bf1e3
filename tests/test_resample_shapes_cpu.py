"""The resample sweep aims where it claims to (CPU): the crop-width lists of
tests/helpers.py, built from the kernel's own tile-shape functions (hresize_tile.hpp through
the emulator), hold the first and last width of every (sw, R) shape of k_hresize; the
hand-made records of tests/resample_cases.py stay inside their images; and the saturating
content really drives Pillow's bicubic sums past both ends of the 8-bit clip, so the
bit-exact GPU comparison cannot pass on a reference that never clips."""

from __future__ import annotations

import numpy as np
import pytest

from tests import resample_cases as rc
from tests.helpers import (SWEEP_DIRECT_SIZES, SWEEP_MAX_WIDTH, SWEEP_SIZES, hresize_shape_table, hresize_tile,
                           pillow_bicubic_row_unclipped, resample_sweep_widths, saturating_rgb)


def _walk(emu, S, stop):
    """[(cw, sw, R)] for cw = 1 .. stop (crop_w == S has no horizontal pass), straight from
    the emulator, not through the table builder."""
    return [(cw, *[hresize_tile(emu, S, cw)[i] for i in (0, 2)]) for cw in range(1, stop + 1) if cw != S]


@pytest.mark.parametrize("S", SWEEP_SIZES)
def test_sweep_widths_cover_every_tile_shape(emu, S):
    ws = resample_sweep_widths(emu, S)
    assert ws == sorted(set(ws)) and ws[0] == 1 and S not in ws
    table, first_ng = hresize_shape_table(emu, S)
    stop = SWEEP_MAX_WIDTH if S > 256 else table[-1][0]
    walk = _walk(emu, S, stop)
    if S <= 256:
        assert walk[-1][2] == 0 and all(R > 0 for _, _, R in walk[:-1])  # ends at the first direct width
    runs = []  # [first, last, sw, R] of each run of equal (sw, R)
    for cw, sw, R in walk:
        if runs and runs[-1][2:] == [sw, R]:
            runs[-1][1] = cw
        else:
            runs.append([cw, cw, sw, R])
    assert len(runs) == len(table) and len({(sw, R) for _, _, sw, R in runs}) == len(runs)  # no shape comes back
    for i, (first, last, sw, R) in enumerate(runs):
        if R == 0 and S not in SWEEP_DIRECT_SIZES:
            continue  # (the direct path is swept at three view sizes)
        # every shape by its first width, and by its predecessor's last
        assert first in ws, f"S={S}: shape {(sw, R)} from width {first} is not in the sweep"
        assert i == 0 or runs[i - 1][1] in ws, f"S={S}: width {runs[i - 1][1]}, the last before shape {(sw, R)}"
    ng_widths = [cw for cw in ws if hresize_tile(emu, S, cw)[5] > 8 and hresize_tile(emu, S, cw)[2] > 0]
    if S <= 256:  # the generic tap-group loop (more than 8 groups: crops over 7.5 S wide)
        assert first_ng == ng_widths[0] and hresize_tile(emu, S, first_ng - 1)[5] == 8
        assert first_ng == int(7.5 * S) + 1
    else:
        assert first_ng is None and not ng_widths and SWEEP_MAX_WIDTH < 7.5 * S


def test_sweep_tables_match_the_hand_computed_ones(emu):
    """Cross-check against a restatement of hresize_tile in Python (the tables quoted when
    the sweep was proposed): the first width of every shape at S = 224, the landmarks at 96."""
    t224, _ = hresize_shape_table(emu, 224)
    assert [t[0] for t in t224] == [1, 221, 241, 297, 337, 445, 468, 508, 546, 561, 609, 690, 776, 863, 977, 1009,
                                    1128, 1317, 1457, 1559, 1887, 2045, 2353, 2806, 2892, 3606, 3706, 4593, 4803,
                                    5251, 6385, 6497, 7729, 8513, 10529]
    t96, _ = hresize_shape_table(emu, 96)
    assert len(t96) == 24
    assert next(t[0] for t in t96 if t[3] < 16) == 317        # the bands shrink
    assert next(t[0] for t in t96 if t[2] < 96) == 509        # the view is sliced
    assert t96[-1][0] == 4513 and t96[-1][3] == 0             # direct


def test_sweep_reaches_sliced_direct_and_wide_slices(emu):
    for S in (224, 96):
        tiles = [hresize_tile(emu, S, cw) for cw in resample_sweep_widths(emu, S)]
        assert any(0 < t[0] < S for t in tiles) and any(t[2] == 0 for t in tiles)
    for S in (518, 1024):
        # slices wider than the 256-lane workgroup (a lane steps by whole slices: dq = 0) from
        # width 1 through every upscale; wider crops bring the slice down across 256 (the
        # listed widths go on to SWEEP_MAX_WIDTH, so both sides of that boundary are swept)
        ws = resample_sweep_widths(emu, S)
        assert max(ws) == SWEEP_MAX_WIDTH
        sw = {cw: hresize_tile(emu, S, cw)[0] for cw in ws}
        assert sw[1] == 400 and all(v > 256 for cw, v in sw.items() if cw <= S)
        assert all(0 < v < S for v in sw.values()) and S % sw[1] != 0  # always sliced, last slice partial
        assert {256, 264} <= set(sw.values()) and min(sw.values()) < 256


@pytest.mark.parametrize("S", SWEEP_SIZES)
def test_sweep_records_are_valid_and_aimed(emu, S):
    cases = rc.resize_cases(emu, S)
    for img, recs in cases:
        H, W, _ = img.shape
        for p in recs:
            assert p.out_size == S and p.crop_w >= 1 and p.crop_h >= 1
            assert 0 <= p.crop_left and p.crop_left + p.crop_w <= W and 0 <= p.crop_top and p.crop_top + p.crop_h <= H
            assert not (p.jitter or p.gray or p.blur or p.solarize)
    flips = [p.flip for _, recs in cases for p in recs]
    assert 0.4 <= sum(flips) / len(flips) <= 0.6
    # the width sweep: one record per listed width, on noise and on the saturating image
    (noise, recs), (sat, recs2) = cases[-2:]
    assert recs is recs2 and noise.shape == sat.shape
    ws = resample_sweep_widths(emu, S)
    assert [p.crop_w for p in recs[:-1]] == ws + rc.extra_widths(S)
    assert {p.crop_left % 4 for p in recs} == {0, 1, 2, 3}
    H, W, _ = noise.shape
    band = {hresize_tile(emu, S, p.crop_w)[2] for p in recs}
    for R in band - {0}:  # every band height in the list meets an odd last row and a second work item
        hs = {p.crop_h for p in recs if hresize_tile(emu, S, p.crop_w)[2] == R}
        assert hs & {R + 1, 8 * R + 1, 1, 7}, (S, R, hs)
    assert {1, 7, min(H, S)} <= {p.crop_h for p in recs}
    assert any(p.crop_h == 8 * hresize_tile(emu, S, p.crop_w)[2] + 1 for p in recs)
    assert any(hresize_tile(emu, S, p.crop_w, p.crop_h)[4] > -(-S // hresize_tile(emu, S, p.crop_w)[0]) for p in recs
               if hresize_tile(emu, S, p.crop_w)[2])  # more work items than slices: a second band group
    # the batch's last view ends at the last column and row of the last image
    images, records, keep = rc.pack_cases(cases)
    last = records[-1][-1]
    assert images[-1] is sat and last.crop_left + last.crop_w == W and last.crop_top + last.crop_h == H
    assert all(len(r) == rc.MAX_VIEWS for r in records) and len(images) == len(records) == len(keep)
    # height sweep and degenerate crops
    himg, hrecs = cases[0]
    want = {1, 2, 3, S - 1, S + 1, 2 * S, 2 * S + 1} | ({1000, 4001} if S <= 224 else set())
    for cw in (S, S + 1):
        assert {p.crop_h for p in hrecs if p.crop_w == cw} == want
    small = {(p.crop_w, p.crop_h) for img, recs in cases[1:5] for p in recs}
    assert {(1, 1), (1, 5), (5, 1), (2, 2), (3, 2)} <= small
    assert {img.shape[:2] for img, _ in cases[1:5]} >= {(1, 1), (3, 2)}
    # constant images: three widths each, an upscale, a downscale and a sliced one
    for (img, recs), val in zip(cases[5:7], (255, 0)):
        assert (img == val).all() and len(recs) == 3
        tiles = [hresize_tile(emu, S, p.crop_w) for p in recs]
        assert recs[0].crop_w < S < recs[1].crop_w and 0 < tiles[2][0] < S


@pytest.mark.parametrize("S", SWEEP_SIZES)
def test_saturating_content_clips_in_pillow(emu, S):
    """Pillow's own coefficient formula in float64, without the clip, on rows of the step-edge
    bands of the sweep's saturating image, for an upscaling and a downscaling width of the
    sweep: the sums leave [0, 255] by more than a level on both sides."""
    W, H = rc.sweep_image_size(emu, S)
    sat = saturating_rgb(W, H, np.random.default_rng(1000 + S))
    up, down = S // 2 + 1, S + S // 2 + 1
    assert {up, down} <= set(rc.extra_widths(S))
    for cw in (up, down):
        lo, hi = np.inf, -np.inf
        for y in (0, H // 4, H // 2):  # bits, checkerboard, stripes
            out = pillow_bicubic_row_unclipped(sat[y, W - cw:, 0], S)
            lo, hi = min(lo, out.min()), max(hi, out.max())
        assert lo < -1.0 and hi > 256.0, (S, cw, lo, hi)
    # and the real thing clips them: Pillow's result on the same rows is 0 / 255 there
    from PIL import Image
    row = sat[0:1, W - up:]
    got = np.asarray(Image.fromarray(row, "RGB").resize((S, 1), Image.BICUBIC))[0, :, 0]
    ref = pillow_bicubic_row_unclipped(row[0, :, 0], S)
    assert (got[ref < -1.0] == 0).all() and (got[ref > 256.0] == 255).all()
    inside = (ref > 0.5) & (ref < 254.5)
    assert np.abs(got[inside] - ref[inside]).max() <= 0.51

"""CPU: the two scratch layouts of the augment workspace (csrc/plan.hpp view_scratch and
dec_scratch, through the emulator) and the Python bound of the decode-only one.

Every region sits exactly where the documented layout puts it, in the documented order,
none overlaps the next, the last ends at `total`, and `total` is the expression the planners
used before the layout had one owner, written out here.  Every region starts on 16 bytes,
with one exception, vt: it follows ht[S][kh] (a view) or vb[oh][2] (decode-only) without
padding, so all it can promise is an int32's 4 bytes.  With S = 30 and kh = 5 (Pillow's tap
counts are odd) a view's vt starts 16 * 30 + 4 * 30 * 5 = 1080 bytes into the block, 8 mod 16;
padding it would change `total`, which this layout must not.  (vb of a view at hb + 8 * S
and ht of a decode-only image at 8 * ow are on 16 bytes when S and ow are even, as all sizes
here are; the kernels need no more of them than 4 either.)"""

from __future__ import annotations

import itertools

import pytest

from dataloader_amd.pipeline import resize_scratch_bound
from tests.helpers import (DEC_SCRATCH_FIELDS, VIEW_SCRATCH_FIELDS, dec_scratch, dec_scratch_total,
                           resample_sweep_widths, view_scratch, view_vcoefs)


def align16(x: int) -> int:
    return (x + 15) & ~15


def _check_regions(L: dict[str, int], order, sizes: dict[str, int], align: dict[str, int]):
    assert [L[k] for k in order] == sorted(L[k] for k in order), L  # the documented order
    for k, nxt in zip(order, order[1:]):
        assert L[k] % align[k] == 0, (k, L)
        assert L[k] + sizes[k] <= L[nxt], (k, L)  # no overlap
    assert align16(L[order[-2]] + sizes[order[-2]]) == L["total"], L  # the last region ends at total (rounded)


@pytest.mark.parametrize("S", [30, 96, 224, 518])
def test_view_layout(emu, S):
    assert S % 2 == 0
    align = {"htmp": 16, "hb": 16, "vb": 16, "ht": 16, "vt": 4, "hx": 16, "hg": 16}
    n = 0
    for c in resample_sweep_widths(emu, S):  # the crop side, as width and as height
        k = emu.emu_resample_ksize(c, S)
        for kh, kv in itertools.product((0, k), (0, k)):
            L = view_scratch(emu, S, c, kh, kv)
            sizes = {"htmp": c * S * 3 if kh else 0, "hb": 8 * S, "vb": 8 * S, "ht": 4 * S * kh, "vt": 4 * S * kv,
                     "hx": 16 * S if kh else 0, "hg": 16 * S * ((kh + 3) // 4)}
            _check_regions(L, VIEW_SCRATCH_FIELDS, sizes, align)
            assert L["htmp"] == 0 and L["hb"] == (align16(c * S * 3) if kh else 0)
            assert (L["vb"], L["ht"], L["vt"]) == (L["hb"] + 8 * S, L["hb"] + 16 * S, L["hb"] + 16 * S + 4 * S * kh)
            assert L["hx"] == L["hb"] + align16(4 * S * (4 + kh + kv)) and L["hg"] == L["hx"] + sizes["hx"]
            old = ((align16(c * S * 3) if kh else 0) + align16(S * (4 + kh + kv) * 4)
                   + (S * 16 * (1 + (kh + 3) // 4) if kh else 0))
            assert L["total"] == old, (S, c, kh, kv)
            assert view_vcoefs(emu, S, kh, kv) == (L["vb"] - L["hb"], L["vt"] - L["hb"])  # vert_apply's spelling
            if kh == 0:  # no horizontal pass: no rows and no dot4 tables
                assert L["hb"] == L["htmp"] and L["hx"] == L["hg"] == L["total"], L
            n += 1
    assert n >= 16


DEC_SHAPES = [(200, 255, 66, 85), (24, 9, 96, 36), (96, 255, 96, 85),  # test_decode_only_extremes_bit_exact
              (66, 255, 66, 85), (200, 85, 66, 85)]                      # kh == 0 (the third too), kv == 0


@pytest.mark.parametrize("w,h,ow,oh", DEC_SHAPES)
def test_decode_only_layout(emu, w, h, ow, oh):
    kh, kv = emu.emu_resample_ksize(w, ow), emu.emu_resample_ksize(h, oh)
    assert (kh == 0) == (w == ow) and (kv == 0) == (h == oh)
    L = dec_scratch(emu, ow, oh, h, kh, kv)
    sizes = {"hb": 8 * ow, "ht": 4 * ow * kh, "vb": 8 * oh, "vt": 4 * oh * kv, "htmp": h * ow * 3 if kh else 0}
    assert ow % 2 == 0
    _check_regions(L, DEC_SCRATCH_FIELDS, sizes, {"hb": 16, "ht": 16, "vb": 16, "vt": 4, "htmp": 16})
    assert (L["hb"], L["ht"]) == (0, 8 * ow)
    assert (L["vb"], L["vt"]) == (align16(4 * ow * (2 + kh)), align16(4 * ow * (2 + kh)) + 8 * oh)
    assert L["htmp"] == L["vb"] + align16(4 * oh * (2 + kv))
    old = align16(ow * (2 + kh) * 4) + align16(oh * (2 + kv) * 4) + (align16(h * ow * 3) if kh else 0)
    assert L["total"] == old
    if kh == 0:
        assert L["htmp"] == L["total"]
    assert L["total"] == dec_scratch_total(emu, w, h, ow, oh)


def test_python_bound_covers_dec_scratch(emu):
    """pipeline.resize_scratch_bound against the exact total over w, h in {9, 24, 200, 1600,
    8192} x ow, oh in {36, 85, 224}.  It is never below.  Above, 14 of the 225 shapes are not
    within 5 % + 256 bytes: on an axis that shrinks the bound counts two taps more than the
    kernels per output column or row (8 bytes each), plus 64 bytes of padding, which against
    a short image's total is a lot.  The largest relative excess is 200 x 9 to 224 x 36 (15 184
    against 13 328 bytes, 13.9 %), the largest absolute one 3 648 bytes (8192 x 8192 to
    224 x 224).  So the margin asserted is that argument's: at most 8 * (ow + oh) + 64 bytes
    above."""
    sides, outs = (9, 24, 200, 1600, 8192), (36, 85, 224)
    worst = (0, None)
    for w, h, ow, oh in itertools.product(sides, sides, outs, outs):
        exact = dec_scratch_total(emu, w, h, ow, oh)
        bound = resize_scratch_bound(w, h, ow, oh)
        worst = max(worst, (bound - exact, (w, h, ow, oh, exact, bound)))
        assert exact <= bound <= exact + 8 * (ow + oh) + 64, (w, h, ow, oh, exact, bound)
    print("largest excess:", worst)

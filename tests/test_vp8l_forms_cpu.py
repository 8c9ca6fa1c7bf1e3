"""VP8L stream forms libwebp's encoder never emits, on the CPU: the host model
(``dino_debug_webp_decode``, the text k_vp8l and k_vp8l_inv compile) and the probe against Pillow
over tests/vp8l_form_cases.py, bit for bit; every damaged file refused where Pillow raises; the
case list held to the writer's own record of what each file contains."""

import numpy as np
import pytest

from dataloader_amd import fallback
from dataloader_amd.tario import spans_of
from tests import vp8l_form_cases as fc
from tests import vp8l_writer as vw
from tests.png_cases import pillow_rgb
from tests.test_webp_cpu import model_decode

CASES = fc.cases()
BAD = fc.bad()
RECS = {c[0]: fc.record(c[0]) for c in CASES}
STREAMS = ("main", "predictor", "cross", "palette", "entropy")


def _probe(data):
    ptrs, lens, _keep = spans_of([data])
    form, ws = fallback.probe_webp(ptrs, lens)
    return form[0], int(ws[0])


@pytest.mark.parametrize("name,data,expect", CASES, ids=[c[0] for c in CASES])
def test_model_and_probe_match_pillow(name, data, expect):
    ref = pillow_rgb(data)
    assert ref is not None, "Pillow must decode every listed case"
    info, layout, rgb = model_decode(data)
    form, ws = _probe(data)
    assert form[0] == {"dev": 2, "declined": 1}[expect]
    if expect == "declined":
        assert info[3] == 0 and ws == 0
        return
    assert info[0] == 0 and tuple(form[1:]) == ref.shape[1::-1] and 0 <= ws - layout[1:5].sum() < 256 and ws == layout[0], (info, layout)
    assert np.array_equal(rgb, ref), int((rgb != ref).sum())


@pytest.mark.parametrize("name,data,expect", [c for c in CASES if c[2] == "dev"], ids=[c[0] for c in CASES if c[2] == "dev"])
def test_feature_words_match_the_writers_record(name, data, expect):
    """Transform mask, cache bits, group count, bundling bits and the kinds of distance code."""
    rec, feat = RECS[name], model_decode(data)[0][4:]
    codes = set().union(*(rec.get(s, {}).get("dist_code", set()) for s in STREAMS))
    bundle = [b + 1 for t, b in rec["tbits"] if t == vw.INDEX]
    want = [sum(1 << t for t in rec["transforms"]), rec["main"]["cache_bits"], rec["main"]["groups"], bundle[0] if bundle else 0,
            int(any(c <= 120 for c in codes)), int(any(c > 120 for c in codes))]
    assert feat.tolist() == want


@pytest.mark.parametrize("name,data", BAD, ids=[c[0] for c in BAD])
def test_damaged_file_is_refused_where_pillow_raises(name, data):
    """Form 1 (Pillow's, which raises) for an error in the prologue, a non-zero status for one in
    the codes or the pixels."""
    assert pillow_rgb(data) is None, "Pillow decodes it: the file belongs in cases()"
    info, _, _ = model_decode(data)
    form, _ = _probe(data)
    assert form[0] in (1, 2) and info[0] != 0, (form, info)
    assert (form[0] == 2) == (name in fc.BODY_ERRORS or "code" in name or "symbol" in name or "repeat" in name or "simple" in name), form


def _codes(rec, streams=STREAMS):
    return [(s, a, f) for s in streams for a, f in rec.get(s, {}).get("codes", [])]


def _any(pred):
    return [n for n, r in RECS.items() if pred(r)]


def _got(key, streams=("main",)):
    return set().union(*(r.get(s, {}).get(key, set()) for r in RECS.values() for s in streams))


def test_case_list_covers_every_form():
    """Every boundary the list is there for, read off the writer's record (the decoder's feature
    words are too coarse for it)."""
    P, X, G, I = vw.PREDICTOR, vw.CROSS, vw.GREEN, vw.INDEX
    orders = {tuple(r["transforms"]): n for n, r in RECS.items()}
    miss = []

    def need(what, ok):
        if not ok:
            miss.append(what)

    # transform orders
    for t in (P, X, G, I):
        need(f"transform {t} alone", (t,) in orders)
    for first in (G, P):
        for w in (300, 257):
            got = {b for n, r in RECS.items() if tuple(r["transforms"]) == (first, I) and f"_{w}x3" in n for t, b in r["tbits"] if t == I}
            need(f"{first} then index at width {w}: two bundlings", len(got) == 2)
        got = {b for r in RECS.values() if tuple(r["transforms"]) == (first, I) for t, b in r["tbits"] if t == I}
        need(f"{first} then index: bundling bits 3, 2, 1, 0", got == {0, 1, 2, 3})
        need(f"{first} then index at 5x2", any(tuple(r["transforms"]) == (first, I) and n.endswith("5x2") for n, r in RECS.items()))
    need("cross-colour as stage 0 on 7x5", RECS["only_cross_b9_7x5"]["transforms"] == [X])
    four = [o for o in orders if len(o) == 4]
    need("all four transforms in two orders that are not the encoder's", len(four) >= 2 and (I, G, P, X) not in four and
         all(o[0] != I for o in four))
    # predictor
    for n in ("predictor_modes_16x16", "predictor_modes_8x66"):
        need(f"{n}: all 16 modes", RECS[n]["predictor"]["greens"] == set(range(16)))
    need("predictor block bits 9", (P, 9) in RECS["predictor_b9_5x5"]["tbits"])
    need("predictor widths 2 and 3", {"predictor_w2", "predictor_w3"} <= set(RECS))
    need("modes 12 and 13 clip both ways, select takes both", RECS["predictor_clip_both_ways"]["clips"] >=
         {(12, "low"), (12, "high"), (13, "low"), (13, "high"), (11, "L"), (11, "T")})
    # cross-colour
    need("multipliers 0x80, 0x7F, 0xFF in all three positions", RECS["cross_multipliers_b2"]["multipliers"] ==
         {(p, m) for p in range(3) for m in (0x80, 0x7F, 0xFF)})
    need("cross-colour block bits 2 and 9", {(X, 2), (X, 9)} <= set().union(*(r["tbits"] for r in RECS.values())))
    # colour cache
    for bits, sym in ((1, 281), (11, 2327)):
        need(f"a {bits}-bit cache with symbol {sym}", bool(_any(lambda r: r["main"]["cache_bits"] == bits and sym in r["main"].get("cache_sym", ()))))
    for s in STREAMS[1:]:
        need(f"a cache in the {s} image", bool(_any(lambda r: r.get(s, {}).get("cache_bits") and r[s].get("cache_sym"))))
    need("200 literals on one slot, then a reference to it", max(_got("collide_run"), default=0) >= 200)
    need("a reference right after a back-reference longer than 64", max(_got("cache_after_copy"), default=0) > 64)
    need("a cache together with several groups", bool(_any(lambda r: r["main"]["cache_bits"] and r["main"]["groups_used"] > 1 and r["main"].get("cache_sym"))))
    # palette
    need("palette sizes", set().union(*(r.get("palette_sizes", set()) for r in RECS.values())) >= {1, 2, 3, 4, 5, 16, 17, 256})
    need("indices past the palette", sum("index_past_end" in n for n in RECS) >= 2)
    # codes
    all_codes = [(n, s, a, f) for n, r in RECS.items() for s, a, f in _codes(r)]
    for a in vw.ALPHABETS:
        need(f"a 15-bit code in {a}", any(x[2] == a and x[3]["maxlen"] == 15 for x in all_codes))
        need(f"a one-symbol code in {a}", any(x[2] == a and x[3]["nsyms"] == 1 for x in all_codes))
    need("pixels of 0 bits", bool(_any(lambda r: r["main"]["zero_bit_pixels"])))
    simple = [x[3] for x in all_codes if x[3]["simple"]]
    need("simple: two equal symbols", any(len(f["simple"][0]) == 2 and len(set(f["simple"][0])) == 1 for f in simple))
    need("simple: a 1-bit symbol", any(not f["simple"][1] for f in simple))
    need("simple: one of two outside the distance alphabet", any(f["n"] == 40 and len(f["simple"][0]) == 2 and f["nsyms"] == 1 and
                                                                 max(f["simple"][0]) >= 40 for f in simple))
    normal = [x[3] for x in all_codes if not x[3]["simple"]]
    need("max_symbol equal to the alphabet, in 16 bits", any(f["max_symbol"] == (f["n"], 7) for f in normal))
    need("max_symbol 2", any(f["max_symbol"] and f["max_symbol"][0] == 2 for f in normal))
    need("16 as the first symbol", any(f["cl_first"] == 16 for f in normal))
    for s in (16, 17, 18):
        need(f"{s} ending at the alphabet's end", any(s in f["cl_ends"] for f in normal))
    need("a code-length code of one symbol", any(f["cl_single"] and f["cl_count"] > 2 for f in normal))
    # back-references
    need("distance 1, length 4096, several groups", bool(_any(lambda r: 1 in r["main"].get("copy4096_dist", ()) and r["main"]["groups_used"] > 1)))
    need("overlapping copies", _got("overlap") >= {2, 3, 63, 64, 65})
    for n in ("short_codes_all_20wide", "short_codes_all_5wide"):
        need(f"{n}: all 120 codes", RECS[n]["main"]["dist_code"] == set(range(1, 121)))
    for w, n in ((5, 3), (2, 12)):
        need(f"short codes that clamp to 1 at width {w}", len(RECS[f"short_codes_all_{w}wide"]["main"].get("dist_clamped", ())) == n)
    need("10 extra length bits, 11 extra distance bits in 64x64", bool(_any(lambda r: 10 in r["main"].get("len_extra", ()) and 11 in r["main"].get("dist_extra", ()))))
    need("a match ending on the last pixel", bool(_got("copy_to_end")))
    for s in ("palette", "predictor", "entropy"):
        need(f"a back-reference in the {s} image", bool(_got("dist_code", (s,))))
    # groups
    need("prefix bits 2 and 9", {2, 9} <= {r["main"].get("prefix_bits") for r in RECS.values()})
    by = {c[0]: c[2] for c in CASES}
    need("exactly 256 groups on the device", any(r["main"]["groups"] == 256 and by[n] == "dev" for n, r in RECS.items()))
    need("257 groups and a sparse index declined", {r["main"]["groups"] for n, r in RECS.items() if by[n] == "declined"} == {257, 6})
    # input ring
    need("a payload over 3 KiB", RECS["ring_3k_payload"]["bytes"] > 3072)
    tails = {(r["nbits"] % 8, r["bytes"] % 2) for n, r in RECS.items() if n.startswith("tail_")}
    need("last bits in the final byte, with and without the pad byte", tails >= {(0, 0), (0, 1), (1, 0), (1, 1)})
    # bad(): one file per error rule
    bad = {n: fc.record(n) for n, _ in BAD}
    need("a transform given twice", bad["bad_transform_twice"]["transforms"] == [G, G])
    need("a back-reference before the first pixel and past the last one, main and sub-image",
         bad["bad_copy_before_first"]["main"]["copy_outside"] == {"before"} and bad["bad_copy_past_last"]["main"]["copy_outside"] == {"past"} and
         bad["bad_copy_before_first_in_sub_image"]["predictor"]["copy_outside"] == {"before"} and
         bad["bad_copy_past_last_in_sub_image"]["predictor"]["copy_outside"] == {"past"})
    need("a stream cut one bit short", bad["bad_cut_one_bit"]["nbits"] % 8 == 1)
    need("every error rule", {n for n, _ in BAD} >= {"bad_cache_bits_0", "bad_cache_bits_12", "bad_simple_all_outside", "bad_max_symbol_above_alphabet",
                                                    "bad_repeat_past_alphabet", "bad_code_length_code_empty", "bad_code_empty",
                                                    "bad_code_oversubscribed", "bad_code_incomplete_two_symbols"})
    assert not miss, miss


def test_ring_case_and_fillers_reach_every_alignment():
    """The batch order test_gpu_vp8l_forms.py uses puts the 3 KiB payload at every offset mod 16."""
    files = fc.ring_batch()
    data = {c[0]: c[1] for c in CASES}["ring_3k_payload"]
    at, seen = 0, set()
    for f in files:
        if f is data:
            seen.add((at + 20) % 16)
        at += len(f)
    assert seen == set(range(16))

"""The view sampler (csrc/sampler.hpp) on the host emulator: Philox stream, record equality with
an independent restatement, distributions against the oracle's draws, rates, op order, the
central-crop fallback and stream keying.

The parity tests replay each exported record through the oracle, so they cannot see a wrong
record; these tests pin the record itself.  Bounds (all computed here, none taken from a run):

* record equality with ``tests/sampler_ref.py``: exact, floats by their bits;
* two-sample Kolmogorov-Smirnov distance against ``cpu_ref.draw_params_like_cpubackend``:
  the critical value at alpha = 1e-6, sqrt(-ln(alpha / 2) / 2) * sqrt((n + m) / (n m));
* rates: |p^ - p| <= 5 sqrt(p (1 - p) / n), which is 0 for p = 0 and p = 1;
* op order: Pearson's chi-square over the 24 permutations below the alpha = 1e-6 quantile of
  chi2(23) (about 71);
* keying: changing one of seed / batch / sample / view changes (box, brightness) in >= 99 % of
  the pairs, and |Pearson r| <= 5 / sqrt(N) between neighbouring streams and between the row
  and the column position inside a record.
The seeds are fixed, so every figure is deterministic; ``pytest -s`` prints them.
"""

from __future__ import annotations

import ctypes
import itertools
import math
import random
from statistics import NormalDist

import numpy as np
import pytest
import torch

from dataloader_amd.config import DINOAugConfig, EvalAugSpec, LeJEPAAugSpec, recipe_aug_config
from dataloader_amd.params import VIEW_PARAMS_DTYPE, make_aug_config
from oracle import cpu_ref
from tests.helpers import P
from tests.sampler_ref import assert_records_equal, philox4x32_10, sample_view_ref

ALPHA = 1e-6
N_DIST = 4000
DIST_SIZES = [(500, 375), (300, 100), (64, 64)]


# ------------------------------------------------------------------------------ helpers
def emu_records(emu, cfg, seed, batch_index, sample, W, H, ok=1) -> np.ndarray:
    nv = cfg.n_global + cfg.n_local
    out = np.zeros(nv, VIEW_PARAMS_DTYPE)
    n = emu.emu_sample_params(ctypes.byref(cfg), ctypes.c_uint64(seed), ctypes.c_uint64(batch_index), int(sample),
                              int(W), int(H), int(ok), out.ctypes.data_as(P))
    assert n == nv
    return out


def ks_distance(a, b) -> float:
    a, b = np.sort(np.asarray(a, np.float64)), np.sort(np.asarray(b, np.float64))
    pts = np.concatenate([a, b])
    return float(np.abs(np.searchsorted(a, pts, "right") / a.size - np.searchsorted(b, pts, "right") / b.size).max())


def ks_bound(n: int, m: int) -> float:
    return math.sqrt(-math.log(ALPHA / 2) / 2) * math.sqrt((n + m) / (n * m))


def chi2_quantile(k: int, alpha: float) -> float:
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1 - alpha, k))
    except ImportError:  # Wilson-Hilferty
        z = NormalDist().inv_cdf(1 - alpha)
        return k * (1 - 2 / (9 * k) + z * math.sqrt(2 / (9 * k))) ** 3


def rate_ok(hits: int, n: int, p: float) -> tuple[bool, float]:
    dev = abs(hits / n - p)
    return dev <= 5 * math.sqrt(p * (1 - p) / n), dev


_POOLS: dict = {}


def emu_pool(emu, W, H, cfg=None, n=N_DIST, key="default") -> np.ndarray:
    """[n, views] records of n samples at W x H: seed fixed, 512 samples per batch index."""
    k = (W, H, n, key)
    if k not in _POOLS:
        c = cfg if cfg is not None else make_aug_config(DINOAugConfig(), 224, 96, 0)
        _POOLS[k] = np.stack([emu_records(emu, c, 0x5EED_0000_0000_0001 + W, s // 512, s % 512, W, H)
                              for s in range(n)])
    return _POOLS[k]


_ORACLE: dict = {}


def oracle_pool(W, H) -> list[list]:
    """[views][N_DIST] ViewParams in the reference's own draw order (one torch and one Python RNG)."""
    if (W, H) not in _ORACLE:
        gen, rnd, cfg = torch.Generator().manual_seed(1234 + W), random.Random(1234 + H), cpu_ref.AugCfg()
        specs = cpu_ref.view_table(cfg)
        per_view = [[] for _ in specs]
        for _ in range(N_DIST):
            for v, spec in enumerate(specs):
                per_view[v].append(cpu_ref.draw_params_like_cpubackend(W, H, spec, cfg, gen, rnd))
        _ORACLE[(W, H)] = per_view
    return _ORACLE[(W, H)]


def crop_stats(top, left, h, w, W, H) -> dict:
    top, left, h, w = (np.asarray(x, np.float64) for x in (top, left, h, w))
    return {"area": w * h / (W * H), "log_ratio": np.log(w / h), "left": left / np.maximum(W - w, 1),
            "top": top / np.maximum(H - h, 1)}


# ------------------------------------------------------------------------------ Philox
def test_philox_known_answers():
    """The three Random123 known-answer vectors of philox4x32_10 (kat_vectors)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, out in kat:
        assert tuple(philox4x32_10(ctr, key)) == out


# ------------------------------------------------------------------------------ record equality
def _tuples(n: int, rng_seed: int):
    """(seed, batch index, sample, W, H, ok): seeds with and without a high word, batch indices
    below and from 2^32, samples 0 and 511, W or H of 1, and undecoded images (1 x 1, ok = 0)."""
    rng = np.random.default_rng(rng_seed)
    out = []
    for k in range(n):
        seed = int(rng.integers(0, 1 << 63)) if k % 4 else int(rng.integers(0, 1 << 32))
        bi = [int(rng.integers(0, 1000)), (1 << 32) + int(rng.integers(0, 1000)), 1 << 32,
              int(rng.integers(1 << 32, 1 << 63))][k % 4 if k % 8 < 4 else 0]
        sample = [0, 511][k % 2] if k % 5 == 0 else int(rng.integers(0, 512))
        W, H, ok = int(rng.integers(1, 1201)), int(rng.integers(1, 901)), 1
        if k % 10 == 3:
            W = 1
        elif k % 10 == 7:
            H = 1
        elif k % 20 == 9:
            W = H = 1
            ok = 0
        out.append((seed, bi, sample, W, H, ok))
    return out


def _probs(**kw):
    return dict(blur_prob_global1=kw["p"], blur_prob_global2=kw["p"], blur_prob_local=kw["p"], solarize_prob=kw["p"],
                color_jitter_prob=kw["p"], grayscale_prob=kw["p"], flip_prob=kw["p"])


EVAL_SIZES = [(256, 300), (256, 256), (400, 256), (256, 1000), (300, 256), (500, 375), (375, 500), (1, 1), (1199, 899),
              (17, 9), (255, 256), (256, 255), (1000, 20), (20, 1000), (257, 256)]

CONFIGS = {
    "default": (lambda: make_aug_config(DINOAugConfig(), 224, 96, 0), 400),
    "all_p0": (lambda: make_aug_config(DINOAugConfig(**_probs(p=0.0)), 224, 96, 0), 100),
    "all_p1": (lambda: make_aug_config(DINOAugConfig(**_probs(p=1.0)), 224, 96, 0), 100),
    "brightness_1.5": (lambda: make_aug_config(DINOAugConfig(brightness=1.5), 224, 96, 0), 100),
    "hue_0": (lambda: make_aug_config(DINOAugConfig(hue=0.0), 224, 96, 0), 100),
    "global_scale_1_1": (lambda: make_aug_config(DINOAugConfig(global_crops_scale=(1.0, 1.0)), 224, 96, 0), 100),
    "no_local": (lambda: make_aug_config(DINOAugConfig(n_local_crops=0), 224, 96, 0), 100),
    "res_160_64": (lambda: make_aug_config(DINOAugConfig(), 160, 64, 1), 40),
    "lejepa": (lambda: make_aug_config(recipe_aug_config(LeJEPAAugSpec()), 224, 96, 0), 60),
    "eval_224": (lambda: make_aug_config(recipe_aug_config(EvalAugSpec()), 224, 224, 0), 30),
    "eval_96": (lambda: make_aug_config(recipe_aug_config(EvalAugSpec(crop_size=96)), 96, 96, 0), 30),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_records_equal_restatement(emu, name):
    """emu_sample_params == sample_view_ref, field for field, floats bitwise."""
    make, n = CONFIGS[name]
    cfg = make()
    nv = cfg.n_global + cfg.n_local
    tuples = _tuples(n, 77)
    if name.startswith("eval"):
        tuples += [(t[0], t[1], t[2], w, h, 1) for t, (w, h) in zip(tuples, EVAL_SIZES)]
    clamped = 0
    for seed, bi, sample, W, H, ok in tuples:
        got = emu_records(emu, cfg, seed, bi, sample, W, H, ok)
        want = np.stack([sample_view_ref(cfg, seed, bi, sample, v, W, H, ok) for v in range(nv)])
        assert_records_equal(got, want, f"{name} seed={seed:#x} batch={bi:#x} sample={sample} {W}x{H} ok={ok}")
        if not ok:
            assert (got["pad1"] == 1).all()
            if not name.startswith("eval"):
                for f, x in (("crop_top", 0), ("crop_left", 0), ("crop_h", 1), ("crop_w", 1)):
                    assert (got[f] == x).all(), (f, got[f])
        else:
            assert (got["pad1"] == 0).all()
        assert (got["pad0"] == 0).all()
        if name == "brightness_1.5":
            assert (got["brightness"] >= 0).all() and (got["brightness"] <= 2.5).all()
            clamped += int(((got["brightness"] < 0.25) & (got["jitter"] == 1)).sum())
        if name == "hue_0":
            assert (got["hue"] == 0).all()
        if name == "lejepa":
            assert (got["gray"] == 0).all() and (got["blur"] == 0).all() and (got["solarize"] == 0).all()
            assert (got["sigma"] == 1.0).all() and (got["ksize"] == 3).all()
            assert list(got["out_size"]) == [224, 96, 96, 96, 96]
            t = got[1:]
            assert (t["flip"] == 0).all() and (t["jitter"] == 0).all() and (t["hue"] == 0).all()
            assert (t["brightness"] == 1).all() and (t["contrast"] == 1).all() and (t["saturation"] == 1).all()
            assert (t["order"] == [0, 1, 2, 3]).all()
        if name.startswith("eval"):
            _check_eval(got[0], W if ok else 1, H if ok else 1, cfg.global_size)
    if name == "brightness_1.5":
        assert clamped > 0  # the range starts at 0, not at 1 - 1.5 clamped after the draw


def _check_eval(r, W, H, S):
    """Resize of the shorter side + centre crop as a box, a resample size and a window; an axis
    whose resampled length equals the source's is folded into the box (no window on it)."""
    nw, nh, left, top = cpu_ref.eval_geometry(W, H, S)
    for f in ("flip", "jitter", "gray", "blur", "solarize"):
        assert r[f] == 0
    want_x = (left, S, S, 0) if nw == W else (0, W, nw, left)
    want_y = (top, S, S, 0) if nh == H else (0, H, nh, top)
    assert (r["crop_left"], r["crop_w"], r["resize_w"], r["out_x"]) == want_x, (W, H, S)
    assert (r["crop_top"], r["crop_h"], r["resize_h"], r["out_y"]) == want_y, (W, H, S)


# ------------------------------------------------------------------------------ distributions
@pytest.mark.parametrize("W,H", DIST_SIZES)
def test_distributions_vs_oracle(emu, W, H):
    """KS distance of the crop statistics (global and local views apart), the four jitter factors
    over jittered records and sigma over blurred ones, against the reference's own draws."""
    got, ref = emu_pool(emu, W, H), oracle_pool(W, H)
    worst = {}
    for group, views in (("global", range(0, 2)), ("local", range(2, 10))):
        g = got[:, list(views)].reshape(-1)
        r = [p for v in views for p in ref[v]]
        a = crop_stats(g["crop_top"], g["crop_left"], g["crop_h"], g["crop_w"], W, H)
        b = crop_stats(*(np.array([getattr(p, f) for p in r]) for f in ("crop_top", "crop_left", "crop_h", "crop_w")),
                       W, H)
        bound = ks_bound(g.size, len(r))
        for k in a:
            worst[f"{group}.{k}"] = (ks_distance(a[k], b[k]), bound)
    flat, rflat = got.reshape(-1), [p for v in ref for p in v]
    for f in ("brightness", "contrast", "saturation", "hue"):
        a, b = flat[f][flat["jitter"] == 1], np.array([getattr(p, f) for p in rflat if p.jitter])
        worst[f] = (ks_distance(a, b), ks_bound(a.size, b.size))
    a, b = flat["sigma"][flat["blur"] == 1], np.array([p.sigma for p in rflat if p.blur])
    worst["sigma"] = (ks_distance(a, b), ks_bound(a.size, b.size))
    print(f"\nKS {W}x{H}: " + ", ".join(f"{k} {d:.4f}/{b:.4f}" for k, (d, b) in worst.items()))
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad
    if (W, H) == (300, 100):  # the size is here for the fallback: part of the global draws must reach it
        fb = np.mean([(p.crop_h, p.crop_w) == (100, 133) for p in ref[0]])
        assert 0.01 < fb < 0.99, fb


def _rate_checks(recs, cfg) -> dict:
    """{name: (hits, n, p)} for every configured probability, per view class."""
    n_s, nv = recs.shape
    out = {"flip": (int(recs["flip"].sum()), recs.size, cfg.flip_prob),
           "jitter": (int(recs["jitter"].sum()), recs.size, cfg.color_jitter_prob),
           "gray": (int(recs["gray"].sum()), recs.size, cfg.grayscale_prob),
           "blur.view0": (int(recs["blur"][:, 0].sum()), n_s, cfg.blur_prob_global1),
           "blur.view1": (int(recs["blur"][:, 1].sum()), n_s, cfg.blur_prob_global2),
           "blur.local": (int(recs["blur"][:, 2:].sum()), n_s * (nv - 2), cfg.blur_prob_local),
           "solarize.view1": (int(recs["solarize"][:, 1].sum()), n_s, cfg.solarize_prob)}
    return out


@pytest.mark.parametrize("key,p", [("default", None), ("all_p0", 0.0), ("all_p1", 1.0)])
def test_rates(emu, key, p):
    """Every probability of the config against its observed rate; p = 0 and p = 1 hold exactly."""
    acfg = DINOAugConfig() if p is None else DINOAugConfig(**_probs(p=p))
    n = N_DIST if p is None else 500
    recs = emu_pool(emu, 500, 375, make_aug_config(acfg, 224, 96, 0), n=n, key=key)
    worst = 0.0
    for name, (hits, cnt, prob) in _rate_checks(recs, acfg).items():
        ok, dev = rate_ok(hits, cnt, prob)
        assert ok, (name, hits, cnt, prob)
        worst = max(worst, dev * math.sqrt(cnt / (prob * (1 - prob))) if 0 < prob < 1 else 0.0)
    print(f"\nrates {key}: largest deviation {worst:.2f} sigma (bound 5)")
    others = np.delete(recs["solarize"], 1, axis=1)
    assert not others.any()  # solarize belongs to view 1 alone


def test_blur_ksize_and_ranges(emu):
    """ksize is the reference's function of sigma for every record; sigma and the four factors
    stay inside their configured ranges and come close to both ends."""
    for W, H in DIST_SIZES:
        r = emu_pool(emu, W, H).reshape(-1)
        want = np.array([cpu_ref.blur_ksize(float(s)) for s in r["sigma"]])
        np.testing.assert_array_equal(r["ksize"], want)
        assert (r["sigma"][r["blur"] == 0] == 1.0).all()
        s = r["sigma"][r["blur"] == 1]
        lo, hi = float(np.float32(0.1)), 2.0
        assert lo <= s.min() < lo + 0.01 and hi - 0.01 < s.max() < hi
        j = r[r["jitter"] == 1]
        one, amount, hue = np.float32(1.0), np.float32(0.8), np.float32(0.2)  # the bounds are float32 sums
        for f in ("brightness", "contrast", "saturation"):
            assert one - amount <= j[f].min() < 0.21 and 1.79 < j[f].max() <= one + amount
        assert -hue <= j["hue"].min() < -0.199 and 0.199 < j["hue"].max() <= hue


def test_op_order_uniform(emu):
    recs = emu_pool(emu, 500, 375).reshape(-1)
    j = recs[recs["jitter"] == 1]
    perms = {p: 0 for p in itertools.permutations(range(4))}
    codes, counts = np.unique(j["order"], axis=0, return_counts=True)
    for c, n in zip(codes, counts):
        perms[tuple(int(x) for x in c)] += int(n)   # KeyError: not a permutation
    assert min(perms.values()) > 0, perms
    exp = len(j) / 24
    chi2 = sum((n - exp) ** 2 / exp for n in perms.values())
    bound = chi2_quantile(23, ALPHA)
    print(f"\nop order: chi-square {chi2:.1f} over {len(j)} records (bound {bound:.1f})")
    assert 70 < bound < 72.5 and chi2 < bound
    nj = recs[recs["jitter"] == 0]
    assert len(nj) > 1000 and (nj["order"] == [0, 1, 2, 3]).all() and (nj["hue"] == 0).all()
    assert (nj["brightness"] == 1).all() and (nj["contrast"] == 1).all() and (nj["saturation"] == 1).all()


def test_row_and_column_positions_independent(emu):
    """The two position draws of a try are separate words: |Pearson r| <= 5 / sqrt(n) between
    the normalised row and column positions of the local views that had room on both axes."""
    W, H = 500, 375
    r = emu_pool(emu, W, H)[:, 2:].reshape(-1)
    r = r[(r["crop_w"] < W) & (r["crop_h"] < H)]
    st = crop_stats(r["crop_top"], r["crop_left"], r["crop_h"], r["crop_w"], W, H)
    rho = float(np.corrcoef(st["top"], st["left"])[0, 1])
    print(f"\nrow / column position: r {rho:.4f} over {r.size} records (bound {5 / math.sqrt(r.size):.4f})")
    assert r.size > 30000 and abs(rho) <= 5 / math.sqrt(r.size)


# ------------------------------------------------------------------------------ fallback
def _central_crop(W, H):
    """torchvision's fallback (top, left, h, w) at ratio (3/4, 4/3)."""
    in_ratio = float(W) / float(H)
    if in_ratio < 3 / 4:
        w, h = W, int(round(W / (3 / 4)))
    elif in_ratio > 4 / 3:
        h, w = H, int(round(H * (4 / 3)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def _boxes(r):
    return np.stack([r["crop_top"], r["crop_left"], r["crop_h"], r["crop_w"]], -1)


def test_fallback_central_crop(emu):
    """Sizes where no try can fit give torchvision's central crop, for every view of 200 samples.

    1000 x 20 and 20 x 1000: a try's short side is at least sqrt(0.05 * 20000 * 3 / 4) = 27 > 20.
    3 x 1: a try fits only as 1 x 1, which needs target_area * aspect > 1/4 and
    target_area / aspect > 1/4, so target_area > 1/4: at the default local scale (area 0.15 to
    0.96) some tries fit, and the box is then (0, j, 1, 1); with the local scale capped at 0.08
    (area <= 0.24) none does and every local view is the central crop."""
    assert _central_crop(1000, 20) == (0, 486, 20, 27) and _central_crop(20, 1000) == (486, 0, 27, 20)
    assert _central_crop(3, 1) == (0, 1, 1, 1)
    cfg = make_aug_config(DINOAugConfig(), 224, 96, 0)
    capped = make_aug_config(DINOAugConfig(local_crops_scale=(0.05, 0.08)), 224, 96, 0)
    gen = torch.Generator().manual_seed(0)
    for W, H in ((1000, 20), (20, 1000)):
        assert cpu_ref.rrc_get_params(W, H, (0.05, 0.32), (3 / 4, 4 / 3), gen) == _central_crop(W, H)
        for s in range(200):
            b = _boxes(emu_records(emu, cfg, 7, s // 50, s, W, H))
            assert (b == _central_crop(W, H)).all(), (W, H, s, b)
    tried = 0
    for s in range(200):
        b = _boxes(emu_records(emu, capped, 7, s // 50, s, 3, 1))[2:]
        assert (b == (0, 1, 1, 1)).all(), (s, b)
        b = _boxes(emu_records(emu, cfg, 7, s // 50, s, 3, 1))[2:]
        assert (b[:, [0, 2, 3]] == (0, 1, 1)).all() and (0 <= b[:, 1]).all() and (b[:, 1] <= 2).all(), (s, b)
        tried += int((b[:, 1] != 1).sum())
    assert tried > 0  # the default scale does place 1 x 1 crops off the centre


def test_fallback_inside_ratio_is_whole_image(emu):
    """in_ratio inside [3/4, 4/3] and no try that fits: the whole image.  With the local scale
    at (0.005, 0.02) a try on 2 x 2, 3 x 4 or 4 x 3 has target_area <= 0.24, and a crop of
    at least 1 x 1 needs more than 1/4 (see test_fallback_central_crop)."""
    cfg = make_aug_config(DINOAugConfig(local_crops_scale=(0.005, 0.02)), 224, 96, 0)
    for W, H in ((2, 2), (3, 4), (4, 3)):
        assert _central_crop(W, H) == (0, 0, H, W)
        for s in range(200):
            b = _boxes(emu_records(emu, cfg, 11, 3, s, W, H))[2:]
            assert (b == (0, 0, H, W)).all(), (W, H, s, b)


# ------------------------------------------------------------------------------ keying
def _key_fields(r):
    return np.concatenate([_boxes(r), r["brightness"].view(np.uint32)[..., None].astype(np.int64)], -1)


def test_keying_black_box(emu):
    """Each of seed low word, seed high word, batch + 1, batch + 2^32, sample and view (2 vs 3,
    one spec) selects another stream: (box, brightness) differs in >= 99 % of the pairs."""
    cfg = make_aug_config(DINOAugConfig(), 224, 96, 0)
    rng = np.random.default_rng(5)
    W, H = 500, 375
    changes = {"seed_lo": lambda s, b, i: (s ^ 1, b, i), "seed_hi": lambda s, b, i: (s ^ (1 << 32), b, i),
               "batch+1": lambda s, b, i: (s, b + 1, i), "batch+2^32": lambda s, b, i: (s, b + (1 << 32), i),
               "sample": lambda s, b, i: (s, b, (i + 1) % 512)}
    same = {k: 0 for k in [*changes, "view"]}
    n = 1000
    for _ in range(n):
        base = (int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 40)), int(rng.integers(0, 512)))
        a = _key_fields(emu_records(emu, cfg, *base, W, H))
        for k, f in changes.items():
            b = _key_fields(emu_records(emu, cfg, *f(*base), W, H))
            same[k] += int((a == b).all(axis=1).sum())
        same["view"] += int((a[2] == a[3]).all())
    print(f"\nkeying: equal pairs {same} of {10 * n} (view: of {n})")
    for k, v in same.items():
        assert v <= 0.01 * (n if k == "view" else 10 * n), (k, v)


def test_neighbouring_streams_uncorrelated(emu):
    """|Pearson r| <= 5 / sqrt(N) of the area fraction and of crop_left between views 2 and 3 of
    a sample, samples s and s + 1, batches k and k + 1, seeds x and x + 1 (view 0 and view 2)."""
    cfg = make_aug_config(DINOAugConfig(), 224, 96, 0)
    W, H, N = 500, 375, N_DIST
    rng = np.random.default_rng(6)
    base, nxt = {k: [] for k in ("sample", "batch", "seed")}, {k: [] for k in ("sample", "batch", "seed")}
    for _ in range(N):
        s, b, i = int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 40)), int(rng.integers(0, 511))
        r = emu_records(emu, cfg, s, b, i, W, H)
        for k, t in (("sample", (s, b, i + 1)), ("batch", (s, b + 1, i)), ("seed", (s + 1, b, i))):
            base[k].append(r)
            nxt[k].append(emu_records(emu, cfg, *t, W, H))
    pairs = {}
    a = np.stack(base["sample"])
    pairs["view2.view3"] = (a[:, 2], a[:, 3])
    for k in base:
        x, y = np.stack(base[k]), np.stack(nxt[k])
        for v in (0, 2):
            pairs[f"{k}.view{v}"] = (x[:, v], y[:, v])
    bound, worst = 5 / math.sqrt(N), 0.0
    for name, (x, y) in pairs.items():
        for stat in ("area", "left"):
            fx = x["crop_w"] * x["crop_h"] / (W * H) if stat == "area" else x["crop_left"].astype(np.float64)
            fy = y["crop_w"] * y["crop_h"] / (W * H) if stat == "area" else y["crop_left"].astype(np.float64)
            r = float(np.corrcoef(fx, fy)[0, 1])
            worst = max(worst, abs(r))
            assert abs(r) <= bound, (name, stat, r, bound)
    print(f"\nneighbouring streams: largest |r| {worst:.4f} (bound {bound:.4f})")

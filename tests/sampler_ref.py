"""Independent restatement of the view sampler (test infrastructure, pure Python + numpy).

``dataloader_amd/csrc/sampler.hpp`` draws one ``dino_view_params`` record per (sample, view)
from a Philox4x32-10 stream.  This module restates it from the documents, not from the code:

* Philox4x32-10 as Random123 defines it (Salmon et al., SC'11): multipliers 0xD2511F53 and
  0xCD9E8D57, Weyl key increments 0x9E3779B9 and 0xBB67AE85, ten rounds;
* the stream layout of the header of ``sampler.hpp``: key = (seed low word, seed high word),
  counter = (block number from 0, view, sample, batch low word ^ batch high word * 0x9E3779B9);
  the four words of a block are consumed in order;
* the draws, in order: per RandomResizedCrop try (ten of them at most) scale, log-ratio and the
  two position words (drawn whether or not the try fits); then flip, jitter, the three words of
  the op-order shuffle, brightness, contrast, saturation, hue, grayscale, blur, sigma, solarize;
  every one is drawn for every record, whatever the flags come to;
* the arithmetic of torchvision ``RandomResizedCrop.get_params`` and ``ColorJitter.get_params``
  and of the reference's ``cpu.py:172-267`` (DINOv2) and ``400-459`` (Eval, LeJEPA): float32
  uniforms ``lo + (hi - lo) * u`` with 24-bit ``u`` (``torch.empty(1).uniform_``), 53-bit
  doubles where the reference calls ``random.random``, Python ``round`` (half to even).

float32 steps are ``np.float32`` operations, double steps are Python floats.
"""

from __future__ import annotations

import math

import numpy as np

from dataloader_amd.params import RECIPE_EVAL, RECIPE_LEJEPA, VIEW_PARAMS_DTYPE

M32 = 0xFFFFFFFF
F32 = np.float32


def philox4x32_10(ctr, key):
    """Random123 Philox4x32-10: ``ctr`` (4 words), ``key`` (2 words) -> 4 words."""
    c0, c1, c2, c3 = (int(x) & M32 for x in ctr)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


class Stream:
    """The word stream of one (seed, batch index, sample, view)."""

    def __init__(self, seed: int, batch_index: int, sample: int, view: int):
        self.key = (seed & M32, (seed >> 32) & M32)
        hi = (batch_index >> 32) & M32
        self.tail = (view & M32, sample & M32, (batch_index & M32) ^ ((hi * 0x9E3779B9) & M32))
        self.block = 0
        self.words: list[int] = []

    def word(self) -> int:
        if not self.words:
            self.words = list(philox4x32_10((self.block, *self.tail), self.key))
            self.block = (self.block + 1) & M32
        return self.words.pop(0)

    def u01f(self):
        """float32 in [0, 1) from the top 24 bits of one word."""
        return F32(self.word() >> 8) * F32(2.0 ** -24)

    def u01d(self) -> float:
        """double in [0, 1) from 27 + 26 bits of two words (``random.random``'s construction)."""
        a = self.word() >> 5
        b = self.word() >> 6
        return (a * 67108864.0 + b) * (1.0 / 9007199254740992.0)

    def below(self, n: int) -> int:
        """integer in [0, n): the high word of word * n."""
        return (self.word() * n) >> 32

    def uniform_f(self, lo, hi):
        lo, hi = F32(lo), F32(hi)
        return F32(lo + F32(F32(hi - lo) * self.u01f()))


def _rrc(g: Stream, W: int, H: int, scale) -> tuple[int, int, int, int]:
    """torchvision RandomResizedCrop.get_params(ratio=(3/4, 4/3)): (top, left, h, w)."""
    area = float(H) * float(W)
    lr0, lr1 = F32(math.log(3.0 / 4.0)), F32(math.log(4.0 / 3.0))  # torch.log(tensor(ratio)) is float32
    for _ in range(10):
        target_area = area * float(g.uniform_f(scale[0], scale[1]))
        aspect = float(F32(math.exp(float(g.uniform_f(lr0, lr1)))))
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        ri, rj = g.word(), g.word()
        if 0 < w <= W and 0 < h <= H:
            return (ri * (H - h + 1)) >> 32, (rj * (W - w + 1)) >> 32, h, w
    in_ratio = float(W) / float(H)
    if in_ratio < 3.0 / 4.0:
        w = W
        h = int(round(w / (3.0 / 4.0)))
    elif in_ratio > 4.0 / 3.0:
        h = H
        w = int(round(h * (4.0 / 3.0)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def sample_view_ref(cfg, seed: int, batch_index: int, sample: int, view: int, W: int, H: int, ok: int) -> np.ndarray:
    """The record of one (sample, view) as a 0-d ``VIEW_PARAMS_DTYPE`` array.  ``cfg`` is the
    ``DinoAugConfig`` struct of ``make_aug_config`` (its floats are float32 already)."""
    g = Stream(seed, batch_index, sample, view)
    r = np.zeros((), VIEW_PARAMS_DTYPE)
    is_global = view < cfg.n_global
    S = cfg.global_size if is_global else cfg.local_size
    scale = tuple(cfg.global_scale) if is_global else tuple(cfg.local_scale)
    if is_global:
        blur_p = cfg.blur_prob_global1 if view == 0 else cfg.blur_prob_global2
    else:
        blur_p = cfg.blur_prob_local
    sol_p = cfg.solarize_prob if view == 1 and is_global else 0.0
    W, H = max(int(W), 1), max(int(H), 1)
    top, left, ch, cw = _rrc(g, W, H, scale)
    flip = g.u01d() < float(cfg.flip_prob)                      # cpu.py:256
    jitter = not (g.u01d() > float(cfg.color_jitter_prob))      # cpu.py:202
    order = [0, 1, 2, 3]
    for i in (3, 2, 1):                                         # torch.randperm(4) as Fisher-Yates
        j = g.below(i + 1)
        order[i], order[j] = order[j], order[i]
    one = F32(1.0)
    factors = []
    for amount in (cfg.brightness, cfg.contrast, cfg.saturation):  # ColorJitter: [max(0, 1 - x), 1 + x]
        lo = F32(one - F32(amount))
        factors.append(g.uniform_f(lo if lo > 0 else F32(0.0), F32(one + F32(amount))))
    hue = g.uniform_f(-F32(cfg.hue), F32(cfg.hue))
    gray = g.u01d() < float(cfg.grayscale_prob)                 # cpu.py:262
    blur = not (g.u01d() > float(blur_p))                       # cpu.py:216
    smin, smax = float(cfg.blur_sigma_min), float(cfg.blur_sigma_max)
    sigma = smin + (smax - smin) * g.u01d()                     # random.uniform, cpu.py:218
    su = g.u01d()
    solarize = sol_p > 0 and su < float(sol_p)                  # cpu.py:265
    if not blur:
        sigma = 1.0
    ksize = max(3, int(sigma * 4 + 1) | 1)                      # cpu.py:219
    rw = rh = ox = oy = 0
    if cfg.recipe == RECIPE_LEJEPA:     # context: RRC + jitter + flip; targets: RRC only (cpu.py:447-459)
        gray = blur = solarize = False
        sigma, ksize = 1.0, 3
        if not is_global:
            flip = jitter = False
    elif cfg.recipe == RECIPE_EVAL:     # Resize(int(S * 256 / 224)) + CenterCrop(S) (cpu.py:400-411)
        size = int(S * 256 / 224)
        if W <= H:
            nw, nh = size, int(size * H / W)
        else:
            nw, nh = int(size * W / H), size
        flip = jitter = gray = blur = solarize = False
        sigma, ksize = 1.0, 3
        top = left = 0
        cw, ch, rw, rh = W, H, nw, nh
        ox, oy = int(round((nw - S) / 2.0)), int(round((nh - S) / 2.0))
        if nw == W:                     # an axis that is not resampled is a plain crop
            left, cw, rw, ox = ox, S, S, 0
        if nh == H:
            top, ch, rh, oy = oy, S, S, 0
    if not jitter:
        factors, hue, order = [one, one, one], F32(0.0), [0, 1, 2, 3]
    r["crop_top"], r["crop_left"], r["crop_h"], r["crop_w"], r["out_size"] = top, left, ch, cw, S
    r["flip"], r["jitter"], r["gray"], r["blur"], r["solarize"] = flip, jitter, gray, blur, solarize
    r["order"] = order
    r["brightness"], r["contrast"], r["saturation"] = factors
    r["hue"] = hue
    r["sigma"] = sigma
    r["ksize"] = ksize
    r["pad1"] = 0 if ok else 1
    r["resize_w"], r["resize_h"], r["out_x"], r["out_y"] = rw, rh, ox, oy
    return r


def draw_dims(cfg, status: int, width: int, height: int) -> tuple[int, int, int]:
    """(W, H, ok) a decoded batch's image is drawn from: a decoded image (status 0) its own size;
    any other 1 x 1, flagged in ``pad1``, except that LeJEPA crops an undecodable one (status < 0)
    from a black 224 x 224 canvas (cpu.py:446-448), unflagged."""
    if status == 0:
        return width, height, 1
    if status < 0 and cfg.recipe == RECIPE_LEJEPA:
        return 224, 224, 1
    return 1, 1, 0


def sample_batch_ref(cfg, seed: int, batch_index: int, images) -> np.ndarray:
    """The records ``dino_sample_params`` writes for a decoded batch, sample-major
    (``[b * n_views + v]``).  ``images`` is one (status, width, height) per image."""
    nv = cfg.n_global + cfg.n_local
    out = np.zeros(len(images) * nv, VIEW_PARAMS_DTYPE)
    for b, img in enumerate(images):
        dims = draw_dims(cfg, *img)
        for v in range(nv):
            out[b * nv + v] = sample_view_ref(cfg, seed, batch_index, b, v, *dims)
    return out


def assert_records_equal(got: np.ndarray, want: np.ndarray, what: str = "") -> None:
    """Field for field, floats by their bits; names the first record and field that differ."""
    got = np.ascontiguousarray(got, VIEW_PARAMS_DTYPE).reshape(-1)
    want = np.ascontiguousarray(want, VIEW_PARAMS_DTYPE).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    bits = {"f": {4: np.uint32, 8: np.uint64}}
    for name in VIEW_PARAMS_DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype.kind == "f":
            a, b = a.view(bits["f"][a.dtype.itemsize]), b.view(bits["f"][b.dtype.itemsize])
        bad = np.flatnonzero((a != b).reshape(len(got), -1).any(axis=1))
        if bad.size:
            i = int(bad[0])
            raise AssertionError(f"{what}: {bad.size} of {len(got)} records differ in {name!r}; first is record {i}: "
                                 f"got {got[i]!r}, want {want[i]!r}")
    raise AssertionError(f"{what}: records differ outside the named fields")

"""k_params on the device: the records dino_sample_params writes equal the host's, bit for bit.

The device draws with its own ``log`` / ``exp`` / ``sqrt`` / ``rint`` in double; both builds use
-ffp-contract=off, ``sqrt`` is correctly rounded, and ``exp`` feeds a float cast (a one-ulp
double difference shows only next to a float rounding midpoint, about 2^-29 per draw), so
equality is the bar: with ``tests/sampler_ref.py`` (the independent restatement) and with the
host emulator (the same source compiled for the CPU).  Also pinned: the launch bounds (no write
past the last record at B = 1, 7, 64, 256 and 10, 4 and 1 views, a short batch's records are a
prefix of the full batch's) and the pipeline's keying (call k draws from (seed, k)).
"""

from __future__ import annotations

import io

import numpy as np
import pytest
import torch
from PIL import Image

from dataloader_amd.config import DINOAugConfig, EvalAugSpec, LeJEPAAugSpec, recipe_aug_config
from dataloader_amd.engine import IngestEngine, pack_jpegs
from dataloader_amd.params import RECORD_BYTES, VIEW_PARAMS_DTYPE, make_aug_config
from dataloader_amd.synthetic import make_jpeg
from tests.sampler_ref import assert_records_equal, draw_dims, sample_batch_ref
from tests.test_sampler_cpu import emu_records

pytestmark = pytest.mark.gpu

B_MAX = 256
GUARD = 4 * RECORD_BYTES
# the sizes the 256 files cycle through; None is a corrupt file (one inside the first 7 images)
SIZES = [(1, 1), (8, 8), None, (17, 9), (64, 64), (300, 100), (100, 300), (1000, 20), (20, 1000), (500, 375),
         (1199, 899), None]
# one seed and one batch index from 2^32 up
KEYS = [(21, 0), ((0x9E37 << 32) | 12345, 7), (99, (1 << 32) + 5)]


def _flat_jpeg(w, h, colour):
    b = io.BytesIO()
    Image.new("RGB", (w, h), colour).save(b, format="JPEG", quality=85)
    return b.getvalue()


def _recipes():
    return {"dinov2": make_aug_config(DINOAugConfig(), 224, 96, 0),
            "lejepa": make_aug_config(recipe_aug_config(LeJEPAAugSpec()), 224, 96, 0),
            "lejepa4": make_aug_config(recipe_aug_config(LeJEPAAugSpec(n_target_views=3)), 224, 96, 0),
            "eval": make_aug_config(recipe_aug_config(EvalAugSpec()), 224, 224, 0)}


class _Batch:
    def __init__(self, device):
        corrupt = [b"not a jpeg at all", make_jpeg(64, 64, 1)[:300]]  # no SOI; cut inside the tables
        unique = [corrupt.pop(0) if s is None else _flat_jpeg(*s, (40 + 17 * i, 200 - 9 * i, 90))
                  for i, s in enumerate(SIZES)]
        self.sizes = [SIZES[i % len(SIZES)] for i in range(B_MAX)]
        buf, off = pack_jpegs([unique[i % len(SIZES)] for i in range(B_MAX)], pin=False)
        self.device = device
        self.d_bytes, self.d_off = buf.to(device), off.to(device)
        self.eng = IngestEngine(device, max_batch=B_MAX, max_views=10, max_crop_size=224)
        self.images = None

    def decode(self, B):
        """Decode the first B files; (status, width, height) per image, checked against the list."""
        info = self.eng.decode(self.d_bytes, self.d_off[:B + 1], B).cpu().numpy()
        images = [(int(s), int(w), int(h)) for s, w, h, _ in info]
        for (s, w, h), size in zip(images, self.sizes):
            assert (s < 0) if size is None else (s, w, h) == (0, *size), (s, w, h, size)
        return images

    def records(self, cfg, seed, batch_index, B):
        """dino_sample_params into a buffer with 4 records' worth of 0xA5 after the last one."""
        n = B * (cfg.n_global + cfg.n_local) * RECORD_BYTES
        buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=self.device)
        self.eng.sample_params(cfg, seed, batch_index, out=buf)
        torch.cuda.synchronize()
        raw = buf.cpu().numpy()
        assert (raw[n:] == 0xA5).all(), f"B={B}: bytes after the last record were written"
        return raw[:n].view(VIEW_PARAMS_DTYPE).copy()


@pytest.fixture(scope="module")
def batch(gpu_device):
    b = _Batch(gpu_device)
    yield b
    b.eng.close()


@pytest.mark.parametrize("recipe", ["dinov2", "lejepa", "eval"])
def test_device_equals_host(batch, emu, recipe):
    """Every record of 256 images x 3 (seed, batch index) pairs equals the restatement and the
    emulator; undecodable files draw from 1 x 1 (flagged), under LeJEPA from the 224 x 224 canvas."""
    cfg = _recipes()[recipe]
    nv = cfg.n_global + cfg.n_local
    images = batch.decode(B_MAX)
    assert sum(s < 0 for s, _, _ in images) >= 2
    for seed, bi in KEYS:
        got = batch.records(cfg, seed, bi, B_MAX)
        assert_records_equal(got, sample_batch_ref(cfg, seed, bi, images), f"{recipe} device vs restatement ({seed:#x}, {bi:#x})")
        host = np.concatenate([emu_records(emu, cfg, seed, bi, b, *draw_dims(cfg, *img)) for b, img in enumerate(images)])
        assert_records_equal(got, host, f"{recipe} device vs emulator ({seed:#x}, {bi:#x})")
        bad = got.reshape(B_MAX, nv)[[s < 0 for s, _, _ in images]]
        if recipe == "lejepa":   # the canvas: unflagged, a box inside 224 x 224 and mostly larger than 1 x 1
            assert (bad["pad1"] == 0).all() and (bad["crop_w"] * bad["crop_h"] > 1).mean() > 0.9
            assert (bad["crop_left"] + bad["crop_w"] <= 224).all() and (bad["crop_top"] + bad["crop_h"] <= 224).all()
        else:
            assert (bad["pad1"] == 1).all() and (got["pad1"].sum() == bad.size)


@pytest.mark.parametrize("recipe,nv", [("dinov2", 10), ("lejepa4", 4), ("eval", 1)])
def test_launch_bounds(batch, recipe, nv):
    """B = 1, 7, 64, 256 at 10, 4 and 1 views: nothing is written after the last record, and the
    records of a short batch are the first records of the full batch on the same files."""
    cfg = _recipes()[recipe]
    assert cfg.n_global + cfg.n_local == nv
    seed, bi = KEYS[1]
    images = batch.decode(B_MAX)
    full = batch.records(cfg, seed, bi, B_MAX)
    assert_records_equal(full[:7 * nv], sample_batch_ref(cfg, seed, bi, images[:7]), f"{recipe} first 7 images")
    for B in (1, 7, 64):
        batch.decode(B)
        got = batch.records(cfg, seed, bi, B)
        assert got.size == B * nv
        assert_records_equal(got, full[:B * nv], f"{recipe} B={B} vs the first records of B={B_MAX}")


def test_pipeline_keys_calls_by_batch_index(gpu_device):
    """run_device_batch three times on the same 8 images: call k's records are the draws of
    (seed, k), and no record of one call appears in another."""
    from dataloader_amd.pipeline import MI355XAugPipeline
    sizes = [(160, 120), (96, 80), (64, 64), (300, 100), (100, 300), (225, 333), (500, 375), (33, 17)]
    jpegs = [make_jpeg(w, h, i) for i, (w, h) in enumerate(sizes)]
    buf, off = pack_jpegs(jpegs, pin=False)
    d_bytes, d_off = buf.to(gpu_device), off.to(gpu_device)
    acfg = DINOAugConfig()
    seed = (5 << 32) | 77
    pipe = MI355XAugPipeline(None, acfg, 8, seed=seed, device=0)
    cfg = make_aug_config(acfg, 224, 96, 0)
    images = [(0, w, h) for w, h in sizes]
    calls = []
    for k in range(3):
        pipe.run_device_batch(d_bytes, d_off, 8)
        torch.cuda.synchronize()
        assert (pipe.last_status() == 0).all()
        recs = pipe.last_params().copy()
        assert_records_equal(recs, sample_batch_ref(cfg, seed, k, images), f"pipeline call {k}")
        calls.append({r.tobytes() for r in recs})
    pipe.close()
    assert all(len(c) == 80 for c in calls)
    assert not (calls[0] & calls[1]) and not (calls[0] & calls[2]) and not (calls[1] & calls[2])

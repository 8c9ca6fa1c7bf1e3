"""Reduced-size JPEG decode on the device (``dino_ctx_set_draft``, ``MI355XBackend(jpeg_draft=N)``)
against Pillow's ``im.draft("RGB", (N, N)); im.convert("RGB")`` on the same bytes, bit for bit."""

from __future__ import annotations

import io

import numpy as np
import pytest
import torch
from PIL import Image

from dataloader_amd import fallback
from dataloader_amd.config import DINOAugConfig, DinoV2AugSpec, PipelineConfig
from dataloader_amd.engine import IngestEngine
from dataloader_amd.synthetic import textured_rgb
from oracle import cpu_ref
from tests import jpeg_writer as jw
from tests import sampling_cases as sc
from tests.helpers import record_to_params
from tests.test_gpu_parity import _to_dev

pytestmark = pytest.mark.gpu

SIZES = ((8, 8), (17, 9), (70, 50), (129, 65))


def _draft(data: bytes, n: int):
    try:
        im = Image.open(io.BytesIO(data))
        if n:
            im.draft("RGB", (n, n))
        return im.convert("RGB")
    except Exception:  # noqa: BLE001 - the reference zero-fills
        return None


def _jpeg(w, h, sampling, seed, **kw) -> bytes:
    img = textured_rgb(w, h, np.random.default_rng(seed))
    if sampling == "440":
        return sc._seq(img, "s440")
    b = io.BytesIO()
    im = Image.fromarray(img)
    (im.convert("L") if sampling == "gray" else im).save(
        b, "JPEG", quality=90, **({} if sampling == "gray" else {"subsampling": sampling}), **kw)
    return b.getvalue()


def _cases():
    out = [(f"{smp}_{w}x{h}_s{s}", dict(w=w, h=h, sampling=smp, seed=w + s), min(w, h) // s, False)
           for smp in ("gray", "4:4:4", "4:2:0", "4:2:2", "440") for (w, h) in SIZES for s in (2, 4, 8)]
    for s in (2, 4, 8):
        out.append((f"restart_s{s}", "restart", 50 // s, False))
        out.append((f"prog_wave_s{s}", dict(w=70, h=50, sampling="4:2:0", seed=s, progressive=True), 50 // s, False))
        out.append((f"prog_lanes_s{s}", dict(w=70, h=50, sampling="4:2:0", seed=s, progressive=True), 50 // s, True))
    return out


@pytest.fixture(scope="module")
def eng(gpu_device):
    return IngestEngine(gpu_device, max_batch=16, max_views=10, max_crop_size=224)


def _check(eng, dev, files, n, raw_mask=None):
    d_bytes, d_off = _to_dev(files, dev)
    rm = None if raw_mask is None else torch.tensor(raw_mask, dtype=torch.uint8, device=dev)
    info = eng.decode(d_bytes, d_off, len(files), raw_mask=rm).cpu().numpy()
    for i, f in enumerate(files):
        ref = _draft(f, n) if raw_mask is None or not raw_mask[i] else Image.frombytes(
            "RGB", (int.from_bytes(f[4:8], "little"), int.from_bytes(f[8:12], "little")), f[16:])
        if ref is None:
            assert info[i, 0] != 0, i
            continue
        assert tuple(info[i, :3]) == (0, *ref.size), (i, info[i], ref.size)
        got = eng.copy_rgb(i, *ref.size).cpu().numpy()
        assert np.array_equal(got, np.asarray(ref)), (i, int((got != np.asarray(ref)).sum()))


@pytest.mark.parametrize("name,spec,n,lanes", _cases(), ids=[c[0] for c in _cases()])
def test_decode_parity(gpu_device, eng, name, spec, n, lanes):
    if spec == "restart":  # one MCU row per interval
        data = jw.encode(textured_rgb(70, 50, np.random.default_rng(7)), sc.ONE_SCAN, samp=((2, 2), (1, 1), (1, 1)), restart=5)
    else:
        data = _jpeg(**spec)
    eng.set_prog_decoder(lanes)
    eng.set_draft(n)
    _check(eng, gpu_device, [data], n)
    eng.set_prog_decoder(False)


@pytest.mark.parametrize("size", [s for s in sc.SMALL_SIZES if min(s) >= 2], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sampling_cases_at_half_size(gpu_device, eng, size):
    """Every layout of sampling_cases.py (4:1:1, 4:1:0, Cb != Cr ..) at s = 2: the per-pixel path."""
    files = [j for name, j in sc.small_cases() if name.endswith(f"_{size[0]}x{size[1]}")]
    n = min(size) // 2
    assert len(files) == len(sc.LAYOUTS) and fallback.draft_scale(*size, n)[0] == 2
    eng.set_draft(n)
    _check(eng, gpu_device, files, n)


def test_mixed_batch_twice_on_one_context(gpu_device):
    rng = np.random.default_rng(11)
    b = io.BytesIO()
    Image.fromarray(textured_rgb(90, 70, rng)).save(b, "PNG")
    files = [_jpeg(40, 30, "4:2:0", 1), _jpeg(200, 136, "4:2:0", 2), fallback.raw_container(textured_rgb(100, 80, rng)),
             b.getvalue(), _jpeg(129, 65, "4:4:4", 3, progressive=True)]
    e = IngestEngine(gpu_device, max_batch=len(files), max_views=10, max_crop_size=224)
    e.set_png(True)
    e.set_draft(32)
    for _ in range(2):
        _check(e, gpu_device, files, 32, raw_mask=[0, 0, 1, 0, 0])


def test_option_off_is_the_full_size_decode(gpu_device):
    _check(IngestEngine(gpu_device, max_batch=1, max_views=10, max_crop_size=224), gpu_device,
           [_jpeg(70, 50, "4:2:0", 5)], 0)


def test_views_through_the_backend(gpu_device):
    from dataloader_amd.backend import MI355XBackend
    from tests.test_gpu_round3 import _ListSource, _collect
    rng = np.random.default_rng(13)
    sizes = ((70, 50), (100, 80), (130, 70), (200, 136), (96, 64), (160, 120), (180, 100))
    batch = [_jpeg(w, h, ("4:2:0", "4:4:4")[k & 1], 20 + k, progressive=k == 2) for k, (w, h) in enumerate(sizes)]
    b = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, size=(90, 120, 4), dtype=np.uint8), "CMYK").save(b, "JPEG")
    batch.append(b.getvalue())  # handed over
    cfg = DINOAugConfig(global_crop_size=32, local_crop_size=16, n_local_crops=2, blur_prob_global1=0.0,
                        blur_prob_global2=0.0, blur_prob_local=0.0)
    spec = DinoV2AugSpec(aug_cfg=cfg)
    be = MI355XBackend(host_workers=2, side_ahead=2, jpeg_draft=32)
    pipe = be.build_pipeline(_ListSource([batch]), spec, PipelineConfig(gpu_queue=1, seed=9, output_dtype="fp32"), None)
    outs = _collect(be.build_pipeline_iterator(pipe, spec, spec.output_map, len(batch)))
    st = pipe.flush_stats()
    assert len(outs) == 1 and st["side_decoded"] == 1 and st["host_decoded"] == 1 and set(st["status"]) == {0}, st
    recs = pipe.last_params()
    for i, data in enumerate(batch):
        img = _draft(data, 32)
        for v, name in enumerate(spec.output_map):
            p = record_to_params(recs[i * cfg.n_views + v])
            ref = cpu_ref.augment_one(data, p, cfg.mean, cfg.std, out_dtype=torch.float32, decoded=img)
            assert torch.equal(outs[0][name][i].cpu(), ref), (i, v, img.size)
    pipe.close()

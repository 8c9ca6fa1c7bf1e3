"""EXIF orientation on the device (``dino_ctx_set_exif_transpose``, ``MI355XBackend(exif_transpose=
True)``) against Pillow's ``ImageOps.exif_transpose(Image.open(b)).convert("RGB")`` on the same
bytes, bit for bit."""

from __future__ import annotations

import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

from dataloader_amd import _lib, fallback
from dataloader_amd.config import DINOAugConfig, DinoV2AugSpec, PipelineConfig, UserAugSpec
from dataloader_amd.engine import IngestEngine
from dataloader_amd.synthetic import textured_rgb
from oracle import cpu_ref
from tests import header_cases as hc
from tests.helpers import record_to_params
from tests.test_gpu_parity import _to_dev
from tests.test_gpu_round3 import _ListSource, _collect

pytestmark = pytest.mark.gpu


def _jpeg(w, h, o, seed, mode="RGB", **kw) -> bytes:
    rng = np.random.default_rng(seed)
    im = Image.fromarray(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), "CMYK") if mode == "CMYK" \
        else Image.fromarray(textured_rgb(w, h, rng)).convert(mode)
    ex, b = Image.Exif(), io.BytesIO()
    ex[0x0112] = o
    im.save(b, "JPEG", quality=90, **({"exif": ex.tobytes()} if o else {}), **kw)
    return b.getvalue()


def _ref(data: bytes, turn: bool = True, draft: int = 0) -> Image.Image:
    im = Image.open(io.BytesIO(data))
    if draft:
        im.draft("RGB", (draft, draft))
    return (ImageOps.exif_transpose(im) if turn else im).convert("RGB")


def _unverified(w, h, seed) -> bytes:  # orientation 6 as a LONG: Pillow turns it, the device's walk declines
    return hc.insert(_jpeg(w, h, 0, seed, subsampling="4:2:0"), "app0", hc.seg(0xE1, hc.EXIF + hc._tiff([(0x0112, 4, 1, 6)])))


@functools.lru_cache(maxsize=None)
def _batch() -> tuple:
    T = _lib.load().dino_orient_tile()
    files = [_jpeg(w, h, o, 8 * k + o, subsampling="4:2:0")
             for k, (w, h) in enumerate(((1, 1), (T - 1, T + 1), (T, T), (T + 1, 2 * T + 1), (37, 21))) for o in range(1, 9)]
    files += [_jpeg(T + 1, T - 1, 6, 91, subsampling="4:4:4"), _jpeg(T + 1, T - 1, 6, 92, mode="L"),
              _jpeg(T + 1, T - 1, 6, 93, subsampling="4:2:0", progressive=True), _jpeg(T + 1, T - 1, 6, 94, mode="CMYK")]
    return tuple(files), _unverified(T + 1, T - 1, 95)


@pytest.mark.parametrize("on", [True, False], ids=["on", "off"])
def test_decode_is_exif_transpose(gpu_device, on):
    files = list(_batch()[0]) + [_batch()[1]]
    eng = IngestEngine(gpu_device, max_batch=len(files), max_views=1, max_crop_size=32)
    eng.set_four_component(True)
    eng.set_exif_transpose(on)
    orient = fallback.probe_orient_list(files)
    assert orient[-1] == fallback.ORIENT_UNVERIFIED and sorted(set(orient[:-1])) == [0, 2, 3, 4, 5, 6, 7, 8]
    d_bytes, d_off = _to_dev(files, gpu_device)
    for _ in range(2):
        info = eng.decode(d_bytes, d_off, len(files)).cpu().numpy()
        for i, f in enumerate(files):
            ref = _ref(f, turn=on and i != len(files) - 1)  # (routing the unverified file to Pillow is the pipeline's job)
            assert tuple(info[i, :3]) == (0, *ref.size), (i, info[i], ref.size)
            got = eng.copy_rgb(i, *ref.size).cpu().numpy()
            assert np.array_equal(got, np.asarray(ref)), (i, int(orient[i]), ref.size, int((got != np.asarray(ref)).sum()))
    eng.close()


def test_draft_then_transpose(gpu_device):
    data = _jpeg(130, 70, 5, 7, subsampling="4:2:0")
    eng = IngestEngine(gpu_device, max_batch=1, max_views=1, max_crop_size=32)
    eng.set_draft(16)
    eng.set_exif_transpose(True)
    info = eng.decode(*_to_dev([data], gpu_device), 1).cpu().numpy()
    ref = _ref(data, draft=16)
    assert ref.size == (18, 33) and tuple(info[0, :3]) == (0, 18, 33)
    assert np.array_equal(eng.copy_rgb(0, 18, 33).cpu().numpy(), np.asarray(ref))
    eng.close()


@pytest.mark.parametrize("route", ["side", "device"])
def test_views_through_the_backend(gpu_device, route):
    from dataloader_amd.backend import MI355XBackend
    sizes = ((70, 50), (100, 80), (130, 70), (200, 136), (96, 64), (160, 120))
    batch = [_jpeg(w, h, (6, 8, 3, 5, 2, 7)[k], 20 + k, subsampling="4:2:0", progressive=k in (1, 3))
             for k, (w, h) in enumerate(sizes)]
    batch += [_unverified(120, 90, 30), _jpeg(180, 100, 0, 31)]
    spec = DinoV2AugSpec(aug_cfg=DINOAugConfig(global_crop_size=32, local_crop_size=16, n_local_crops=2, blur_prob_global1=0.0,
                                               blur_prob_global2=0.0, blur_prob_local=0.0))
    cfg = spec.aug_cfg
    be = MI355XBackend(host_workers=2, side_ahead=2, multiscan_route=route, exif_transpose=True)
    pipe = be.build_pipeline(_ListSource([batch]), spec, PipelineConfig(gpu_queue=1, seed=9, output_dtype="fp32"), None)
    outs = _collect(be.build_pipeline_iterator(pipe, spec, spec.output_map, len(batch)))
    st = pipe.flush_stats()
    assert len(outs) == 1 and set(st["status"]) == {0} and st["host_decoded"] == 1, st
    assert st["orient_device"] == 6 and st["orient_host"] == 1 and st["side_decoded"] == (2 if route == "side" else 0), st
    recs = pipe.last_params()
    for i, data in enumerate(batch):
        img = _ref(data)
        for v, name in enumerate(spec.output_map):
            p = record_to_params(recs[i * cfg.n_views + v])
            ref = cpu_ref.augment_one(data, p, cfg.mean, cfg.std, out_dtype=torch.float32, decoded=img)
            assert torch.equal(outs[0][name][i].cpu(), ref), (i, v, img.size)
    pipe.close()


def test_user_aug_spec_sees_the_upright_image(gpu_device):
    from dataloader_amd.backend import MI355XBackend
    data, upright = _jpeg(48, 32, 6, 41, subsampling="4:2:0"), io.BytesIO()
    spec = UserAugSpec(aug_fn=lambda x: {"a": x}, _output_map=["a"], decode_size=32, warn_not_dali=False)
    be = MI355XBackend(exif_transpose=True)
    pipe = be.build_pipeline(_ListSource([[data]]), spec, PipelineConfig(output_dtype="fp32"), None)
    out = next(be.build_pipeline_iterator(pipe, spec, spec.output_map, 1))[0]["a"].cpu()
    _ref(data).save(upright, "PNG")
    ref = cpu_ref.decode_only_one(upright.getvalue(), 32, spec.mean, spec.std, out_dtype=torch.float32)
    assert out.shape == (1, 3, 48, 32) and torch.equal(out[0], ref)
    pipe.close()

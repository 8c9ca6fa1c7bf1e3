"""Four-component (Adobe CMYK / YCCK) JPEGs on the device (``dino_ctx_set_four_component``,
``MI355XBackend(four_component="device")``): every file of ``tests/cmyk_cases.py`` against
Pillow on the same bytes, bit for bit; the option off keeps today's status 1.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from dataloader_amd.config import DINOAugConfig, DinoV2AugSpec, PipelineConfig
from dataloader_amd.engine import IngestEngine, params_from_device
from dataloader_amd.params import OUT_BF16, VIEW_PARAMS_DTYPE, make_aug_config
from dataloader_amd.synthetic import encode_jpeg, textured_rgb
from tests import cmyk_cases as cc
from tests.test_gpu_parity import _check_views, _to_dev
from tests.test_gpu_round3 import _ListSource, _collect

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files():
    return cc.cases()


@pytest.fixture(scope="module")
def refs(files):
    return {n: cc.pillow_rgb(b) for n, b in files.items()}


@pytest.mark.parametrize("lane", [False, True])
def test_decode_bit_exact_with_the_option_on(gpu_device, files, refs, lane):
    """Both settings of dino_ctx_set_prog_decoder (the lane decoder declines four-component
    images: they end up on the wave decoder).  Where Pillow raises: negative status, zeros."""
    names = list(files)
    jpegs = [files[n] for n in names]
    eng = IngestEngine(gpu_device, max_batch=len(jpegs), max_views=10, max_crop_size=224)
    eng.set_four_component(True)
    eng.set_prog_decoder(lane)
    d_bytes, d_off = _to_dev(jpegs, gpu_device)
    info = eng.decode(d_bytes, d_off, len(jpegs)).cpu().numpy()
    bad = []
    for i, n in enumerate(names):
        ref, st = refs[n], int(info[i, 0])
        w, h = cc.size_of(files[n])
        if ref is None:
            got = eng.copy_rgb(i, w, h).cpu().numpy()  # (an image that failed is skipped: the zeros stay)
            if st >= 0 or got.any():
                bad.append((n, "reference rejects; status", st))
        elif st != 0:
            bad.append((n, "status", st))
        elif (int(info[i, 1]), int(info[i, 2]), int(info[i, 3])) != (w, h, 4):
            bad.append((n, "info", info[i].tolist()))
        else:
            got = eng.copy_rgb(i, w, h).cpu().numpy()
            if not np.array_equal(got, ref):
                bad.append((n, "bytes differing", int((got != ref).sum())))
    eng.close()
    assert not bad, f"{len(bad)} of {len(names)}: {bad}"


def test_option_off_reports_unsupported(gpu_device, files):
    """The default, and the option switched off again on the same context: status 1 for every file."""
    jpegs = list(files.values()) + [encode_jpeg(textured_rgb(64, 48, np.random.default_rng(1)))]
    eng = IngestEngine(gpu_device, max_batch=len(jpegs), max_views=10, max_crop_size=224)
    d_bytes, d_off = _to_dev(jpegs, gpu_device)
    for toggle in (None, True, False):
        if toggle is not None:
            eng.set_four_component(toggle)
        st = eng.decode(d_bytes, d_off, len(jpegs)).cpu().numpy()[:, 0]
        if toggle:
            assert (st[:-1] <= 0).all() and (st[:-1] == 0).sum() >= len(files) - 2
        else:
            assert (st[:-1] == 1).all(), st
        assert st[-1] == 0
    eng.close()


@pytest.mark.parametrize("route", ["side", "device"])
def test_backend_device_option_matches_the_pillow_hand_over(gpu_device, files, route):
    """A 16-image batch with two CMYK files, one YCCK file and one progressive CMYK file (and
    plain batches around it): MI355XBackend(four_component="device") gives the views of the
    default backend (Pillow hand-over) bit for bit, with no hand-over."""
    from dataloader_amd.backend import MI355XBackend
    rng = np.random.default_rng(60)
    uniq = [encode_jpeg(textured_rgb(160 + 8 * s, 120 + 4 * s, rng)) for s in range(5)]
    B, nb = 16, 3
    batches = [[uniq[(k + i) % 5] for i in range(B)] for k in range(nb)]
    batches[1][2] = files["pil_base_70x50"]
    batches[1][7] = files["cmyk_k1_70x50"]
    batches[1][11] = files["ycck_10blk_70x50"]
    batches[1][14] = files["pil_prog_70x50"]
    batches[2][0] = encode_jpeg(textured_rgb(96, 64, rng), progressive=True)
    spec = DinoV2AugSpec(aug_cfg=DINOAugConfig(global_crop_size=64, local_crop_size=32, n_local_crops=2))

    def run(**kw):
        be = MI355XBackend(host_workers=2, multiscan_route=route, side_ahead=2, **kw)
        pipe = be.build_pipeline(_ListSource(batches), spec, PipelineConfig(gpu_queue=2, seed=5), None)
        outs = _collect(be.build_pipeline_iterator(pipe, spec, spec.output_map, B))
        st = pipe.flush_stats()
        pipe.close()
        return outs, st

    (ref, st0), (got, st1) = run(), run(four_component="device")
    assert len(ref) == len(got) == nb
    assert st0["host_decoded"] == 4 and st0["four_component"] == 0, st0
    assert st1["host_decoded"] == 0 and st1["four_component"] == 4, st1
    assert set(st0["status"]) == set(st1["status"]) == {0}
    if route == "side":  # they join the side pools like the progressive file
        assert st0["side_decoded"] == 1 and st1["side_decoded"] == 5, (st0, st1)
    for k, (a, b) in enumerate(zip(ref, got)):
        for name in a:
            assert torch.equal(a[name], b[name]), (k, name)
    for v in got[1].values():  # not zeros
        assert all(torch.count_nonzero(v[i].float()) > 0 for i in (2, 7, 11, 14))


def test_augment_parity_on_a_ten_block_ycck_file(gpu_device, files):
    """Device-drawn records against the oracle fed Pillow's RGB (as test_augment_parity_on_unusual_mcus)."""
    jpegs = [files["ycck_10blk_70x50"], files["ycck_prog_sa_10blk_70x50"],
             files["ycck_12blk_one_scan_33x31"], files["truncated_mid_scan_70x50"]]  # Pillow raises: zero views
    cfg = DINOAugConfig(global_crop_size=64, local_crop_size=32, n_local_crops=2)
    B = len(jpegs)
    eng = IngestEngine(gpu_device, max_batch=B, max_views=cfg.n_views, max_crop_size=64)
    eng.set_four_component(True)
    d_bytes, d_off = _to_dev(jpegs, gpu_device)
    params = torch.empty(B * cfg.n_views * VIEW_PARAMS_DTYPE.itemsize, dtype=torch.uint8, device=gpu_device)
    views, info = eng.run_batch(d_bytes, d_off, B, make_aug_config(cfg, 64, 32, OUT_BF16), seed=77, batch_index=1,
                                params_out=params)
    torch.cuda.synchronize()
    st = info[:, 0].cpu().numpy()
    assert (st[:2] == 0).all() and (st[2:] < 0).all(), info
    _check_views(jpegs, views, params_from_device(params), cfg.n_views, torch.bfloat16, cfg.mean, cfg.std)
    assert all(torch.count_nonzero(v[i].float()) == 0 for v in views for i in (2, 3))
    eng.close()

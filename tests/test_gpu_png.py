"""PNG files on the device (``dino_ctx_set_png``, ``MI355XBackend(png="device")``): every file
of ``tests/png_cases.py`` against Pillow on the same bytes, bit for bit, and against the host
model's statuses; the option off keeps status -1 and zero views.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from dataloader_amd.config import DINOAugConfig
from dataloader_amd.engine import IngestEngine
from dataloader_amd.pipeline import MI355XAugPipeline
from dataloader_amd.synthetic import make_jpeg
from tests import png_cases as pc
from tests.test_gpu_parity import _to_dev
from tests.test_png_cpu import EMU, model_decode

pytestmark = pytest.mark.gpu

CASES = pc.cases()


@pytest.fixture(scope="module")
def emu():
    return ctypes.CDLL(str(EMU))


@pytest.fixture(scope="module")
def refs():
    return {c[0]: pc.pillow_rgb(c[1]) for c in CASES}


def _decode(eng, files, dev):
    d_bytes, d_off = _to_dev(files, dev)
    eng.reserve(sum(len(f) for f in files) * 8 + (64 << 20), 0)
    return eng.decode(d_bytes, d_off, len(files)).cpu().numpy()


def test_case_list_bit_exact_with_the_option_on(gpu_device, emu, refs):
    files = [c[1] for c in CASES]
    eng = IngestEngine(gpu_device, max_batch=len(files), max_views=10, max_crop_size=224)
    eng.set_png(True)
    info = _decode(eng, files, gpu_device)
    bad = []
    for i, (name, data, expect) in enumerate(CASES):
        m, zs, inf, _ = model_decode(emu, data)
        st = int(info[i, 0])
        if expect == "gap":
            continue
        if st != int(m[0]):
            bad.append((name, "status", st, "model", int(m[0])))
            continue
        if expect != "dev":
            continue
        ref = refs[name]
        got = eng.copy_rgb(i, ref.shape[1], ref.shape[0]).cpu().numpy()
        if not np.array_equal(got, ref):
            # name the failing stage from the two debug regions
            z = eng.debug_region(i, 10, len(zs)).cpu().numpy()
            r = eng.debug_region(i, 11, len(inf)).cpu().numpy()
            stage = "k_pngwalk" if not np.array_equal(z, zs) else "k_inflate" if not np.array_equal(r, inf) else "k_unfilter"
            bad.append((name, stage, int((got != ref).sum())))
    eng.close()
    assert not bad, bad


def test_option_off_keeps_status_minus_one_and_zero_views(gpu_device):
    files = [c[1] for c in CASES]  # every PNG of the list
    eng = IngestEngine(gpu_device, max_batch=len(files), max_views=10, max_crop_size=224)
    info = _decode(eng, files, gpu_device)
    assert (info[:, 0] == -1).all(), info[:, 0]
    eng.close()
    cfg = DINOAugConfig(global_crop_size=32, local_crop_size=16, n_local_crops=2)
    pipe = MI355XAugPipeline(lambda: files[:4], cfg, batch_size=4, seed=3, out_dtype="fp32")
    out = pipe.run_one_batch()
    torch.cuda.synchronize()
    assert all(not out[f"view_{v}"].any() for v in range(cfg.n_views))
    pipe.close()


def test_mixed_batch_twice_on_one_context(gpu_device, refs):
    """Baseline JPEG, progressive JPEG, PNGs of every block type and a declined PNG, decoded
    twice on one context: leftover tables or ring state would show in the second pass."""
    from pathlib import Path
    prog = (Path(__file__).resolve().parent / "golden" / "prog_640x480.jpg").read_bytes()
    names = ["zlib_300x200", "ring_wrap", "five_blocks", "all_15bit", "palette_short", "depth16", "stored_65535"]
    by = {c[0]: c[1] for c in CASES}
    files = [make_jpeg(64, 48, 2), by[names[0]], prog] + [by[n] for n in names[1:]]
    eng = IngestEngine(gpu_device, max_batch=len(files), max_views=10, max_crop_size=224)
    eng.set_png(True)
    for _ in range(2):
        info = _decode(eng, files, gpu_device)
        assert info[0, 0] == 0 and info[2, 0] == 0
        for i, n in [(1, names[0])] + [(3 + k, n) for k, n in enumerate(names[1:])]:
            if n == "depth16":
                assert info[i, 0] == 1
                continue
            ref = refs[n]
            assert info[i, 0] == 0, (n, info[i])
            assert np.array_equal(eng.copy_rgb(i, ref.shape[1], ref.shape[0]).cpu().numpy(), ref), n
    eng.close()


def test_130_pngs_on_a_small_grid(gpu_device, refs, monkeypatch):
    """More tickets than resident waves: DINO_INFLATE_WAVES=3 makes three waves take 130 images."""
    monkeypatch.setenv("DINO_INFLATE_WAVES", "3")
    pool = [c for c in CASES if c[2] == "dev" and len(c[1]) < 4096]
    pick = [pool[k % len(pool)] for k in range(130)]
    eng = IngestEngine(gpu_device, max_batch=130, max_views=10, max_crop_size=224)
    eng.set_png(True)
    info = _decode(eng, [c[1] for c in pick], gpu_device)
    assert (info[:, 0] == 0).all(), info[:, 0]
    for i in (0, 64, 65, 129):
        ref = refs[pick[i][0]]
        assert np.array_equal(eng.copy_rgb(i, ref.shape[1], ref.shape[0]).cpu().numpy(), ref), pick[i][0]
    eng.close()


def _run_backend(batches, route, **kw):
    from dataloader_amd.backend import MI355XBackend
    from dataloader_amd.config import DinoV2AugSpec, PipelineConfig
    from tests.test_gpu_round3 import _ListSource, _collect
    spec = DinoV2AugSpec(aug_cfg=DINOAugConfig(global_crop_size=64, local_crop_size=32, n_local_crops=2))
    be = MI355XBackend(host_workers=2, multiscan_route=route, side_ahead=2, **kw)
    pipe = be.build_pipeline(_ListSource(batches), spec, PipelineConfig(gpu_queue=2, seed=5), None)
    outs = _collect(be.build_pipeline_iterator(pipe, spec, spec.output_map, len(batches[0])))
    st = pipe.flush_stats()
    pipe.close()
    return outs, st


def test_backend_modes(gpu_device):
    """B = 16 from a host list source, a PNG batch between two plain ones: png="device" gives the
    views of png="host" (Pillow's pixels through the same augment kernels, which
    tests/test_gpu_parity.py holds to the oracle) bit for bit on the side route and on
    multiscan_route="device"; the counts are right; png="off" gives zeros for the PNGs."""
    by = {c[0]: c[1] for c in CASES}
    pngs = {2: "zlib_300x200", 4: "alternate5", 7: "palette", 9: "filter4_bpp4", 11: "depth16", 13: "apng", 14: "rows129"}
    uniq = [make_jpeg(160 + 8 * s, 120 + 4 * s, s) for s in range(5)]
    B, nb = 16, 3
    batches = [[uniq[(k + i) % 5] for i in range(B)] for k in range(nb)]
    for i, n in pngs.items():
        batches[1][i] = by[n]
    (dev, st), (host, sth) = _run_backend(batches, "side", png="device"), _run_backend(batches, "side", png="host")
    (direct, _), (off, sto) = _run_backend(batches, "device", png="device"), _run_backend(batches, "side")
    assert st["png_device"] == 5 and st["png_host"] == 2 and st["host_decoded"] == 2 and st["side_decoded"] == 5, st
    assert sth["png_device"] == 0 and sth["png_host"] == 7 and sth["host_decoded"] == 7, sth
    assert sto["png_device"] == 0 and sto["png_host"] == 0 and sto["host_decoded"] == 0, sto
    assert len(dev) == len(host) == len(direct) == len(off) == nb
    for k in range(nb):
        for name in dev[k]:
            assert torch.equal(dev[k][name], host[k][name]), (k, name)
            assert torch.equal(dev[k][name], direct[k][name]), (k, name)
            for i in range(B):
                if k == 1 and i in pngs:
                    assert not off[k][name][i].any() and dev[k][name][i].any(), (name, i)
                else:
                    assert torch.equal(off[k][name][i], dev[k][name][i]), (k, name, i)


@pytest.mark.parametrize("route", ["side", "device"])
def test_backend_device_views_against_the_oracle(gpu_device, route):
    """MI355XBackend(png="device"), B = 16 from a host list source: every view of the PNG batch
    against the CPU oracle fed Pillow's pixels of the same file (bit-exact but for blur within
    one level on <= 0.5 % of a view: tests/test_gpu_round3.py _check_pipeline_views), device
    PNGs and handed-over ones alike."""
    from dataloader_amd.backend import MI355XBackend
    from dataloader_amd.config import DinoV2AugSpec, PipelineConfig
    from tests.test_gpu_round3 import _ListSource, _check_pipeline_views, _collect
    by = {c[0]: c[1] for c in CASES}
    names = ["zlib_300x200", "alternate5", "palette", "filter4_bpp4", "depth16", "apng", "rows129", "ring_wrap",
             "filter3_bpp2", "trns_gray", "idat_300_chunks", "stored_65535"]
    batch = [by[n] for n in names] + [make_jpeg(160 + 8 * s, 120 + 4 * s, s) for s in range(4)]
    cfg = DINOAugConfig(global_crop_size=64, local_crop_size=32, n_local_crops=2)
    spec = DinoV2AugSpec(aug_cfg=cfg)
    be = MI355XBackend(host_workers=2, multiscan_route=route, side_ahead=2, png="device")
    pipe = be.build_pipeline(_ListSource([batch]), spec, PipelineConfig(gpu_queue=1, seed=9), None)
    outs = _collect(be.build_pipeline_iterator(pipe, spec, spec.output_map, len(batch)))
    assert len(outs) == 1
    st = pipe.flush_stats()
    assert st["png_device"] == 10 and st["png_host"] == 2 and set(st["status"]) == {0}, st
    out = {f"view_{v}": outs[0][n] for v, n in enumerate(spec.output_map)}
    _check_pipeline_views(pipe, batch, out, cfg.n_views)
    assert all(out[f"view_{v}"][b].any() for v in range(cfg.n_views) for b in range(len(batch)))
    pipe.close()


@pytest.mark.parametrize("mode", ["off", "host", "device"])
def test_user_aug_pipeline_hands_pngs_over(gpu_device, mode):
    """UserAugSpec through MI355XBackend(png=...): "host" and "device" hand every PNG Pillow may
    decode to it (the oracle's decode-only output, bit for bit); "off" leaves them zeros."""
    from oracle import cpu_ref
    from dataloader_amd.backend import MI355XBackend
    from dataloader_amd.config import PipelineConfig, UserAugSpec
    import zlib
    # square files, so that the decode-only resize gives one shape to stack: two PNGs the device
    # would take, a JPEG, and a 16-bit gray PNG it declines
    files = [pc.pw.simple(pc._pix(s, s, 3, s), 2, types=(4,)) for s in (40, 33)] + [make_jpeg(64, 64, 1)]
    files.append(pc.pw.png(8, 8, 0, zlib.compress(bytes([0] + [0x12, 0x34] * 8) * 8), depth=16))

    class Src:
        _batch_size = len(files)
        _resolution_src = None

        def __call__(self):
            return files

    spec = UserAugSpec(aug_fn=lambda x: {"a": x}, _output_map=["a"], decode_size=32, warn_not_dali=False)
    be = MI355XBackend(png=mode)
    pipe = be.build_pipeline(Src(), spec, PipelineConfig(output_dtype="fp32"), None)
    out = next(be.build_pipeline_iterator(pipe, spec, spec.output_map, len(files)))[0]["a"].cpu()
    torch.cuda.synchronize()
    for b, f in enumerate(files):
        ref = cpu_ref.decode_only_one(f, 32, spec.mean, spec.std, out_dtype=torch.float32)
        if mode == "off" and f[:4] == b"\x89PNG":
            assert not out[b].any(), b
        else:
            assert torch.equal(out[b], ref), (mode, b)
    assert pipe.flush_stats()["host_decoded"] == (0 if mode == "off" else 3)
    pipe.close()


def test_bogus_mode_raises():
    from dataloader_amd.backend import MI355XBackend
    with pytest.raises(ValueError):
        MI355XBackend(png="bogus")

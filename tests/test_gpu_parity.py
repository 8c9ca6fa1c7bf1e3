"""GPU parity: the HIP path through the C ABI vs the CPU oracle on the same bytes.

Tolerances:
  * decode: bit-exact RGB vs Pillow (libjpeg-turbo) for every supported JPEG;
  * resize / jitter / hue / grayscale / solarize / normalize / casts: bit-exact;
  * gaussian blur: the reference's float32 kernel comes from torch.exp/sum whose
    CPU implementation (MKL/Sleef, ISA dependent) is not reproducible bit for bit;
    blurred views may differ by exactly 1 uint8 level (=1/255/std before the cast)
    on <= 0.5 % of the pixels of a view;
  * masks: bit-exact.
"""

from __future__ import annotations

import random

import numpy as np
import pytest
import torch

from dataloader_amd.config import DINOAugConfig
from dataloader_amd.engine import IngestEngine, pack_jpegs, params_from_device, params_to_device
from dataloader_amd.params import OUT_BF16, OUT_FP8_E4M3, OUT_FP32, VIEW_PARAMS_DTYPE, make_aug_config
from dataloader_amd.synthetic import encode_jpeg, make_jpeg, textured_rgb
from oracle import cpu_ref
from oracle.masking_ref import RefMaskingGenerator
from tests.helpers import dc_extremes_rgb, record_to_params

pytestmark = pytest.mark.gpu

STD_MIN = min(cpu_ref.IMAGENET_STD)
ONE_LEVEL = 1.0 / 255.0 / STD_MIN


def _jpeg_zoo():
    rng = np.random.default_rng(123)
    out = []
    # 640x480: one segment, short lanes (finished by k_huff1); 1024x768: one segment, long
    # lanes (k_huff3); 1601x1203: several segments (k_huff2 cross-segment sync)
    for (w, h) in [(64, 64), (225, 333), (640, 480), (17, 9), (8, 8), (33, 17), (1, 1), (1024, 768), (1601, 1203)]:
        for sub in (0, 1, 2):
            out.append(encode_jpeg(textured_rgb(w, h, rng), quality=85, subsampling=sub))
    out.append(encode_jpeg(textured_rgb(200, 150, rng), gray=True))
    out.append(encode_jpeg(textured_rgb(640, 480, rng), restart_mcus=7))
    out.append(encode_jpeg(textured_rgb(321, 123, rng), restart_mcus=40, subsampling=0))
    out.append(encode_jpeg(textured_rgb(300, 200, rng), quality=50))
    out.append(encode_jpeg(textured_rgb(300, 200, rng), quality=95))
    for sub, q in ((0, 95), (2, 95), (2, 50)):
        out.append(encode_jpeg(dc_extremes_rgb(160, 96, rng), quality=q, subsampling=sub))
    return out


def _to_dev(jpegs, device):
    buf, off = pack_jpegs(jpegs, pin=False)
    return buf.to(device), off.to(device)


def test_decode_bit_exact(gpu_device):
    jpegs = _jpeg_zoo()
    eng = IngestEngine(gpu_device, max_batch=len(jpegs), max_views=10, max_crop_size=224)
    d_bytes, d_off = _to_dev(jpegs, gpu_device)
    info = eng.decode(d_bytes, d_off, len(jpegs)).cpu().numpy()
    bad = []
    for i, j in enumerate(jpegs):
        ref = np.asarray(cpu_ref.decode_rgb(j))
        assert info[i, 0] == 0, f"image {i} status {info[i, 0]}"
        assert (info[i, 1], info[i, 2]) == (ref.shape[1], ref.shape[0])
        got = eng.copy_rgb(i, ref.shape[1], ref.shape[0]).cpu().numpy()
        if not np.array_equal(got, ref):
            bad.append((i, int((got != ref).sum())))
    eng.close()
    assert not bad, f"decode mismatches (image, n bytes): {bad}"


def _check_views(jpegs, views, recs, nv, out_dtype, mean, std):
    worst = 0
    for b, jpg in enumerate(jpegs):
        img = cpu_ref.decode_rgb(jpg)
        for v in range(nv):
            p = record_to_params(recs[b * nv + v])
            ref = cpu_ref.augment_one(jpg, p, mean, std, out_dtype=out_dtype, decoded=img).float()
            got = views[v][b].cpu().float()
            diff = (ref - got).abs()
            if p.blur:
                tol = ONE_LEVEL + (0.0161 if out_dtype == torch.bfloat16 else 0.26 if out_dtype != torch.float32 else 1e-6)
                assert diff.max().item() <= tol, f"b{b} v{v} blur max {diff.max().item()}"
                frac = (diff > 0).float().mean().item()
                assert frac <= 0.005, f"b{b} v{v} blur: {frac:.4%} of pixels differ"
                worst = max(worst, frac)
            else:
                assert torch.equal(ref, got), f"b{b} v{v}: {int((diff > 0).sum())} values differ (max {diff.max()})"
    return worst


@pytest.mark.parametrize("out_code,tdtype", [(OUT_BF16, torch.bfloat16), (OUT_FP32, torch.float32),
                                             (OUT_FP8_E4M3, torch.float8_e4m3fn)])
def test_augment_parity_device_params(gpu_device, out_code, tdtype):
    cfg = DINOAugConfig()  # 2x224 + 8x96, reference defaults
    rng = np.random.default_rng(5)
    jpegs = [make_jpeg(int(rng.integers(100, 700)), int(rng.integers(100, 700)), int(s)) for s in range(6)]
    jpegs.append(encode_jpeg(textured_rgb(90, 300, rng), gray=True))
    jpegs.append(b"not a valid jpeg")  # reference cpu.py:250-253 -> zeros
    B = len(jpegs)
    eng = IngestEngine(gpu_device, max_batch=B, max_views=cfg.n_views, max_crop_size=224)
    ccfg = make_aug_config(cfg, 224, 96, out_code)
    d_bytes, d_off = _to_dev(jpegs, gpu_device)
    params = torch.empty(B * cfg.n_views * VIEW_PARAMS_DTYPE.itemsize, dtype=torch.uint8, device=gpu_device)
    views, info = eng.run_batch(d_bytes, d_off, B, ccfg, seed=1234, batch_index=3, params_out=params)
    torch.cuda.synchronize()
    recs = params_from_device(params)
    st = info[:, 0].cpu().numpy()
    assert (st[:-1] == 0).all() and st[-1] < 0
    for v in views:
        assert v.dtype == tdtype
    assert all(torch.count_nonzero(v[-1].float()) == 0 for v in views)
    _check_views(jpegs[:-1], [v[:-1] for v in views], recs, cfg.n_views, tdtype, cfg.mean, cfg.std)
    eng.close()


def test_augment_parity_reference_draws(gpu_device):
    """Params drawn in CPUBackend's own order (torch + python RNG), fed through the C ABI."""
    cfg = DINOAugConfig(global_crop_size=32, local_crop_size=16, n_local_crops=2)  # reference small_aug_cfg
    ocfg = cpu_ref.AugCfg(global_crop_size=32, local_crop_size=16, n_local_crops=2)
    jpegs = [make_jpeg(64, 64, s) for s in range(4)]
    gen = torch.Generator().manual_seed(0)
    rnd = random.Random(0)
    table = cpu_ref.view_table(ocfg)
    recs = []
    from tests.helpers import params_to_record
    for j in jpegs:
        w, h = cpu_ref.decode_rgb(j).size
        for spec in table:
            recs.append(params_to_record(cpu_ref.draw_params_like_cpubackend(w, h, spec, ocfg, gen, rnd)))
    recs = np.stack(recs)
    eng = IngestEngine(gpu_device, max_batch=4, max_views=cfg.n_views, max_crop_size=32)
    d_bytes, d_off = _to_dev(jpegs, gpu_device)
    eng.decode(d_bytes, d_off, 4)
    views = eng.augment(make_aug_config(cfg, 32, 16, OUT_BF16), params_to_device(recs, gpu_device))
    torch.cuda.synchronize()
    _check_views(jpegs, views, recs, cfg.n_views, torch.bfloat16, cfg.mean, cfg.std)
    eng.close()


def test_masks_bit_exact(gpu_device):
    from dataloader_amd.masking import MaskingGenerator
    for grid, seed in [(14, 0), (16, 1), (37, 42)]:
        ref = RefMaskingGenerator(grid, py_rng=random.Random(seed), np_rng=np.random.RandomState(seed))
        g = MaskingGenerator(grid, device=gpu_device)
        g.seed(seed)
        got = g.generate(8).cpu().numpy()
        for k in range(8):
            np.testing.assert_array_equal(got[k], ref(flat=True))
    # reference-API path: global RNG side effects identical
    random.seed(42)
    np.random.seed(42)
    g = MaskingGenerator((16, 16), device=gpu_device)
    m1 = g(flat=True)
    after_py, after_np = random.random(), np.random.randint(1 << 30)
    random.seed(42)
    np.random.seed(42)
    ref = RefMaskingGenerator((16, 16), py_rng=random, np_rng=np.random.mtrand._rand)
    np.testing.assert_array_equal(m1, ref(flat=True))
    assert (random.random(), np.random.randint(1 << 30)) == (after_py, after_np)


def test_fp8_formatter(gpu_device):
    from dataloader_amd.backend import HipFP8Formatter
    x = torch.randn(3, 4, 5, 6, device=gpu_device).to(torch.bfloat16) * 3
    got = HipFP8Formatter().quantise(x)
    assert got.dtype == torch.float8_e4m3fn
    ref = x.cpu().to(torch.float8_e4m3fn)
    assert torch.equal(got.cpu().view(torch.uint8), ref.view(torch.uint8))
    # every bf16 bit pattern (NaN payloads, infinities, saturation at +-448, subnormals, ties),
    # whole, with a ragged tail (no multiple of the block), and through non-contiguous views
    allbf = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    d_all = allbf.to(gpu_device)
    grid = d_all.view(256, 256)
    for name, x in [("all", d_all), ("ragged", d_all[:65536 - 3]), ("offset", d_all[3:]), ("strided", d_all[::3]),
                    ("transposed", grid.t()), ("columns", grid[:, 5:250])]:
        got = HipFP8Formatter().quantise(x)
        assert got.dtype == torch.float8_e4m3fn and got.shape == x.shape, name
        ref = x.cpu().to(torch.float8_e4m3fn)
        assert torch.equal(got.cpu().contiguous().view(torch.uint8), ref.contiguous().view(torch.uint8)), name


def test_pipeline_iterator_and_close(gpu_device):
    from dataloader_amd.backend import MI355XBackend
    from dataloader_amd.config import DinoV2AugSpec, PipelineConfig, ResolutionSource
    cfg = DINOAugConfig(global_crop_size=32, local_crop_size=16, n_local_crops=2, max_global_crop_size=64,
                        max_local_crop_size=32)
    res = ResolutionSource(32, 16)
    calls = [0]

    def source():
        if calls[0] >= 2:
            raise StopIteration
        calls[0] += 1
        return [np.frombuffer(make_jpeg(64, 64, calls[0] * 10 + i), np.uint8) for i in range(4)]
    source._batch_size = 4
    source._resolution_src = res
    be = MI355XBackend()
    spec = DinoV2AugSpec(aug_cfg=cfg)
    pipe = be.build_pipeline(source, spec, PipelineConfig(device_id=0, seed=0))
    it = be.build_pipeline_iterator(pipe, spec, spec.output_map, 4)
    out = next(it)[0]
    assert out["view_0"].shape == (4, 3, 32, 32) and out["view_3"].shape == (4, 3, 16, 16)
    assert out["view_0"].device.type == "cuda"
    res.set(64, 32)
    out = next(it)[0]
    assert out["view_0"].shape == (4, 3, 64, 64) and out["view_2"].shape == (4, 3, 32, 32)
    with pytest.raises(StopIteration):
        next(it)
    pipe.close()
    pipe.close()
    with pytest.raises(RuntimeError, match="close"):
        pipe.run_one_batch()


def test_bench_pattern_multi_batch(gpu_device):
    """The benchmark's access pattern: one device-resident dataset, offset slices, reused views."""
    from dataloader_amd.pipeline import MI355XAugPipeline
    cfg = DINOAugConfig()
    uniq = [make_jpeg(640, 480, s) for s in range(8)]
    jpegs = [uniq[i % 8] for i in range(96)]
    buf, off = pack_jpegs(jpegs, pin=True)
    d_bytes, d_off = buf.to(gpu_device), off.to(gpu_device)
    B = 32
    pipe = MI355XAugPipeline(None, cfg, B, seed=3, device=0)
    views = pipe.engine.alloc_views(pipe._cfg(224, 96), B)
    sums = []
    for k in range(6):
        s = (k % 3) * B
        pipe.run_device_batch(d_bytes, d_off[s:s + B + 1], B, views=views)
        assert (pipe.last_status() == 0).all()
        sums.append(float(views[0].float().abs().sum()))
    torch.cuda.synchronize()
    recs = pipe.last_params()
    _check_views(jpegs[96 - B:], views, recs, cfg.n_views, torch.bfloat16, cfg.mean, cfg.std)
    pipe.close()


def _edge_records(dims, gsize, lsize):
    """Hand-made records that reach every branch of the resize / blur kernels:
    crop == S on one or both axes (no resample pass), S % 4 != 0 (scalar paths),
    crops too wide for LDS staging (direct path), blur kernel sizes 3..13
    (templated and generic), every jitter op order, flip, gray, solarize."""
    P = cpu_ref.ViewParams
    recs = []
    from tests.helpers import params_to_record
    orders = [(3, 2, 1, 0), (1, 0, 2, 3), (0, 1, 2, 3), (2, 3, 0, 1)]
    for k, (w, h) in enumerate(dims):
        views = []
        for v, S in enumerate((gsize, gsize, lsize, lsize)):
            cw = [w, min(S, w), min(w, S if v == 3 else w // 2 + 1), S if S <= w else w][v]
            ch = [h, min(S, h), min(h, S), min(h, h // 2 + 1)][v]
            if v == 1 and (w < S or h < S):
                cw, ch = w, h
            top, left = (h - ch) // 3, (w - cw) // 2
            ks = [9, 13, 11, 3, 5, 7][(k + v) % 6]
            while ks // 2 >= S:
                ks -= 2
            views.append(P(out_size=S, crop_top=top, crop_left=left, crop_h=ch, crop_w=cw, flip=bool((k + v) & 1),
                           jitter=v != 2, order=orders[(k + v) % 4], brightness=1.25, contrast=0.7, saturation=1.3,
                           hue=[0.1, -0.07, 0.03, -0.2][v], gray=(k + v) % 3 == 0, blur=v != 1,
                           sigma=[1.9, 2.6, 2.4, 0.5, 1.1, 1.6][(k + v) % 6] * ks / 9 + 0.1, ksize=ks,
                           solarize=v == 1))
        recs += [params_to_record(p) for p in views]
    return np.stack(recs)


@pytest.mark.parametrize("gsize,lsize", [(30, 18), (32, 16)])
def test_augment_edge_paths(gpu_device, gsize, lsize):
    rng = np.random.default_rng(9)
    dims = [(12000, 24), (7000, 40), (300, 200), (gsize, gsize), (lsize, 50), (41, lsize)]
    jpegs = [encode_jpeg(textured_rgb(w, h, rng), quality=90) for w, h in dims]
    cfg = DINOAugConfig(global_crop_size=gsize, local_crop_size=lsize, n_local_crops=2)
    recs = _edge_records(dims, gsize, lsize)
    eng = IngestEngine(gpu_device, max_batch=len(jpegs), max_views=4, max_crop_size=32, max_image_dim=16384)
    d_bytes, d_off = _to_dev(jpegs, gpu_device)
    info = eng.decode(d_bytes, d_off, len(jpegs)).cpu().numpy()
    assert (info[:, 0] == 0).all(), info
    for out_code, tdtype in [(OUT_BF16, torch.bfloat16), (OUT_FP32, torch.float32)]:
        views = eng.augment(make_aug_config(cfg, gsize, lsize, out_code), params_to_device(recs, gpu_device))
        torch.cuda.synchronize()
        _check_views(jpegs, views, recs, 4, tdtype, cfg.mean, cfg.std)
    eng.close()


def test_decode_marker_edge_cases(gpu_device):
    """Entropy-segment edge cases of the destuffing pass, at every byte alignment
    of the packed buffer: 0xFF fill bytes before EOI (legal, B.1.1.2), junk after
    EOI, a scan cut before EOI (Pillow raises -> TRUNCATED), a lone trailing 0xFF,
    restart markers, and the last image ending exactly at the end of the buffer."""
    rng = np.random.default_rng(77)
    base = encode_jpeg(textured_rgb(120, 90, rng), quality=90)
    dri = encode_jpeg(textured_rgb(160, 64, rng), restart_mcus=2)
    assert base[-2:] == b"\xff\xd9"
    cases = [
        (base, 0),
        (base[:-2] + b"\xff\xff\xff\xd9", 0),
        (base + b"trailing junk \xff\x00\xff", 0),
        (base[: len(base) * 3 // 4], -2),
        (base[:-2] + b"\xff", -2),
        (dri, 0),
        (dri[:-2] + b"\xff\xff\xd9", 0),
    ]
    for pad in range(16):
        jpegs = [b"\0" * pad] + [c for c, _ in cases] + [base]
        eng = IngestEngine(gpu_device, max_batch=len(jpegs), max_views=10, max_crop_size=224)
        d_bytes, d_off = _to_dev(jpegs, gpu_device)
        d_bytes = d_bytes[: int(d_off[-1])].clone()  # exact-size buffer: no slack after the last image
        info = eng.decode(d_bytes, d_off, len(jpegs)).cpu().numpy()
        assert info[0, 0] < 0
        for i, (data, want) in enumerate(cases + [(base, 0)], start=1):
            ref = cpu_ref.decode_rgb(data)
            assert (ref is None) == (want != 0), i
            assert info[i, 0] == want, f"pad {pad} case {i}: status {info[i, 0]} want {want}"
            if want == 0:
                got = eng.copy_rgb(i, int(info[i, 1]), int(info[i, 2])).cpu().numpy()
                np.testing.assert_array_equal(got, np.asarray(ref), err_msg=f"pad {pad} case {i}")
        eng.close()


def test_depth2_overlap_matches_serial(gpu_device):
    """Two batches in flight (two ctx + streams) give bit-identical views to the
    serial pipeline for the same (seed, batch index); the prefetching iterator
    hands batches over in order."""
    from dataloader_amd.pipeline import MI355XAugPipeline, MI355XPipelineIterator
    cfg = DINOAugConfig()
    uniq = [make_jpeg(320 + 16 * s, 240 + 8 * s, s) for s in range(8)]
    B = 16
    batches = [[uniq[(k * 3 + i) % 8] for i in range(B)] for k in range(5)]

    def run(depth):
        src = iter(batches)
        pipe = MI355XAugPipeline(lambda: next(src), cfg, B, seed=11, device=0, depth=depth)
        it = MI355XPipelineIterator(pipe, [f"view_{i}" for i in range(cfg.n_views)], B)
        outs = [{k: v.clone() for k, v in out[0].items()} for out in it]
        torch.cuda.synchronize()
        pipe.close()
        return outs

    serial, overlapped = run(1), run(2)
    assert len(serial) == len(overlapped) == len(batches)
    for a, b in zip(serial, overlapped):
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_shm_shard_feed_matches_python_source(gpu_device, tmp_path):
    """C5 feed: tar shards in the /dev/shm cache format -> native index -> pinned gather
    -> H2D gives bit-identical views to the Python list source on the same JPEG bytes,
    at depth 1 and 3 (per-slot pinned staging reuse)."""
    import io
    import tarfile

    from dataloader_amd.pipeline import MI355XAugPipeline, MI355XPipelineIterator
    from dataloader_amd.tario import ShardBatchFeeder, ShmShardCache
    cfg = DINOAugConfig()
    uniq = [make_jpeg(200 + 8 * s, 160 + 4 * s, s) for s in range(7)]
    B, nb = 12, 4
    jpegs = [uniq[(i * 5) % 7] for i in range(B * nb + 5)]
    cache = ShmShardCache(job_id="feedtest", base_dir=tmp_path)
    paths = []
    for s0 in range(0, len(jpegs), 10):  # shards of 10: batches straddle shards
        buf = io.BytesIO()
        with tarfile.open(fileobj=buf, mode="w") as tf:
            for i in range(s0, min(len(jpegs), s0 + 10)):
                ti = tarfile.TarInfo(f"sample_{i:06d}.jpg")
                ti.size = len(jpegs[i])
                tf.addfile(ti, io.BytesIO(jpegs[i]))
        paths.append(f"/x/shard-{s0:04d}.tar")
        cache.put(paths[-1], buf.getvalue())

    def run(source, depth):
        pipe = MI355XAugPipeline(source, cfg, B, seed=5, device=0, depth=depth)
        it = MI355XPipelineIterator(pipe, [f"view_{i}" for i in range(cfg.n_views)], B)
        outs = [{k: v.clone() for k, v in out[0].items()} for out in it]
        torch.cuda.synchronize()
        pipe.close()
        return outs

    src = iter([jpegs[k * B:(k + 1) * B] for k in range(nb)])
    ref = run(lambda: next(src), 1)
    for depth in (1, 3):
        got = run(ShardBatchFeeder(cache, paths, B, nthreads=3), depth)
        assert len(got) == len(ref) == nb          # the partial last batch is dropped
        for a, b in zip(ref, got):
            for k in a:
                assert torch.equal(a[k], b[k]), (depth, k)
    cache.close(remove=True)


def test_per_dataset_normalisation(gpu_device):
    """Per-image {mean, std} (DALI NormSource semantics, reference pipeline.py:109-180) through
    dino_set_norm, wired by MI355XBackend.build_pipeline from the specs and the source's
    dataset-index callback: each image matches the oracle run with its dataset's stats."""
    from dataloader_amd.backend import MI355XBackend
    from dataloader_amd.config import DinoV2AugSpec, PipelineConfig
    from dataloader_amd.pipeline import MI355XPipelineIterator

    class Spec:
        def __init__(self, mean, std):
            self.mean, self.std = mean, std

    specs = [Spec(None, None), Spec((0.5, 0.4, 0.3), (0.25, 0.2, 0.3)), Spec((0.1, 0.2, 0.3), (0.5, 0.6, 0.7))]
    cfg = DINOAugConfig(global_crop_size=64, local_crop_size=32, n_local_crops=2)
    rng = np.random.default_rng(9)
    jpegs = [make_jpeg(int(rng.integers(90, 300)), int(rng.integers(90, 300)), s) for s in range(6)]
    ds_idx = [0, 1, 2, 1, 7, 0]  # 7 is past the table: last entry (norm_utils.py:78-86)

    class Source:
        _batch_size = 6
        _resolution_src = None

        def __init__(self):
            self.cbs = []

        def register_dataset_index_callback(self, cb):
            self.cbs.append(cb)

        def __call__(self):
            for cb in self.cbs:
                cb(ds_idx)
            return jpegs

    src = Source()
    pipe = MI355XBackend().build_pipeline(src, DinoV2AugSpec(cfg), PipelineConfig(output_dtype="fp32", seed=3), specs)
    it = MI355XPipelineIterator(pipe, [f"view_{i}" for i in range(cfg.n_views)], 6)
    out = next(it)[0]
    torch.cuda.synchronize()
    recs = pipe.last_params()
    nv = cfg.n_views
    for b, jpg in enumerate(jpegs):
        sp = specs[min(ds_idx[b], len(specs) - 1)]
        mean = sp.mean or cfg.mean
        std = sp.std or cfg.std
        img = cpu_ref.decode_rgb(jpg)
        for v in range(nv):
            p = record_to_params(recs[b * nv + v])
            ref = cpu_ref.augment_one(jpg, p, mean, std, out_dtype=torch.float32, decoded=img)
            got = out[f"view_{v}"][b].cpu()
            tol = ONE_LEVEL * max(STD_MIN / min(std), 1.0) + 1e-6 if p.blur else 0.0
            assert (ref - got).abs().max().item() <= tol, (b, v)
    pipe.close()


@pytest.mark.parametrize("dtype,tdtype", [("fp32", torch.float32), ("bf16", torch.bfloat16)])
def test_eval_spec_parity(gpu_device, dtype, tdtype):
    """EvalAugSpec (reference CPUEvalPipeline, cpu.py:395-413): resize shorter side to
    int(S*256/224) BICUBIC + centre crop on the same kernels (a window of the resampled
    image); bit-exact vs the oracle, including images whose one axis is not resampled."""
    from dataloader_amd.backend import MI355XBackend
    from dataloader_amd.config import EvalAugSpec, PipelineConfig
    from dataloader_amd.pipeline import MI355XPipelineIterator
    rng = np.random.default_rng(21)
    sizes = [(640, 480), (480, 640), (256, 400), (300, 256), (257, 1000), (1111, 333), (256, 256), (90, 70)]
    jpegs = [encode_jpeg(textured_rgb(w, h, rng), quality=90) for w, h in sizes] + [b"corrupt"]
    spec = EvalAugSpec(crop_size=224)

    class Src:
        _batch_size = len(jpegs)
        _resolution_src = None

        def __call__(self):
            return jpegs

    pipe = MI355XBackend().build_pipeline(Src(), spec, PipelineConfig(output_dtype=dtype), None)
    out = next(MI355XPipelineIterator(pipe, spec.output_map, len(jpegs)))[0]["view_0"].cpu()
    torch.cuda.synchronize()
    assert out.shape == (len(jpegs), 3, 224, 224) and out.dtype == tdtype
    for b, j in enumerate(jpegs):
        ref = cpu_ref.eval_one(j, 224, out_dtype=tdtype)
        assert torch.equal(ref, out[b]), f"{sizes[b] if b < len(sizes) else 'corrupt'}: {(ref.float() - out[b].float()).abs().max()}"
    pipe.close()


def test_lejepa_spec_parity(gpu_device):
    """LeJEPAAugSpec (reference CPULeJEPAPipeline, cpu.py:435-461): context view with RRC +
    ColorJitter + flip, targets with RRC only, on the same kernels; every view matches the
    oracle replay of its record and the recipe's flags hold."""
    from dataloader_amd.backend import MI355XBackend
    from dataloader_amd.config import LeJEPAAugSpec, PipelineConfig
    from dataloader_amd.pipeline import MI355XPipelineIterator
    rng = np.random.default_rng(22)
    jpegs = [make_jpeg(int(rng.integers(150, 500)), int(rng.integers(150, 500)), s) for s in range(6)]
    spec = LeJEPAAugSpec(n_target_views=3)

    class Src:
        _batch_size = len(jpegs)
        _resolution_src = None

        def __call__(self):
            return jpegs

    pipe = MI355XBackend().build_pipeline(Src(), spec, PipelineConfig(output_dtype="fp32", seed=5), None)
    out = next(MI355XPipelineIterator(pipe, spec.output_map, len(jpegs)))[0]
    torch.cuda.synchronize()
    assert list(out) == spec.output_map
    recs = pipe.last_params()
    nv = 1 + spec.n_target_views
    assert not recs["blur"].any() and not recs["gray"].any() and not recs["solarize"].any()
    r2 = recs.reshape(-1, nv)
    assert not r2[:, 1:]["flip"].any() and not r2[:, 1:]["jitter"].any()
    assert r2[:, 0]["jitter"].any() and (r2[:, 0]["out_size"] == 224).all() and (r2[:, 1:]["out_size"] == 96).all()
    for b, j in enumerate(jpegs):
        img = cpu_ref.decode_rgb(j)
        for v, name in enumerate(spec.output_map):
            p = record_to_params(recs[b * nv + v])
            ref = cpu_ref.augment_one(j, p, spec.mean, spec.std, out_dtype=torch.float32, decoded=img)
            assert torch.equal(ref, out[name][b].cpu()), (b, name)
    pipe.close()

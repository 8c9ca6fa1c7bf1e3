"""Round-3 GPU tests: the drop-in path as the measured path, and the last zero-fill gaps.

* ``MI355XBackend.build_pipeline`` maps ``PipelineConfig.gpu_queue`` to batches in flight
  (reference pipeline.py:317, dali_backend.py:163-164) with the host half on a prefetch
  thread; its output must be bit-identical to the serial (depth 1, no thread) pipeline,
  including Pillow hand-overs made on that thread;
* any JPEG side (<= 65535) decodes on the device (reference cpu.py:251 decodes every image
  Pillow accepts); a caller-chosen ``max_image_dim`` hands larger JPEGs to Pillow with
  identical views;
* ``UserAugSpec``: an image that probes fine but fails on the device raises the
  reference's ``torch.stack`` error when its zero tensor's shape differs (cpu.py:490-500).
"""

from __future__ import annotations

import io

import numpy as np
import pytest
import torch
from PIL import Image

from dataloader_amd.config import DINOAugConfig, DinoV2AugSpec, PipelineConfig
from dataloader_amd.engine import IngestEngine, pack_jpegs
from dataloader_amd.synthetic import encode_jpeg, textured_rgb
from oracle import cpu_ref

pytestmark = pytest.mark.gpu


class _ListSource:
    """A callable source with the reference's conventions (_batch_size, _resolution_src)."""

    def __init__(self, batches):
        self._it = iter(batches)
        self._batch_size = len(batches[0])
        self._resolution_src = None

    def __call__(self):
        return next(self._it)


def _cmyk(w, h, rng):
    b = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8), "CMYK").save(b, format="JPEG")
    return b.getvalue()


def _collect(it):
    outs = [{k: v.clone() for k, v in out[0].items()} for out in it]
    torch.cuda.synchronize()
    return outs


def test_backend_queue_depth_matches_serial(gpu_device):
    """gpu_queue = 6 -> 3 batches in flight + the prefetch thread; every view of every batch
    equals the gpu_queue = 1 pipeline's (same seed, same batch indices), with a progressive
    file (the device side route, the backend default since round 4) and a CMYK file (Pillow
    hand-over on the thread) in some batches."""
    from dataloader_amd.backend import MI355XBackend
    rng = np.random.default_rng(50)
    uniq = [encode_jpeg(textured_rgb(300 + 12 * s, 220 + 6 * s, rng)) for s in range(6)]
    prog = encode_jpeg(textured_rgb(256, 192, rng), progressive=True)
    cmyk = _cmyk(120, 90, rng)
    B, nb = 12, 7
    batches = [[uniq[(k * 5 + i) % 6] for i in range(B)] for k in range(nb)]
    batches[1][3] = prog
    batches[4][0] = cmyk
    batches[4][7] = prog
    spec = DinoV2AugSpec(aug_cfg=DINOAugConfig())
    be = MI355XBackend(host_workers=2)

    def run(gpu_queue):
        pipe = be.build_pipeline(_ListSource(batches), spec, PipelineConfig(gpu_queue=gpu_queue, seed=3), None)
        assert pipe.depth == min(gpu_queue, 3) and pipe.prefetch_ahead == 1
        outs = _collect(be.build_pipeline_iterator(pipe, spec, spec.output_map, B))
        st = pipe.flush_stats()
        pipe.close()
        return outs, st

    (ref, st1), (got, st3) = run(1), run(6)
    assert len(ref) == len(got) == nb
    assert st1["host_decoded"] == st3["host_decoded"] == 1 and set(st3["status"]) == {0}
    assert st1["side_decoded"] == st3["side_decoded"] == 2
    for k, (a, b) in enumerate(zip(ref, got)):
        for name in a:
            assert torch.equal(a[name], b[name]), (k, name)


def test_prefetch_thread_epochs_and_reset(gpu_device):
    """StopIteration raised on the prefetch thread ends the epoch after the in-flight batches;
    after the source's reset the next epoch runs again (DALI iterator reset, dali_node.py:84-91)."""
    from dataloader_amd.pipeline import MI355XAugPipeline, MI355XPipelineIterator
    rng = np.random.default_rng(51)
    uniq = [encode_jpeg(textured_rgb(160, 120, rng)) for _ in range(4)]
    B = 8

    class Epochs:
        _batch_size = B
        _resolution_src = None

        def __init__(self):
            self.k = 0

        def __call__(self):
            if self.k >= 3:
                raise StopIteration
            self.k += 1
            return [uniq[(self.k + i) % 4] for i in range(B)]

    src = Epochs()
    cfg = DINOAugConfig(global_crop_size=64, local_crop_size=32)
    pipe = MI355XAugPipeline(src, cfg, B, seed=1, depth=2)
    assert pipe.prefetch_ahead == 1
    it = MI355XPipelineIterator(pipe, [f"view_{i}" for i in range(cfg.n_views)], B)
    first = _collect(it)
    assert len(first) == 3
    with pytest.raises(StopIteration):
        next(it)
    src.k = 0
    it.reset()
    second = _collect(it)
    assert len(second) == 3
    pipe.close()


def _check_pipeline_views(pipe, jpegs, out, nv):
    """The views of the pipeline's last batch against the oracle: bit-exact except blur, which
    may differ by one uint8 level on <= 0.5 % of a view's values."""
    from tests.test_gpu_parity import _check_views
    recs = pipe.last_params()
    views = [out[f"view_{v}"] for v in range(nv)]
    dt = views[0].dtype
    cfg = pipe._aug_cfg
    _check_views(jpegs, views, recs, nv, dt, cfg.mean, cfg.std)


def test_wide_and_tall_jpegs_on_device_and_over_a_limit(gpu_device):
    """VERDICT r2 #7 / ADVICE r2: 9000 x 400, 300 x 9001 and 20000 x 64 JPEGs decode on the
    device bit-exact with Pillow, and their views match the oracle; with max_image_dim=4096 the
    same JPEGs are handed to Pillow and give identical views (no zero fill anywhere)."""
    from dataloader_amd.pipeline import MI355XAugPipeline
    rng = np.random.default_rng(52)
    jpegs = [encode_jpeg(textured_rgb(9000, 400, rng)), encode_jpeg(textured_rgb(300, 9001, rng)),
             encode_jpeg(textured_rgb(20000, 64, rng)), encode_jpeg(textured_rgb(640, 480, rng))]
    from dataloader_amd import fallback
    eng = IngestEngine(gpu_device, max_batch=len(jpegs), max_views=10, max_crop_size=224)
    buf, off = pack_jpegs(jpegs, pin=False)
    pinfo, ws, _ = fallback.probe(buf.data_ptr(), off.numpy(), len(jpegs), 0)
    assert (pinfo[:, 0] == 0).all(), pinfo  # no side limit by default
    eng.reserve(ws, 0)  # the bare engine's default workspace holds ~1 of these; the pipeline probes + reserves
    info = eng.decode(buf.to(gpu_device), off.to(gpu_device), len(jpegs)).cpu().numpy()
    assert (info[:, 0] == 0).all(), info
    for i, j in enumerate(jpegs):
        ref = np.asarray(cpu_ref.decode_rgb(j))
        got = eng.copy_rgb(i, ref.shape[1], ref.shape[0]).cpu().numpy()
        np.testing.assert_array_equal(got, ref, err_msg=str(i))
    eng.close()

    cfg = DINOAugConfig()
    outs = []
    for limit in (0, 4096):
        pipe = MI355XAugPipeline(lambda: jpegs, cfg, len(jpegs), seed=21, max_image_dim=limit, host_workers=2)
        out = {k: v.clone() for k, v in pipe.run_one_batch().items()}
        torch.cuda.synchronize()
        st = pipe.flush_stats()
        assert set(st["status"]) == {0}
        assert st["host_decoded"] == (0 if limit == 0 else 3)
        if limit == 0:
            _check_pipeline_views(pipe, jpegs, out, cfg.n_views)
        outs.append(out)
        pipe.close()
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_user_aug_device_failure_raises_like_the_stack(gpu_device):
    """a JPEG whose header probes fine but whose entropy data is cut (Pillow
    raises at convert) is the reference's (ds, ds) zero tensor; next to (ow, oh) != (ds, ds)
    views its torch.stack raises, so does the device pipeline.  With square images the
    batch returns and the failure is accounted asynchronously."""
    from dataloader_amd.backend import MI355XBackend
    from dataloader_amd.config import UserAugSpec
    rng = np.random.default_rng(53)
    good = encode_jpeg(textured_rgb(640, 480, rng))
    cut = good[: len(good) // 2]
    assert cpu_ref.decode_rgb(cut) is None
    spec = UserAugSpec(aug_fn=lambda x: {"a": x}, _output_map=["a"], decode_size=64, warn_not_dali=False)
    be = MI355XBackend()
    pipe = be.build_pipeline(_ListSource([[good, cut]]), spec, PipelineConfig(output_dtype="fp32"), None)
    with pytest.raises(RuntimeError, match="equal size"):
        next(be.build_pipeline_iterator(pipe, spec, spec.output_map, 2))
    pipe.close()
    sq = encode_jpeg(textured_rgb(200, 200, rng))
    sq_cut = sq[: len(sq) // 2]
    pipe = be.build_pipeline(_ListSource([[sq, sq_cut]]), spec, PipelineConfig(output_dtype="fp32"), None)
    out = next(be.build_pipeline_iterator(pipe, spec, spec.output_map, 2))[0]["a"].cpu()
    assert torch.count_nonzero(out[1]) == 0 and torch.count_nonzero(out[0]) > 0
    st = pipe.flush_stats()
    assert st["images"] == 2 and st["status"][0] == 1 and sum(v for k, v in st["status"].items() if k < 0) == 1
    pipe.close()


def test_reserve_is_stream_ordered_with_batches_in_flight(gpu_device):
    """dino_reserve grows a slot's workspaces on the slot's own stream while the other
    slots' batches are still running (no device-wide synchronisation): a batch of large
    images after small ones decodes and augments bit-identically to a fresh pipeline."""
    from dataloader_amd.pipeline import MI355XAugPipeline
    rng = np.random.default_rng(54)
    small = [encode_jpeg(textured_rgb(96, 64, rng)) for _ in range(4)]
    big = [encode_jpeg(textured_rgb(1600, 1200, rng)) for _ in range(4)]
    cfg = DINOAugConfig()
    seq = [small, small, big, small, big]

    def run(batches, ws):
        src = iter(batches)
        pipe = MI355XAugPipeline(lambda: next(src), cfg, 4, seed=8, depth=3, workspace_bytes=ws)
        outs = []
        for _ in batches:
            outs.append({k: v.clone() for k, v in pipe.run_one_batch().items()})
        torch.cuda.synchronize()
        st = pipe.flush_stats()
        pipe.close()
        return outs, st

    got, st = run(seq, 1 << 20)  # 1 MiB: every big batch must grow its slot's workspace
    assert st["reserves"] >= 2 and set(st["status"]) == {0}
    ref, _ = run(seq, 4 * (64 << 20))
    for a, b in zip(ref, got):
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_shard_spans_feed_dma_matches_packed_feed(gpu_device, tmp_path):
    """The native shard feed (C++ threads pack + probe into pinned slots, dino_feed_copy) and
    the /dev/shm feed handed over where it lies (page-locked shard ranges DMA'd to HBM, tar
    headers and sidecars included, decoded through dino_run_batch_spans) gives every view
    bit-identical to the packed feed (dino_gather into pinned staging), across shard
    boundaries and with a CMYK sample (a Pillow hand-over: that batch takes the packing path)."""
    import io as _io
    import json
    import tarfile

    from dataloader_amd.backend import MI355XBackend
    from dataloader_amd.tario import ShardBatchFeeder, ShmShardCache
    rng = np.random.default_rng(55)
    uniq = [encode_jpeg(textured_rgb(200 + 8 * s, 150 + 4 * s, rng)) for s in range(5)]
    samples = [uniq[i % 5] for i in range(60)]
    samples[23] = _cmyk(96, 64, rng)
    shards = []
    for s0 in range(0, 60, 25):  # 25, 25, 10 samples: batches of 8 straddle shards
        buf = _io.BytesIO()
        with tarfile.open(fileobj=buf, mode="w") as tf:
            for i in range(s0, min(60, s0 + 25)):
                for name, data in ((f"sample_{i:06d}.jpg", samples[i]), (f"sample_{i:06d}.json", json.dumps({"i": i}).encode())):
                    ti = tarfile.TarInfo(name)
                    ti.size = len(data)
                    tf.addfile(ti, _io.BytesIO(data))
        shards.append(buf.getvalue())
    cache = ShmShardCache(job_id="spans_gpu", base_dir=tmp_path)
    paths = [f"/d/shard-{k}.tar" for k in range(len(shards))]
    for p, t in zip(paths, shards):
        cache.put(p, t)
    spec = DinoV2AugSpec(aug_cfg=DINOAugConfig(global_crop_size=96, local_crop_size=48))
    be = MI355XBackend(host_workers=2)

    def run(register):
        feeder = ShardBatchFeeder(cache, paths, 8, nthreads=2, register=register)
        pipe = be.build_pipeline(feeder, spec, PipelineConfig(gpu_queue=6, seed=5), None)
        outs = _collect(be.build_pipeline_iterator(pipe, spec, spec.output_map, 8))
        st = pipe.flush_stats()
        pipe.close()
        feeder.close()
        assert feeder.register_error is None and not feeder._reg, (feeder.register_error, feeder._reg)
        return outs, st

    def run_native():
        from dataloader_amd.tario import NativeShardFeed
        feed = NativeShardFeed(cache, paths, 8, nthreads=3, slots=5)
        pipe = be.build_pipeline(feed, spec, PipelineConfig(gpu_queue=6, seed=5), None)
        outs = _collect(be.build_pipeline_iterator(pipe, spec, spec.output_map, 8))
        st = pipe.flush_stats()
        pipe.close()
        assert feed.stats()["batches"] >= 7
        feed.close()
        return outs, st

    (ref, st0), (got, st1), (nat, st2) = run(False), run(True), run_native()
    assert len(ref) == len(got) == len(nat) == 7
    assert st0["host_decoded"] == st1["host_decoded"] == st2["host_decoded"] == 1
    assert set(st1["status"]) == set(st2["status"]) == {0}
    for k, (a, b, c) in enumerate(zip(ref, got, nat)):
        for name in a:
            assert torch.equal(a[name], b[name]), (k, name)
            assert torch.equal(a[name], c[name]), (k, name, "native feed")
    cache.close(remove=True)


def test_shard_spans_from_a_page_locked_copy(gpu_device, tmp_path):
    """A feeder whose runtime does not register mappings (``page_lock`` "copy", what a refused
    hipHostRegister switches to): every batch is page-locked and lies outside the mapping, its
    ranges DMA'd to HBM and cut at offsets/lens are the shard's images across shard boundaries
    and a second epoch, and a shard's copy is freed once it is consumed and its batches have
    retired."""
    import ctypes
    import io as _io
    import tarfile

    from dataloader_amd import _lib
    from dataloader_amd.tario import ShardBatchFeeder, ShmShardCache
    rng = np.random.default_rng(57)
    samples = [rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes() for n in rng.integers(700, 5000, size=13)]
    shards = []
    for s0 in (0, 5, 10):  # 5, 5, 3 samples: batches of 4 straddle shards
        buf = _io.BytesIO()
        with tarfile.open(fileobj=buf, mode="w") as tf:
            for i in range(s0, min(13, s0 + 5)):
                ti = tarfile.TarInfo(f"sample_{i:06d}.jpg")
                ti.size = len(samples[i])
                tf.addfile(ti, _io.BytesIO(samples[i]))
        shards.append(buf.getvalue())
    cache = ShmShardCache(job_id="spans_copy", base_dir=tmp_path)
    paths = [f"/d/shard-{k}.tar" for k in range(len(shards))]
    for p, t in zip(paths, shards):
        cache.put(p, t)
    maps = [cache.get_array(p) for p in paths]
    feeder = ShardBatchFeeder(cache, paths, 4, nthreads=2, register=True)
    feeder.page_lock = "copy"
    lib = _lib.load()
    stream = torch.cuda.current_stream(gpu_device)
    for _epoch in range(2):
        got = []
        while True:
            try:
                bs = feeder.next_batch_spans()
            except StopIteration:
                break
            assert bs.registered
            for addr, n in bs.parts:
                assert not any(m.ctypes.data <= addr < m.ctypes.data + m.nbytes for m in maps)
            d = torch.empty(int(bs.offsets[-1]), dtype=torch.uint8, device=gpu_device)
            pos = 0
            for addr, n in bs.parts:
                _lib.check(lib.dino_copy_h2d(ctypes.c_void_p(d.data_ptr() + pos), ctypes.c_void_p(addr), n,
                                             ctypes.c_void_p(stream.cuda_stream)), "dino_copy_h2d")
                pos += n
            ev = torch.cuda.Event()
            ev.record(stream)
            feeder.retire(bs, ev)
            flat = d.cpu().numpy().tobytes()
            got += [flat[bs.offsets[i]:bs.offsets[i] + bs.lens[i]] for i in range(4)]
        assert got == samples[:12]
        assert 0 not in feeder._reg, feeder._reg  # consumed, retired and copied long ago
        feeder.reset()
    feeder.close()
    assert feeder.page_lock == "copy" and feeder.register_error is None and not feeder._reg
    cache.close(remove=True)


def test_pack_jpegs_packs_pageable_when_no_page_locked_buffer_is_granted(gpu_device, monkeypatch):
    """A host that refuses the page-locked buffer (a capped virtual machine, a very large set):
    pack_jpegs says so in a warning and packs the same bytes and offsets into pageable memory;
    an allocation that fails without pinning still raises."""
    rng = np.random.default_rng(58)
    jpegs = [rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes() for n in (1, 700, 33)]
    ref, ref_off = pack_jpegs(jpegs, pin=True)
    assert ref.is_pinned()
    real = torch.empty

    def refusing(*a, **kw):
        if kw.get("pin_memory"):
            raise RuntimeError("HIP error: out of memory")  # torch.AcceleratorError is a RuntimeError
        return real(*a, **kw)

    monkeypatch.setattr(torch, "empty", refusing)
    with pytest.warns(RuntimeWarning, match="pageable"):
        got, off = pack_jpegs(jpegs, pin=True)
    assert not got.is_pinned() and torch.equal(got[:734], ref[:734]) and torch.equal(off, ref_off)
    assert torch.equal(got.to(gpu_device)[:734].cpu(), ref[:734])

    def failing(*a, **kw):
        raise RuntimeError("no memory at all")

    monkeypatch.setattr(torch, "empty", failing)
    with pytest.raises(RuntimeError, match="no memory at all"):
        pack_jpegs(jpegs, pin=False)


def test_output_views_reused_only_after_the_caller_drops_them(gpu_device):
    """A slot refills its previous output tensors only when the caller no longer references
    them (DALI's iterator contract); batches the caller keeps are never overwritten."""
    from dataloader_amd.pipeline import MI355XAugPipeline, MI355XPipelineIterator
    rng = np.random.default_rng(56)
    uniq = [encode_jpeg(textured_rgb(160, 120, rng)) for _ in range(6)]
    B, nb = 4, 9
    batches = [[uniq[(k + i) % 6] for i in range(B)] for k in range(nb)]
    cfg = DINOAugConfig(global_crop_size=64, local_crop_size=32)

    def run(keep):
        src = _ListSource(batches)
        pipe = MI355XAugPipeline(src, cfg, B, seed=4, depth=3)
        it = MI355XPipelineIterator(pipe, [f"view_{i}" for i in range(cfg.n_views)], B)
        kept, snaps, ptrs = [], [], []
        for out in it:
            d = out[0]
            torch.cuda.synchronize()
            snaps.append({k: v.clone() for k, v in d.items()})
            ptrs.append(d["view_0"].data_ptr())
            if keep:
                kept.append(d)
            del out, d
        torch.cuda.synchronize()
        pipe.close()
        return kept, snaps, ptrs

    kept, snaps, ptrs_keep = run(True)
    for d, s in zip(kept, snaps):
        for k in d:
            assert torch.equal(d[k], s[k]), k          # nothing the caller holds was refilled
    assert len(set(ptrs_keep)) == nb
    _, snaps2, ptrs_drop = run(False)
    assert len(set(ptrs_drop)) < nb                    # dropped outputs are refilled in place
    for a, b in zip(snaps, snaps2):
        for k in a:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("side_decoder", ["wave", "lanes"])
def test_side_route_matches_in_batch_device_route(gpu_device, side_decoder, monkeypatch):
    """multiscan_route="side": progressive / multi-scan images decoded on the device ahead of
    their batch (progside.py) give every view bit-identical to the in-batch k_prog route
    ("device"), with a CMYK file (Pillow hand-over) and a cut progressive file (undecodable:
    it stays in its batch and comes back zero-filled, as the reference's) in the mix.  The side
    contexts run either decoder (round 6: the lane decoder is the side plan's choice at the
    default look-ahead; the in-batch route keeps the wave decoder)."""
    monkeypatch.setenv("DINO_SIDE_DECODER", side_decoder)
    monkeypatch.setenv("DINO_SIDE_LANE_MIN", "1")  # this test's pools are a few images
    from dataloader_amd.pipeline import MI355XAugPipeline, MI355XPipelineIterator
    rng = np.random.default_rng(57)
    uniq = [encode_jpeg(textured_rgb(240 + 8 * s, 180 + 4 * s, rng)) for s in range(5)]
    progs = [encode_jpeg(textured_rgb(200 + 16 * s, 150 + 8 * s, rng), progressive=True) for s in range(4)]
    cut = progs[0][: len(progs[0]) * 2 // 3]
    B, nb = 8, 9
    batches = [[uniq[(k + i) % 5] for i in range(B)] for k in range(nb)]
    for k in range(nb):
        batches[k][k % B] = progs[k % 4]
        if k % 3 == 0:
            batches[k][(k + 3) % B] = progs[(k + 1) % 4]
    batches[2][5] = _cmyk(100, 80, rng)
    batches[5][6] = cut
    cfg = DINOAugConfig(global_crop_size=96, local_crop_size=48)

    side_lane_launches = [0]

    def run(route):
        src = _ListSource(batches)
        pipe = MI355XAugPipeline(src, cfg, B, seed=9, depth=3, multiscan_route=route, host_workers=2, side_ahead=4)
        it = MI355XPipelineIterator(pipe, [f"view_{i}" for i in range(cfg.n_views)], B)
        outs = _collect(it)
        st = pipe.flush_stats()
        if pipe._side is not None:
            side_lane_launches[0] = pipe._side.lane_launches
        pipe.close()
        return outs, st

    (ref, st0), (got, st1) = run("device"), run("side")
    assert len(ref) == len(got) == nb
    assert st1.get("side_lanes") == (side_decoder == "lanes"), st1
    assert (side_lane_launches[0] > 0) == (side_decoder == "lanes")
    assert st1["side_decoded"] == nb + 3 and st0["side_decoded"] == 0, (st0, st1)  # the cut file fails on the side too
    assert st0["status"] == st1["status"] and st0["host_decoded"] == st1["host_decoded"] == 1
    for k, (a, b) in enumerate(zip(ref, got)):
        for name in a:
            assert torch.equal(a[name], b[name]), (k, name)

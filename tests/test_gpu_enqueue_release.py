"""A batch whose launch fails hands back what it held, exactly once, and the pipeline goes on.

``MI355XAugPipeline._enqueue_prepared`` owns a prepared batch's host resources from the pull
to the launch: its pinned staging goes back to the ring, its page-locked shard ranges are
retired to the feed.  Here ``_launch`` is replaced by a function that raises a plain Python
exception (no kernel runs), so the batch fails after its uploads were enqueued; afterwards
every staging of the ring can be acquired again, the feed saw one ``retire`` for the batch,
and the next batch gives the views of a fresh pipeline at the same (seed, batch index).

The pipelines run with ``prefetch=0``: the host half then runs inline, so no prefetch thread
holds a staging (for a batch packed ahead) while the ring is counted.
"""

from __future__ import annotations

import io
import tarfile

import numpy as np
import pytest
import torch

from dataloader_amd.config import DINOAugConfig
from dataloader_amd.pipeline import MI355XAugPipeline
from tests import jpeg_writer as jw
from tests.test_tario_cpu import _add

pytestmark = pytest.mark.gpu

B, SEED = 2, 11
CFG = DINOAugConfig(global_crop_size=32, local_crop_size=16, n_local_crops=2)


def _baseline(w: int, h: int, seed: int) -> bytes:
    img = np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    return jw.encode(img, [jw.scan((0, 1, 2))])


@pytest.fixture(scope="module")
def batches():
    """Two batches of the two JPEGs; the second one is what runs after the failed launch."""
    a, b = _baseline(16, 16, 1), _baseline(24, 16, 2)
    return [[a, b], [b, a]]


def _pipe(source):
    return MI355XAugPipeline(source, CFG, B, seed=SEED, depth=2, prefetch=0, host_workers=1)


@pytest.fixture(scope="module")
def fresh_views(gpu_device, batches):
    """The second batch as the first batch (index 0) of a fresh pipeline with the same seed."""
    pipe = _pipe(lambda: batches[1])
    try:
        out = {k: v.clone() for k, v in pipe.run_one_batch().items()}
        torch.cuda.synchronize()
        assert set(pipe.flush_stats()["status"]) == {0}
    finally:
        pipe.close()
    return out


def _ring_is_whole(pipe) -> None:
    """Every staging of the ring can be acquired, none of them twice, without waiting."""
    ring = pipe._ring
    assert not any(st.busy for st in ring._bufs)  # (a busy one would make acquire wait for good)
    held = [ring.acquire() for _ in ring._bufs]
    assert len({id(st) for st in held}) == len(ring._bufs)
    for st in held:
        ring.release(st, None)


def _fail_then_recover(pipe, fresh_views, after_failure=lambda: None) -> None:
    launch = pipe._launch

    def boom(*args, **kwargs):
        raise RuntimeError("boom")

    pipe._launch = boom
    with pytest.raises(RuntimeError, match="boom"):
        pipe.run_one_batch()
    pipe._launch = launch
    after_failure()
    _ring_is_whole(pipe)
    out = pipe.run_one_batch()
    torch.cuda.synchronize()
    assert set(out) == set(fresh_views)
    for k, v in fresh_views.items():
        assert torch.equal(out[k], v), k
    _ring_is_whole(pipe)
    st = pipe.flush_stats()
    assert st["batches"] == 1 and set(st["status"]) == {0}


def test_failed_launch_returns_the_staging_and_the_next_batch_is_right(gpu_device, batches, fresh_views):
    src = iter(batches)
    pipe = _pipe(lambda: next(src))
    try:
        _fail_then_recover(pipe, fresh_views)
    finally:
        pipe.close()


def test_failed_launch_retires_the_shard_ranges_once(gpu_device, batches, fresh_views, tmp_path):
    """The same on a feed that hands batches over where they lie: the failed batch's shard
    ranges are retired once (by the failed launch when they were page-locked and DMA'd as they
    lie, else by the pack that copied them out), and the next batch's once."""
    from dataloader_amd.tario import ShardBatchFeeder, ShmShardCache
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w") as tf:
        for i, j in enumerate(batches[0] + batches[1]):
            _add(tf, f"sample_{i:06d}.jpg", j)
    cache = ShmShardCache(job_id="enqueue_release", base_dir=tmp_path)
    cache.put("/d/shard-0.tar", buf.getvalue())
    feeder = ShardBatchFeeder(cache, ["/d/shard-0.tar"], B, nthreads=1, register=True)
    retired = []
    retire = feeder.retire

    def counting(batch, event=None):
        retired.append(batch)
        return retire(batch, event)

    feeder.retire = counting
    pipe = _pipe(feeder)

    def retired_once():
        assert len(retired) == 1, f"the failed batch was retired {len(retired)} times"

    try:
        _fail_then_recover(pipe, fresh_views, after_failure=retired_once)
        assert len(retired) == 2 and retired[0] is not retired[1]
    finally:
        pipe.close()
        feeder.close()
        cache.close(remove=True)
    assert not feeder._reg, feeder._reg

"""The host half's buffers and its worker threads: the pinned staging ring, the prepared-batch
record that travels from the pull to the launch, and the prefetcher that fills both ahead of
the launch thread.  The prefetcher takes its pipeline as a duck-typed object (``_pull_raw``,
``_pack_raw``, ``_prepare_next``, ``_stage_early``, ``_drop``; ``_spans_feed``, ``_native``).
"""

from __future__ import annotations

import os
import queue
import threading

import numpy as np
import torch


class _Staging:
    """A pinned host buffer the batch's JPEG bytes (+ int64 offsets + raw mask) are packed
    into before the H2D copy.  Owned by the host half while it is being filled and until the
    launch that copies it out has retired (``released`` event)."""

    def __init__(self):
        self.buf: torch.Tensor | None = None
        self.off: torch.Tensor | None = None
        self.lens: torch.Tensor | None = None
        self.mask: torch.Tensor | None = None
        self.released: torch.cuda.Event | None = None
        self.busy = False

    def fit(self, nbytes: int, n: int) -> None:
        if nbytes > 0 and (self.buf is None or self.buf.numel() < nbytes):
            self.buf = torch.empty(max(nbytes, 1) * 5 // 4 + 64, dtype=torch.uint8, pin_memory=True)
        if self.off is None or self.off.numel() < n + 1:
            self.off = torch.empty(n + 1, dtype=torch.int64, pin_memory=True)
            self.lens = torch.empty(n, dtype=torch.int64, pin_memory=True)
            self.mask = torch.empty(n, dtype=torch.uint8, pin_memory=True)


class _StagingRing:
    """Round-robin staging buffers shared by the host half (fills) and the launch (frees)."""

    def __init__(self, n: int):
        self._bufs = [_Staging() for _ in range(max(2, n))]
        self._next = 0
        self._cv = threading.Condition()
        self._closed = False

    def close(self) -> None:
        with self._cv:
            self._closed = True
            self._cv.notify_all()

    def acquire(self) -> _Staging:
        with self._cv:
            st = self._bufs[self._next]
            self._next = (self._next + 1) % len(self._bufs)
            while st.busy and not self._closed:  # still waiting to be launched (rare: the ring is sized for it)
                self._cv.wait()
            if self._closed:
                raise RuntimeError("MI355XAugPipeline closed")
            st.busy = True
        if st.released is not None:
            st.released.synchronize()  # the H2D copy of its previous batch retired
            st.released = None
        return st

    def release(self, st: _Staging, event: torch.cuda.Event | None) -> None:
        with self._cv:
            st.released = event
            st.busy = False
            self._cv.notify_all()


class _Prepared:
    """A pulled, packed and probed host batch whose host-routed images are decoding in the pool."""

    def __init__(self, staging: _Staging, jpegs, offsets: np.ndarray, info: np.ndarray, ws: int, aws: int,
                 sizes: tuple[int, int], futures: dict, spans=None, feed=None):
        self.staging = staging        # None: no Python staging (native feed slot, or not yet needed)
        self.spans = spans            # tario.BatchSpans: the batch stays in its page-locked shard ranges
        self.feed = feed              # tario.FeedBatch: the batch is packed in a native feed slot
        self.side = None              # progside.SideJob: its coefficient-buffer images, decoded ahead
        self.room: dict = {}          # batch index -> offset of room for its container in the HBM copy
        self.side_submitted = False   # _side_submit ran (on the prefetch thread, or at the pull)
        self.jpegs = jpegs            # the source's list (None for the native feed)
        self.offsets = offsets
        self.info = info
        self.ws, self.aws = ws, aws
        self.sizes = sizes            # (G, L) the augment-workspace bound was computed for
        self.futures = futures
        # side look-ahead: the batch's input copied to HBM when it entered the look-ahead (its
        # pinned staging / feed slot / shard ranges are free again); ready after `copied`
        self.dev = None               # (d_bytes, d_offsets, d_lens or None)
        self.lens = None              # host image lengths of a spans batch staged on the device
        self.copied: torch.cuda.Event | None = None


_END = object()


RAW_AHEAD = 2  # pulled, not yet packed batches the prefetcher's puller thread holds (list sources)
# pack threads of a list source's prefetcher (DINO_PACK_THREADS): two measured no faster than
# one on c2_prog (the packs then contend for the job's CPU share, profiles/r06_side_plan/r6x)
PACK_THREADS = 1


class _Prefetcher:
    """The host half of the pipeline on worker threads (DALI's prefetch queue, reference
    pipeline.py:317 ``prefetch_queue_depth``): pull the next batch from the source, pack it
    into pinned staging (``dino_gather``), ``dino_probe`` it and submit its Pillow
    hand-overs, up to ``ahead`` batches ahead of the launches.  The GIL is released inside
    the native calls, so this overlaps the launch thread and the GPU.

    For a source that hands over JPEG lists (the reference's ``_ReaderAdapter``) the pull
    runs on a thread of its own, up to ``RAW_AHEAD`` batches ahead, and ``PACK_THREADS``
    threads pack the pulled batches: the source's Python call and the native pack overlap
    instead of adding up (c2_prog: ~0.8 ms pull + 1.2-3 ms pack per batch).
    Batches are handed out in the source's order (sequence numbers, a reorder buffer of at
    most ``ahead`` batches); the source's end and its errors arrive in place."""

    def __init__(self, pipe: "MI355XAugPipeline", ahead: int):
        self._pipe = pipe
        self._ahead = max(1, ahead)
        self._stop = threading.Event()
        self.finished = False       # the source raised StopIteration (the END marker is queued)
        self._cv = threading.Condition()
        self._out: dict = {}        # sequence number -> _Prepared, _END or an exception
        self._next = 0              # sequence number get() hands out next
        self._raw: queue.Queue | None = None
        self._threads: list[threading.Thread] = []
        if not pipe._spans_feed and not pipe._native:
            self._raw = queue.Queue(maxsize=RAW_AHEAD)
            n = max(1, int(os.environ.get("DINO_PACK_THREADS", PACK_THREADS)))
            self._threads.append(threading.Thread(target=self._pull_loop, name="dino-pull", daemon=True))
            self._threads += [threading.Thread(target=self._pack_loop, name=f"dino-prefetch-{k}", daemon=True)
                              for k in range(n)]
        else:
            self._threads.append(threading.Thread(target=self._run, name="dino-prefetch", daemon=True))
        for t in self._threads:
            t.start()

    # ---- producers
    def _emit(self, seq: int, item) -> bool:
        """Place item `seq` in the reorder buffer once it is within `ahead` of the next hand-out."""
        with self._cv:
            while seq - self._next >= self._ahead and not self._stop.is_set():
                self._cv.wait(0.1)
            if self._stop.is_set():
                return False
            self._out[seq] = item
            self._cv.notify_all()
            return True

    def _settle(self, seq: int, item) -> bool:
        """Emit a prepared batch, or drop it if the prefetcher is closing."""
        if isinstance(item, _Prepared) and not self._emit(seq, item):
            self._pipe._drop(item)
            return False
        return isinstance(item, _Prepared) or self._emit(seq, item)

    def _run(self) -> None:  # one thread pulls and packs (spans / native sources)
        seq = 0
        try:
            while not self._stop.is_set():
                pb = self._pipe._prepare_next()
                self._pipe._stage_early(pb)
                if not self._settle(seq, pb):
                    return
                seq += 1
        except StopIteration:
            self.finished = True
            self._emit(seq, _END)
        except BaseException as e:  # noqa: BLE001 - handed to the launch thread
            self._emit(seq, e)

    def _put_raw(self, item) -> bool:
        while not self._stop.is_set():
            try:
                self._raw.put(item, timeout=0.1)
                return True
            except queue.Full:
                continue
        return False

    def _pull_loop(self) -> None:
        seq = 0
        try:
            while not self._stop.is_set():
                if not self._put_raw((seq, self._pipe._pull_raw())):
                    return
                seq += 1
        except StopIteration:
            self._put_raw((seq, _END))
        except BaseException as e:  # noqa: BLE001 - handed to a pack thread, then the launch thread
            self._put_raw((seq, e))

    def _pack_loop(self) -> None:
        while not self._stop.is_set():
            try:
                seq, raw = self._raw.get(timeout=0.1)
            except queue.Empty:
                continue
            if raw is _END or isinstance(raw, BaseException):
                if raw is _END:
                    self.finished = True
                self._put_raw((seq, raw))  # the other pack threads see the end too
                self._emit(seq, raw)
                return
            try:
                pb = self._pipe._pack_raw(raw)
                self._pipe._stage_early(pb)
            except BaseException as e:  # noqa: BLE001 - handed to the launch thread in place
                self._emit(seq, e)
                continue
            if not self._settle(seq, pb):
                return

    # ---- consumer
    def get(self, block: bool = True) -> _Prepared | None:
        with self._cv:
            while self._next not in self._out:
                if not block or self._stop.is_set():
                    return None
                self._cv.wait(0.1)
            item = self._out[self._next]
            if item is not _END and not isinstance(item, BaseException):
                del self._out[self._next]
                self._next += 1
                self._cv.notify_all()
        if item is _END:
            raise StopIteration
        if isinstance(item, BaseException):
            raise item
        return item

    def close(self) -> None:
        self._stop.set()
        with self._cv:
            self._cv.notify_all()
        for t in self._threads:
            t.join(timeout=5.0)
        with self._cv:  # free staging of batches never launched
            items, self._out = list(self._out.values()), {}
        for item in items:
            if isinstance(item, _Prepared):
                self._pipe._drop(item)
        while self._raw is not None:
            try:
                self._raw.get_nowait()
            except queue.Empty:
                break

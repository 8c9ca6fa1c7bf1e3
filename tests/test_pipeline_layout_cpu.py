"""The host half's module layout: what moved out of ``pipeline.py`` (the role-stream registry to
``streams.py``, the staging ring and the prefetcher to ``staging.py``, the decode-only pipeline
to ``useraug.py``) is still importable from it as the same objects, ``streams.py`` stands on
its own, and the stream-set bookkeeping hands out the lowest free id.  No device is touched."""

from __future__ import annotations

import subprocess
import sys
from pathlib import Path

import pytest

from dataloader_amd import params, pipeline, staging, streams, useraug

ROOT = Path(__file__).resolve().parents[1]

MOVED = {
    streams: ["role_stream", "acquire_stream_set", "release_stream_set", "release_role_streams",
              "_RAW_ROLE_STREAMS", "_ROLE_STREAMS", "_LIVE"],
    staging: ["_Prefetcher", "_Prepared", "PACK_THREADS", "RAW_AHEAD"],
    useraug: ["resize_scratch_bound", "MI355XUserAugPipeline", "MI355XUserAugIterator"],
    params: ["make_aug_config"],
}


@pytest.mark.parametrize("module,name", [(m, n) for m, names in MOVED.items() for n in names],
                         ids=lambda v: v if isinstance(v, str) else v.__name__.rsplit(".", 1)[-1])
def test_pipeline_re_exports_the_same_objects(module, name):
    assert getattr(pipeline, name) is getattr(module, name)


def test_streams_imports_neither_the_pipeline_nor_the_side_decoder():
    code = ("import sys; import dataloader_amd.streams; "
            "print(sorted(m for m in sys.modules if m in ('dataloader_amd.pipeline', 'dataloader_amd.progside', "
            "'dataloader_amd.engine')))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == "[]", r.stdout


def test_progside_takes_its_streams_from_streams():
    text = (ROOT / "dataloader_amd" / "progside.py").read_text()
    assert "from .pipeline import" not in text
    assert "from .streams import role_stream" in text


def test_stream_sets_are_handed_out_lowest_free_first(monkeypatch):
    """``acquire_stream_set`` / ``release_stream_set`` on an explicit device index keep a set of
    ids per device (no device call).  The sets that pipelines of this process hold are put
    aside for the test."""
    monkeypatch.setitem(streams._SETS_BUSY, 0, set())
    monkeypatch.setitem(streams._SETS_BUSY, 1, set())
    assert streams.acquire_stream_set(0) == 0
    assert streams.acquire_stream_set(0) == 1
    streams.release_stream_set(0, 0)
    assert streams._SETS_BUSY[0] == {1}
    assert streams.acquire_stream_set(0) == 0
    assert streams.acquire_stream_set(0) == 2
    assert streams.acquire_stream_set(1) == 0  # each device counts on its own
    streams.release_stream_set(0, 7)           # releasing a set nobody holds changes nothing
    assert streams._SETS_BUSY[0] == {0, 1, 2} and streams._SETS_BUSY[1] == {0}

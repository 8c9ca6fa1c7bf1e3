"""``gif`` on the CPU: the host model (``dino_debug_gif_decode``, the text k_gifwalk, k_giflzw and
k_gif_rgb compile, the 64 lanes as a loop) against Pillow over tests/gif_cases.py, the probe, the
rows ``accept_gif`` writes."""

import ctypes

import numpy as np
import pytest

from dataloader_amd import _lib, fallback
from dataloader_amd.tario import spans_of
from tests import gif_cases as gc
from tests.png_cases import pillow_rgb

CASES = gc.cases()


def model_decode(b: bytes, max_dim: int = 0):
    """(info int32[8], layout int64[5], rgb or None) of the host model (include/dino_ingest.h)."""
    info, layout = np.zeros(8, np.int32), np.zeros(5, np.int64)
    rgb = np.zeros(1 << 17, np.uint8)
    buf = np.frombuffer(b, np.uint8)
    vp = ctypes.c_void_p
    _lib.check(_lib.load().dino_debug_gif_decode(buf.ctypes.data_as(vp), len(b), max_dim, rgb.ctypes.data_as(vp), rgb.size,
                                                 info.ctypes.data_as(vp), layout.ctypes.data_as(vp)), "dino_debug_gif_decode")
    w, h = int(info[1]), int(info[2])
    return info, layout, rgb[: w * h * 3].reshape(h, w, 3) if info[0] == 0 else None


@pytest.mark.parametrize("name,data,expect", CASES, ids=[c[0] for c in CASES])
def test_model_and_probe_match_pillow(name, data, expect):
    info, layout, rgb = model_decode(data)
    ptrs, lens, _keep = spans_of([data])
    form, ws = fallback.probe_gif(ptrs, lens)
    ref = pillow_rgb(data)
    if expect in ("declined", "none"):
        assert form[0, 0] == (expect == "declined") and ws[0] == 0 and info[3] == 0 and (ref is None or expect == "declined")
        return
    assert form[0, 0] == 2 and info[3] == 2 and ws[0] == layout[0] and 0 <= ws[0] - layout[1:].sum() < 256, (info, layout)
    if expect == "corrupt":
        assert ref is None and info[0] == -1, info
        return
    assert info[0] == 0 and tuple(form[0, 1:]) == ref.shape[1::-1], info
    assert np.array_equal(rgb, ref), int((rgb != ref).sum())


def test_accept_gif_rows_and_bytes():
    files = [c[1] for c in CASES] + [b"GIF88a" + bytes(20)]
    ptrs, lens, _keep = spans_of(files)
    info, ws0, _ = fallback.probe_spans(ptrs, lens, 0, None)
    assert (info[:, 0] == -1).all() and (info[:, 3] == -1).all() and ws0 == 0
    form, ws = fallback.probe_gif(ptrs, lens)
    mine = np.array([c[2] in ("dev", "corrupt") for c in CASES] + [False])
    none = np.array([c[2] == "none" for c in CASES] + [True])
    assert (form[:, 0] == np.where(mine, 2, np.where(none, 0, 1))).all()
    out, extra, _ = fallback.accept_gif(info, form, ws, "device")
    assert (out[mine, 0] == 0).all() and (out[mine, 3] == 1).all() and extra == int(ws[mine].sum()) > 0
    assert (out[~mine, 0] == np.where(none, -1, 1)[~mine]).all()
    host, extra_h, _ = fallback.accept_gif(info, form, ws, "host")
    assert (host[:, 0] == np.where(none, -1, 1)).all() and extra_h == 0
    off, _, _ = fallback.accept_gif(info, form, ws, "off")
    assert np.array_equal(off, info)
    small, _ = fallback.probe_gif(ptrs, lens, 100)  # a side above max_image_dim: Pillow's
    assert [int(f) for f, c in zip(small[:, 0], CASES) if c[0] in ("noise256_96x80", "flat_200x100")] == [2, 1]


def test_refuses_unknown_mode():
    from dataloader_amd.backend import MI355XBackend
    with pytest.raises(ValueError, match="gif"):
        fallback.check_gif("gpu")
    with pytest.raises(ValueError, match="gif"):
        MI355XBackend(gif="gpu")

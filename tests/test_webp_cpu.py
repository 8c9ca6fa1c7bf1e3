"""``webp`` on the CPU: the host model (``dino_debug_webp_decode``, the text k_vp8l and k_vp8l_inv
compile) against Pillow over tests/webp_cases.py, the probe, the rows ``accept_webp`` writes."""

import ctypes

import numpy as np
import pytest

from dataloader_amd import _lib, fallback
from dataloader_amd.tario import spans_of
from tests import webp_cases as wc
from tests.png_cases import pillow_rgb

CASES = wc.cases()
DAMAGED = wc.damaged()


def model_decode(b: bytes, max_dim: int = 0):
    """(info int32[10], layout int64[6], rgb or None) of the host model (include/dino_ingest.h)."""
    info, layout = np.zeros(10, np.int32), np.zeros(6, np.int64)
    rgb = np.zeros(1 << 20, np.uint8)
    buf = np.frombuffer(b, np.uint8)
    vp = ctypes.c_void_p
    _lib.check(_lib.load().dino_debug_webp_decode(buf.ctypes.data_as(vp), len(b), max_dim, rgb.ctypes.data_as(vp), rgb.size,
                                                  info.ctypes.data_as(vp), layout.ctypes.data_as(vp)), "dino_debug_webp_decode")
    w, h = int(info[1]), int(info[2])
    return info, layout, rgb[: w * h * 3].reshape(h, w, 3) if info[0] == 0 else None


@pytest.mark.parametrize("name,data,expect", CASES, ids=[c[0] for c in CASES])
def test_model_and_probe_match_pillow(name, data, expect):
    info, layout, rgb = model_decode(data)
    ptrs, lens, _keep = spans_of([data])
    form, ws = fallback.probe_webp(ptrs, lens)
    assert form[0, 0] == {"dev": 2, "declined": 1, "none": 0}[expect]
    if expect != "dev":
        assert info[3] == 0 and ws[0] == 0 and (expect == "declined" or pillow_rgb(data) is None)
        return
    ref = pillow_rgb(data)
    assert info[0] == 0 and tuple(form[0, 1:]) == ref.shape[1::-1] and 0 <= ws[0] - layout[1:5].sum() < 256 and ws[0] == layout[0], (info, layout)
    assert np.array_equal(rgb, ref), int((rgb != ref).sum())


def test_case_list_covers_every_feature():
    """The feature mask of the host decoder over the list: all four transforms, a colour cache,
    several groups, each bundling width, short and long distance codes."""
    feats = np.array([model_decode(c[1])[0][4:] for c in CASES if c[2] == "dev"])
    assert np.bitwise_or.reduce(feats[:, 0]) == 15
    assert (feats[:, 1] > 0).any() and (feats[:, 2] > 1).any()
    assert {1, 2, 3, 4} <= set(feats[:, 3].tolist())  # 8, 4, 2, 1 index bits a pixel
    assert feats[:, 4].any() and feats[:, 5].any()


@pytest.mark.parametrize("name,data", DAMAGED, ids=[c[0] for c in DAMAGED])
def test_damaged_payload_is_pillows(name, data):
    """Zeros (status -1, or declined to Pillow, which raises) where Pillow raises, its pixels where it does not."""
    info, _, rgb = model_decode(data)
    ref = pillow_rgb(data)
    if ref is None:
        assert info[0] != 0, info
    else:
        assert info[0] == 0 and np.array_equal(rgb, ref), info


def test_accept_webp_rows_and_bytes():
    files = [c[1] for c in CASES]
    ptrs, lens, _keep = spans_of(files)
    info, ws0, _ = fallback.probe_spans(ptrs, lens, 0, None)
    assert (info[:, 0] == -1).all() and (info[:, 3] == -1).all() and ws0 == 0
    form, ws = fallback.probe_webp(ptrs, lens)
    dev = np.array([c[2] == "dev" for c in CASES])
    out, extra, _ = fallback.accept_webp(info, form, ws, "device")
    assert (out[dev, 0] == 0).all() and (out[dev, 3] == 1).all() and extra == sum(int(model_decode(f)[1][0]) for f in files)
    assert out[~dev, 0].tolist() == [1, 1, 1, -1]
    host, extra_h, _ = fallback.accept_webp(info, form, ws, "host")
    assert host[:, 0].tolist() == [1] * (len(files) - 1) + [-1] and extra_h == 0
    off, _, _ = fallback.accept_webp(info, form, ws, "off")
    assert np.array_equal(off, info)
    small, _ = fallback.probe_webp(ptrs, lens, 100)  # a side above max_image_dim: Pillow's
    assert [int(f) for f, c in zip(small[:, 0], CASES) if c[0] in ("wide_131x5", "flat_70x130")] == [1, 1]


def test_constructor_refuses_unknown_mode():
    from dataloader_amd.backend import MI355XBackend
    with pytest.raises(ValueError, match="webp"):
        MI355XBackend(webp="gpu")

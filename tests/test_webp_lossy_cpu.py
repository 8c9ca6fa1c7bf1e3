"""``webp_forms`` on the CPU: the host model (``dino_debug_vp8_decode``, the text k_vp8_tok, k_vp8_rec
and k_vp8_rgb compile) against Pillow over tests/webp_lossy_cases.py, the probe, the option checks."""

import ctypes

import numpy as np
import pytest

from dataloader_amd import _lib, fallback
from dataloader_amd.tario import spans_of
from tests import webp_lossy_cases as wc
from tests.png_cases import pillow_rgb

CASES = wc.cases()
DAMAGED = wc.damaged()


def model_decode(b: bytes, max_dim: int = 0):
    """(info int32[12], layout int64[5], rgb or None) of the host model (include/dino_ingest.h)."""
    info, layout = np.zeros(12, np.int32), np.zeros(5, np.int64)
    rgb = np.zeros(1 << 16, np.uint8)
    buf = np.frombuffer(b, np.uint8)
    vp = ctypes.c_void_p
    _lib.check(_lib.load().dino_debug_vp8_decode(buf.ctypes.data_as(vp), len(b), max_dim, rgb.ctypes.data_as(vp), rgb.size,
                                                 info.ctypes.data_as(vp), layout.ctypes.data_as(vp)), "dino_debug_vp8_decode")
    w, h = int(info[1]), int(info[2])
    return info, layout, rgb[: w * h * 3].reshape(h, w, 3) if info[0] == 0 else None


@pytest.mark.parametrize("name,data,expect", CASES, ids=[c[0] for c in CASES])
def test_model_and_probe_match_pillow(name, data, expect):
    info, layout, rgb = model_decode(data)
    ptrs, lens, _keep = spans_of([data])
    form, ws = fallback.probe_webp_forms(ptrs, lens)
    assert fallback.probe_webp(ptrs, lens)[0][0, 0] == 1, "dino_probe_webp itself is unchanged"
    assert form[0, 0] == (expect == "dev")
    if expect != "dev":
        assert info[0] == -1 and info[3] == 0 and ws[0] == 0
        return
    ref = pillow_rgb(data)
    assert info[0] == 0 and tuple(form[0, 1:]) == ref.shape[1::-1] and ws[0] == layout[0] and layout[0] % 256 == 0, (info, layout)
    assert 0 <= layout[0] - layout[1:5].sum() < 256
    assert np.array_equal(rgb, ref), int((rgb != ref).sum())


def test_case_list_covers_every_branch():
    """The coverage record ORed over the sound cases: every 16x16, sub-block and chroma mode, the
    three filter types, the three hev thresholds, segments off and on, a skip, category 6."""
    cover = np.bitwise_or.reduce(np.array([model_decode(c[1])[0][4:] for c in CASES if c[2] == "dev"]))
    assert cover[0] == 15 and cover[1] == 1023 and cover[2] == 15, cover
    assert cover[3] == 7 and cover[4] == 7 and cover[5] == 3 and cover[6] == 1 and cover[7] & 8, cover


@pytest.mark.parametrize("name,data", DAMAGED, ids=[c[0] for c in DAMAGED])
def test_damaged_payload_is_pillows(name, data):
    """Status -1 where Pillow raises, its pixels bit for bit where it does not."""
    info, _, rgb = model_decode(data)
    ref = pillow_rgb(data)
    assert info[3] == 1, "the walk still verifies the file"
    if ref is None:
        assert info[0] == -1, info
    else:
        assert info[0] == 0 and np.array_equal(rgb, ref), info


def test_option_checks_and_accepted_rows():
    fallback.check_webp_forms("all", "device")
    for forms, webp in (("all", "host"), ("all", "off"), ("lossy", "device")):
        with pytest.raises(ValueError, match="webp_forms"):
            fallback.check_webp_forms(forms, webp)
    from dataloader_amd.backend import MI355XBackend
    with pytest.raises(ValueError, match="webp_forms"):
        MI355XBackend(webp="host", webp_forms="all")
    # a hand-made probe table: a JPEG, a lossless WebP taken, two WebPs handed over, one of them lossy
    info = np.array([[0, 8, 8, 0], [0, 5, 6, 1], [1, 0, 0, -1], [1, 0, 0, -1]], np.int32)
    form = np.array([[0, 0, 0], [0, 0, 0], [1, 50, 83, ], [0, 0, 0]], np.int32)
    out, ws, aws = fallback.accept_webp_forms(info, form, np.array([7, 7, 4096, 7]))
    assert out.tolist() == [[0, 8, 8, 0], [0, 5, 6, 1], [0, 50, 83, fallback.KIND_MULTISCAN], [1, 0, 0, -1]] and ws == 4096 and aws == 0

"""``png_forms="all"`` on the CPU: the host model (``dino_debug_png_forms_decode``) against Pillow
over tests/png_forms_cases.py, the forms probe against the model's layout, the routing."""

import ctypes

import numpy as np
import pytest

from dataloader_amd import _lib, fallback
from dataloader_amd.tario import spans_of
from tests import png_cases as pc
from tests import png_forms_cases as fc

CASES = fc.cases()


def model_decode(b: bytes, max_dim: int = 0):
    """(info = [status, width, height, form], layout int64[8], rgb or None) of the host model."""
    info, layout = np.zeros(4, np.int32), np.zeros(8, np.int64)
    w, h = (int.from_bytes(b[16:20], "big"), int.from_bytes(b[20:24], "big")) if len(b) > 24 else (0, 0)
    rgb = np.zeros(max(1, min(w * h * 3, 1 << 26)), np.uint8)
    buf = np.frombuffer(b, np.uint8)
    vp = ctypes.c_void_p
    _lib.check(_lib.load().dino_debug_png_forms_decode(buf.ctypes.data_as(vp), len(b), max_dim, rgb.ctypes.data_as(vp),
                                                       rgb.size, info.ctypes.data_as(vp), layout.ctypes.data_as(vp)),
               "dino_debug_png_forms_decode")
    return info, layout, rgb[: w * h * 3].reshape(h, w, 3) if info[0] == 0 and info[3] else None


@pytest.mark.parametrize("name,data,expect", CASES, ids=[c[0] for c in CASES])
def test_model_matches_pillow(name, data, expect):
    info, _, rgb = model_decode(data)
    ref = pc.pillow_rgb(data)
    if expect == "declined":
        assert info[3] == 0 and ref is None
    elif expect == "raise":
        assert info[3] == 1 and info[0] == -1 and ref is None, info
    else:
        assert info[3] == 1 and info[0] == 0 and ref is not None, info
        assert np.array_equal(rgb, ref), int((rgb != ref).sum())


def test_sixteen_bit_gray_rule_over_every_value():
    """Pillow's I;16 -> RGB is min(v, 255), not the high byte: the rule png_form_to_rgb follows."""
    ref = pc.pillow_rgb(dict((c[0], c[1]) for c in CASES)["gray16_every_value"])
    assert np.array_equal(ref[:, :, 0].reshape(-1), np.minimum(np.arange(65536), 255))


def test_probe_rows_and_workspace_against_the_model():
    files = [c[1] for c in CASES] + [pc.cases()[0][1], b"\xff\xd8\xff\xd9", b""]
    ptrs, lens, _keep = spans_of(files)
    form, ws = fallback.probe_png_forms(ptrs, lens)
    info, _, _ = fallback.probe_spans(ptrs, lens, 0)
    for i, b in enumerate(files):
        m, layout, _ = model_decode(b) if b else (np.zeros(4, np.int32), np.zeros(8, np.int64), None)
        assert form[i, 0] == int(m[3]), i
        assert ws[i] == layout[0] and layout[0] % 256 == 0, i
        if m[3]:  # the context-free probe keeps calling it declined; the layout holds what the kernels touch
            assert tuple(info[i]) == (-1, 0, 0, 5) and tuple(form[i, 1:]) == (m[1], m[2])
            assert layout[3] >= layout[6] + 64 and layout[2] >= 16 and layout[5] >= 3 * m[1] * m[2] + 16
    assert not form[len(CASES):, 0].any() and form[len(CASES) - 1, 0] == 0


def test_accept_png_forms_on_a_mixed_info_array():
    from dataloader_amd.config import DINOAugConfig
    from dataloader_amd.params import make_aug_config
    cfg = make_aug_config(DINOAugConfig(), 224, 96, 0)
    info = np.array([[0, 64, 48, 0], [-1, 0, 0, 5], [-1, 0, 0, 5], [-1, 30, 20, 4], [1, 0, 0, 5], [-1, 0, 0, -1]], np.int32)
    form = np.array([[0, 0, 0], [1, 9, 7], [0, 0, 0], [1, 5, 5], [1, 4, 3], [1, 2, 2]], np.int32)
    ws = np.array([0, 512, 0, 999, 256, 77], np.int64)
    for src in (info, fallback.accept_png(info, "device")):
        out, extra, aws = fallback.accept_png_forms(src, form, ws, cfg)
        assert out[1].tolist() == [0, 9, 7, 1] and out[4].tolist() == [0, 4, 3, 1] and extra == 768
        assert out[2, 3] == 5 and out[2, 0] == src[2, 0] and out[5].tolist() == [-1, 0, 0, -1]
        assert (out[[0, 3]] == np.asarray(src)[[0, 3]]).all()
        assert aws == fallback.augment_need(out[[1, 4]], cfg) > 0


def test_option_needs_png_device():
    from dataloader_amd.backend import MI355XBackend
    for kw in ({"png_forms": "all"}, {"png": "host", "png_forms": "all"}, {"png": "device", "png_forms": "some"}):
        with pytest.raises(ValueError):
            MI355XBackend(**kw)

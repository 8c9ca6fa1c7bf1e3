"""Four-component (Adobe CMYK / YCCK) JPEGs without a GPU: the colour arithmetic, the host
model of the device decode, the probes' kind 3 and the routing — all against Pillow on the
same bytes (``tests/cmyk_cases.py``).
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
from PIL import Image

from dataloader_amd import fallback
from dataloader_amd.engine import pack_jpegs
from dataloader_amd.params import make_aug_config
from dataloader_amd.config import DINOAugConfig
from dataloader_amd.synthetic import encode_jpeg, textured_rgb
from tests import cmyk_cases as cc

P = ctypes.c_void_p


@pytest.fixture(scope="module")
def emu4():
    return cc.build_emu4()


@pytest.fixture(scope="module")
def files():
    return cc.cases()


def _probe(jpegs, cfg=None):
    buf, off = pack_jpegs(jpegs, pin=False)
    return fallback.probe(buf.data_ptr(), off.numpy(), len(jpegs), 0, cfg)


def test_cmyk2rgb_matches_pillow_on_every_pair(emu4):
    """four_to_rgb (CMYK) == Pillow's "CMYK;I" read + convert("RGB") for all 65 536 (c, k) pairs
    (the other two channels take other values of the same range alongside)."""
    c, k = np.meshgrid(np.arange(256), np.arange(256))
    s = np.stack([c, 255 - c, (c * 7 + k) & 255, k], -1).astype(np.uint8)  # samples as libjpeg hands them over
    out = np.zeros((256, 256, 3), np.uint8)
    emu4.emu4_four_to_rgb(s.ctypes.data_as(P), 256 * 256, 0, out.ctypes.data_as(P))
    ref = np.asarray(Image.frombytes("CMYK", (256, 256), s.tobytes(), "raw", "CMYK;I").convert("RGB"))
    assert np.array_equal(out, ref)
    # the formula the issue quotes, checked against the same Pillow
    nk = s[..., 3].astype(np.int64)  # 255 - K with K = 255 - sample
    t = (255 - s[..., :3].astype(np.int64)) * nk[..., None] + 128
    assert np.array_equal(np.clip(nk[..., None] - (((t >> 8) + t) >> 8), 0, 255), ref)


def test_ycck_random_planes_match_pillow(emu4):
    """libjpeg's YCCK -> CMYK step on uniformly random planes (quality 100: every sample value
    and sharp chroma excursions that clip in ycc_rgb_convert), through a real file."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (64, 64, 4), dtype=np.uint8)
    for adobe in (2, 0):
        b = cc.encode4(img, cc.ONE_SCAN, quality=100, adobe=adobe)
        st, got = cc.emu4_decode(emu4, b, 64, 64)
        assert st == 0
        assert np.array_equal(got, cc.pillow_rgb(b)), adobe


@pytest.mark.parametrize("name", list(cc.cases()))
def test_host_model_matches_pillow(emu4, files, name):
    b = files[name]
    w, h = cc.size_of(b)
    ref = cc.pillow_rgb(b)
    st, got = cc.emu4_decode(emu4, b, w, h)
    if ref is None:  # Pillow raises: the reference zero-fills (cpu.py:252-253)
        assert st < 0 and not got.any()
    else:
        assert st == 0 and np.array_equal(got, ref)


def test_colour_space_of_a_four_component_frame(emu4, files):
    """jdapimin.c default_decompress_parms: Adobe transform 0 CMYK (3), 2 and any other YCCK (4), no
    Adobe marker (JFIF or not, or an 11-byte one) CMYK; off, the parser stops at SOF with status 1."""
    want = {"pil_base_33x31": 3, "ycck_11_33x31": 4, "adobe_t1_33x31": 4, "no_adobe_33x31": 3,
            "jfif_no_adobe_33x31": 3, "jfif_adobe_t2_17x9": 4, "adobe_11_bytes_33x31": 3}
    info = np.zeros(6, np.int32)
    for name, color in want.items():
        buf = np.frombuffer(files[name], np.uint8)
        assert emu4.emu4_parse(buf.ctypes.data_as(P), len(buf), 1, info.ctypes.data_as(P)) == 0
        assert (info[3], info[4], info[5]) == (4, color, 1), name  # four components, kind 1 even for one scan
        assert emu4.emu4_parse(buf.ctypes.data_as(P), len(buf), 0, info.ctypes.data_as(P)) == 1


def test_probe_reports_kind_3_and_counts_the_workspace(files):
    rng = np.random.default_rng(7)
    base = [encode_jpeg(textured_rgb(64, 48, rng)) for _ in range(3)]
    cfg = make_aug_config(DINOAugConfig(global_crop_size=64, local_crop_size=32, n_local_crops=2), 64, 32, 0)
    _, ws0, aws0 = _probe(base, cfg)
    for name in ("pil_base_70x50", "ycck_10blk_70x50", "pil_prog_70x50", "ycck_12blk_per_comp_70x50"):
        info, ws, aws = _probe(base + [files[name]], cfg)
        assert tuple(info[3]) == (1, 70, 50, 3), (name, info[3])
        # the dense int16 coefficients of the file's four planes (128 bytes a block)
        samp = cc.S10 if "10blk" in name else cc.S12 if "12blk" in name else cc.S11
        mx, my = -(-70 // (8 * 2)), -(-50 // (8 * 2))
        blocks = sum(h * v for h, v in samp) * mx * my if samp != cc.S11 else 4 * 9 * 7
        assert ws - ws0 >= blocks * 128, name
        assert aws > aws0, name
        assert fallback.augment_need(info, cfg) == aws  # a re-augment at other sizes counts its views too
    # a four-component file the device cannot decode either stays plainly unsupported
    for name in ("ycck_12blk_one_scan_33x31", "truncated_mid_scan_70x50"):
        info, ws, _ = _probe(base + [files[name]], cfg)
        assert info[3, 0] == 1 and info[3, 3] == -1 and ws == ws0, name


def test_route_mask_with_both_option_values(files):
    rng = np.random.default_rng(8)
    jpegs = [encode_jpeg(textured_rgb(64, 48, rng)), files["pil_base_33x31"],
             encode_jpeg(textured_rgb(64, 48, rng), progressive=True), files["ycck_10blk_33x31"],
             files["ycck_12blk_one_scan_33x31"]]
    info, _, _ = _probe(jpegs)
    assert info[:, 0].tolist() == [0, 1, 0, 1, 1] and info[:, 3].tolist() == [0, 3, 1, 3, -1]
    host = fallback.route_mask(info, True, "device", 8)
    assert host.tolist() == [False, True, False, True, True]
    assert np.array_equal(host, fallback.route_mask(info, True, "device", 8, four_component="host"))
    dev = fallback.route_mask(info, True, "device", 8, four_component="device")
    assert dev.tolist() == [False, False, False, False, True]  # (what Pillow refuses is still handed over)
    # like any coefficient-buffer image: the host route and "auto" take them along
    assert fallback.route_mask(info, True, "host", 8, four_component="device").tolist() == [False, True, True, True, True]
    assert fallback.route_mask(info, True, "auto", 8, four_component="device").tolist() == [False, True, True, True, True]
    assert fallback.route_mask(info, True, "auto", 2, four_component="device").tolist() == [False, False, False, False, True]
    acc = fallback.accept_four_component(info)
    assert acc[:, 0].tolist() == [0, 0, 0, 0, 1] and acc[:, 3].tolist() == [0, 1, 1, 1, -1]
    assert info[1, 0] == 1  # a copy
    out, n, rm = fallback.hand_over(jpegs, info[:, 0], four_component="device", kind=info[:, 3])
    assert n == 1 and out[1] is jpegs[1] and out[3] is jpegs[3] and out[4] == b"" and not rm.any()
    out, n, rm = fallback.hand_over(jpegs, info[:, 0])
    assert n == 3 and rm.tolist() == [0, 1, 0, 1, 0]
    with pytest.raises(ValueError):
        fallback.route_mask(info, True, "device", 8, four_component="gpu")

"""``exif_transpose`` on the host: ``dino_probe_orient`` against Pillow's ``getexif``, the one
mapping of the eight orientations against ``ImageOps.exif_transpose``, and the hand-over."""

from __future__ import annotations

import io

import numpy as np
import pytest
from PIL import Image, ImageOps

from dataloader_amd import fallback
from tests import header_cases as hc

XMP6 = hc.seg(0xE1, b'http://ns.adobe.com/xap/1.0/\x00<x:xmpmeta><rdf:Description tiff:Orientation="6"/></x:xmpmeta>')


def _mm(value: int) -> bytes:
    return b"MM\x00*" + (8).to_bytes(4, "big") + b"\x00\x01\x01\x12\x00\x03\x00\x00\x00\x01" \
        + value.to_bytes(2, "big") + b"\x00\x00" + b"\0\0\0\0"


def orient_files() -> list[tuple[str, bytes, bool]]:
    """(name, file, the rule of exif_parse.hpp calls it verified)."""
    b = hc.bases()
    _exif = lambda tiff: hc.seg(0xE1, hc.EXIF + tiff)  # noqa: E731
    at = lambda segs, base="b420": hc.insert(b[base], "app0", segs)  # noqa: E731
    out = [(f"{e}{v}", at(_exif(hc._tiff([(0x0112, 3, 1, v)]) if e == "ii" else _mm(v))), 1 <= v <= 8)
           for e in ("ii", "mm") for v in range(10)]
    out += [
        ("untagged", b["b420"], True),
        ("no_entry", at(_exif(hc._tiff([(0x0110, 3, 1, 6)]))), True),
        ("long", at(_exif(hc._tiff([(0x0112, 4, 1, 6)]))), False),
        ("count2", at(_exif(hc._tiff([(0x0112, 3, 2, 6)]))), False),
        ("ifd_outside", at(_exif(hc._tiff([(0x0112, 3, 1, 6)], ifd=4000))), False),
        ("ifd_truncated", at(_exif(hc._tiff([(0x0110, 3, 1, 1), (0x0112, 3, 1, 6)])[:-10])), False),
        ("two_exif", at(_exif(hc.ORIENT6) + _exif(hc.ORIENT6)), False),
        ("xmp_only", at(XMP6), False),
        ("exif3_xmp6", at(_exif(hc._tiff([(0x0112, 3, 1, 3)])) + XMP6), True),
        ("exif1_xmp6", at(_exif(hc._tiff([(0x0112, 3, 1, 1)])) + XMP6), True),
        ("after_6k", at(hc.seg(0xE5, hc._noise(6144, 3)) + _exif(hc.ORIENT6)), True),
        ("gray", at(_exif(hc.ORIENT6), "gray"), True),
        ("prog", at(_exif(hc.ORIENT6), "prog"), True),
    ]
    return out


@pytest.mark.parametrize("name,data,verified", orient_files(), ids=[c[0] for c in orient_files()])
def test_probe_orient_is_pillows_tag_or_unverified(name, data, verified):
    got = int(fallback.probe_orient_list([data])[0])
    want = Image.open(io.BytesIO(data)).getexif().get(0x0112, 1)
    assert got in ((0 if want == 1 else want), fallback.ORIENT_UNVERIFIED), (got, want)
    assert not (verified and got == fallback.ORIENT_UNVERIFIED)


@pytest.mark.parametrize("o", range(1, 9))
def test_mapping_is_exif_transpose(o):
    src = np.arange(18, dtype=np.uint8).reshape(2, 3, 3)  # H = 2, W = 3, every pixel distinct
    im, ex = Image.fromarray(src), Image.Exif()
    ex[0x0112] = o
    im.info["exif"] = ex.tobytes()
    ref = np.asarray(ImageOps.exif_transpose(im))
    for y in range(2):
        for x in range(3):
            ox, oy = fallback.orient_map(o, 3, 2, x, y)
            assert np.array_equal(ref[oy, ox], src[y, x]), (o, x, y, ox, oy)


@pytest.mark.parametrize("draft", [0, 16])
def test_hand_over_is_upright(draft):
    rng, b, ex = np.random.default_rng(5), io.BytesIO(), Image.Exif()
    ex[0x0112] = 5
    Image.fromarray(rng.integers(0, 256, (70, 130, 3), dtype=np.uint8)).save(b, "JPEG", exif=ex.tobytes())
    im = Image.open(io.BytesIO(b.getvalue()))
    if draft:
        im.draft("RGB", (draft, draft))
    ref = np.asarray(ImageOps.exif_transpose(im).convert("RGB"))
    assert ref.shape[:2] == ((33, 18) if draft else (130, 70))
    for c in (fallback.pillow_container(b.getvalue(), draft, True),
              fallback.hand_over([b.getvalue()], np.array([1]), draft=draft, exif_transpose=True)[0][0]):
        assert c == fallback.raw_container(ref)


def test_view_scratch_follows_the_upright_size():
    """The scratch bound is not symmetric (crop_h rows of the horizontal pass): a landscape file
    that turns to portrait needs more than the probe, which sees the coded size, reserved."""
    from dataloader_amd.config import DINOAugConfig
    from dataloader_amd.engine import pack_jpegs
    from dataloader_amd.params import make_aug_config
    cfg = make_aug_config(DINOAugConfig(), 224, 96, 0)
    files = [hc.insert(hc.encode_jpeg(np.zeros((30, 400, 3), np.uint8)), "app0", hc.seg(0xE1, hc.EXIF + hc.ORIENT6)), hc.bases()["b420"]]
    buf, off = pack_jpegs(files, pin=False)
    info, _, aws = fallback.probe(buf.data_ptr(), off.numpy(), 2, 0, cfg)
    up, _, more = fallback.accept_orient(info, fallback.probe_orient_list(files), cfg)
    assert tuple(up[0, 1:3]) == (30, 400) and more > 0 and aws + more == fallback.augment_need(up, cfg)

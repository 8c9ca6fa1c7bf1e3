"""``jpeg_draft`` on the host: the scale rule against Pillow's ``Image.draft``, the hand-overs
under the option, and the values the option refuses."""

from __future__ import annotations

import io

import numpy as np
import pytest
from PIL import Image

from dataloader_amd import fallback
from dataloader_amd.engine import pack_jpegs
from dataloader_amd.synthetic import textured_rgb
from tests import jpeg_writer as jw

SIDES = (1, 7, 8, 9, 16, 17, 70, 641, 1600)
NS = (1, 4, 8, 16, 100, 224, 2000)


def _save(im, fmt="JPEG") -> bytes:
    b = io.BytesIO()
    im.save(b, fmt)
    return b.getvalue()


@pytest.mark.parametrize("w", SIDES)
def test_draft_scale_is_pillows_rule(w):
    for h in SIDES:
        data = _save(Image.new("L", (w, h)))
        for n in NS:
            im = Image.open(io.BytesIO(data))
            im.draft("RGB", (n, n))
            assert fallback.draft_scale(w, h, n) == (im.decoderconfig[0], *im.size), (w, h, n)


def test_hand_overs_decode_under_the_draft():
    rng = np.random.default_rng(31)
    smoothed = jw.encode(textured_rgb(70, 50, rng), jw.unrefined_progression(), progressive=True)
    cmyk = _save(Image.fromarray(rng.integers(0, 256, size=(50, 70, 4), dtype=np.uint8), "CMYK"))
    png = _save(Image.fromarray(textured_rgb(70, 50, rng)), "PNG")
    files = [smoothed, cmyk, png]
    buf, off = pack_jpegs(files, pin=False)
    info, _, _ = fallback.probe(buf.data_ptr(), off.numpy(), len(files), 0)
    assert list(info[:2, 0]) == [fallback.IMG_UNSUPPORTED] * 2 and info[2, 3] == fallback.KIND_PNG
    pool = fallback.HostDecoder(1, draft=16)
    pool._inline = True  # the in-process path: the workers run the same pillow_container
    for out in (fallback.hand_over(files, info[:, 0], kind=info[:, 3], png="host", draft=16)[0],
                [pool.submit(f).result() for f in files]):
        for data, c, size in zip(files, out, ((35, 25), (35, 25), (70, 50))):
            im = Image.open(io.BytesIO(data))
            im.draft("RGB", (16, 16))
            ref = np.asarray(im.convert("RGB"))
            assert (ref.shape[1], ref.shape[0]) == size
            assert c == fallback.raw_container(ref)
    assert fallback.pillow_container(png, 16) == fallback.pillow_container(png)


@pytest.mark.parametrize("kw", [dict(jpeg_draft=-1), dict(jpeg_draft=1.5), dict(jpeg_draft="32"),
                                dict(jpeg_draft=32, four_component="device")])
def test_bad_values_raise(kw):
    from dataloader_amd.backend import MI355XBackend
    with pytest.raises(ValueError):
        MI355XBackend(**kw)
    assert MI355XBackend(jpeg_draft=32)._jpeg_draft == 32 and MI355XBackend()._jpeg_draft == 0

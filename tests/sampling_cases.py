"""JPEG files of the chroma samplings and colour markers that Pillow's writer cannot produce
(TEST INFRASTRUCTURE ONLY; shared by test_sampling_cpu.py and test_gpu_sampling.py).

Every file comes from ``tests/jpeg_writer.py`` with a seeded generator; nothing is stored in
git.  Each group returns ``[(name, jpeg_bytes)]`` and is built once per process.  The
expectation for every file is whatever ``oracle.cpu_ref.decode_rgb`` does with its bytes: an
image -> status 0 and identical pixels, ``None`` -> status < 0 and a zero-filled image.

Blocks per MCU (sum of h*v over the components; libjpeg's D_MAX_BLOCKS_IN_MCU and this
decoder's kMaxBlocksPerMcu are both 10):

  s440 4, s411 6, s410 10, s1x4 6, c2x1 8, c1x2 8, cbcr 7, cbfull 9, ylow22 9, ylow21 4, h3 5.

``b11`` (4,2),(2,1),(1,1) and ``b12`` (4,2),(2,1),(2,1) have 11 and 12 blocks: libjpeg raises
JERR_BAD_MCU_SIZE, Pillow fails and the reference zero-fills them, as it does for the
fractional ratio of ``frac`` (3,2),(2,1),(1,1).  They stay in the small and progressive groups
as rejected files; libjpeg counts blocks per interleaved scan, so b12 under the deep script
(single-component scans only) decodes.  The route files of the largest MCU use s410, the
layout that really has ten blocks.
"""

from __future__ import annotations

import functools

import numpy as np

from dataloader_amd.synthetic import textured_rgb
from tests import jpeg_writer as jw

LAYOUTS = {
    "s440": ((1, 2), (1, 1), (1, 1)),    # 4:4:0: kUpH1V2Fancy
    "s411": ((4, 1), (1, 1), (1, 1)),    # 4:1:1: kUpInt
    "s410": ((4, 2), (1, 1), (1, 1)),    # 4:1:0: kUpInt, 10 blocks per MCU
    "s1x4": ((1, 4), (1, 1), (1, 1)),
    "c2x1": ((2, 2), (2, 1), (2, 1)),    # chroma 2x1 under luma 2x2
    "c1x2": ((2, 2), (1, 2), (1, 2)),    # chroma 1x2 under luma 2x2
    "cbcr": ((2, 2), (1, 1), (2, 1)),    # Cb and Cr at different samplings
    "cbfull": ((2, 2), (2, 2), (1, 1)),  # Cb at luma resolution
    "ylow22": ((1, 1), (2, 2), (2, 2)),  # luma below chroma: the luma plane is upsampled
    "ylow21": ((1, 1), (2, 1), (1, 1)),
    "h3": ((3, 1), (1, 1), (1, 1)),      # 3x horizontal
    "b11": ((4, 2), (2, 1), (1, 1)),     # rejected: 11 blocks per MCU
    "b12": ((4, 2), (2, 1), (2, 1)),     # rejected: 12 blocks per MCU
    "frac": ((3, 2), (2, 1), (1, 1)),    # rejected: fractional upsampling ratio
}
REJECTED_LAYOUTS = ("b11", "b12", "frac")
SMALL_SIZES = ((1, 1), (3, 5), (4, 4), (5, 3), (17, 9), (33, 31), (70, 50))
WIDE_SIZE = (2305, 9)
WIDE_LAYOUTS = ("s440", "s411", "cbcr", "ylow22")
ROUTE_LAYOUTS = ("s440", "s410", "cbcr")

# Huffman routes (kernels.hip k_htab / huff_single_segment): an image is one
# segment up to kHuffSegBits = 2 Mbit of destuffed entropy data; a one-segment image's 256 lane
# ranges finish in k_huff1 while a range is <= 3072 bits, i.e. up to 96 KiB.
HUFF1_MAX_BYTES = 256 * 3072 // 8   # 98 304: above it the lanes are re-decoded by k_huff3
SEGMENT_BYTES = 2048 * 1024 // 8    # 262 144: above it k_huff2 syncs across segments
# (w, h) of the uniform-noise quality-98 files, sized a few per cent past each threshold
ROUTE_SIZES = {
    "huff3": {"s440": (320, 224), "s410": (352, 288), "cbcr": (320, 240)},
    "huff2": {"s440": (480, 352), "s410": (608, 448), "cbcr": (512, 384)},
}

ONE_SCAN = [jw.scan((0, 1, 2))]


def _seq(img, layout, **kw) -> bytes:
    return jw.encode(img, ONE_SCAN, samp=LAYOUTS[layout], **kw)


def _noise(w, h, rng) -> np.ndarray:
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def sof_size(jpeg: bytes) -> tuple[int, int]:
    """(width, height) from the first SOF0/1/2 segment."""
    k = min(i for i in (jpeg.find(bytes([0xFF, m])) for m in (0xC0, 0xC1, 0xC2)) if i >= 0)
    return int.from_bytes(jpeg[k + 7:k + 9], "big"), int.from_bytes(jpeg[k + 5:k + 7], "big")


def entropy_bytes(jpeg: bytes) -> int:
    """Destuffed entropy bytes of a one-scan file: what the decoder's lane plan is sized from."""
    k = jpeg.index(b"\xff\xda")
    scan = jpeg[k + 2 + int.from_bytes(jpeg[k + 2:k + 4], "big"):-2]
    n_rst = sum(scan.count(bytes([0xFF, 0xD0 + r])) for r in range(8))
    return len(scan) - scan.count(b"\xff\x00") - 2 * n_rst


@functools.lru_cache(maxsize=None)
def small_cases():
    rng = np.random.default_rng(1101)
    return [(f"{name}_{w}x{h}", _seq(textured_rgb(w, h, rng), name))
            for name in LAYOUTS for (w, h) in SMALL_SIZES]


@functools.lru_cache(maxsize=None)
def wide_cases():
    rng = np.random.default_rng(1102)
    w, h = WIDE_SIZE
    return [(f"{name}_{w}x{h}", _seq(textured_rgb(w, h, rng), name, quality=90)) for name in WIDE_LAYOUTS]


@functools.lru_cache(maxsize=None)
def route_cases():
    """One file per (layout, Huffman route); names ``<layout>_<route>_<w>x<h>``."""
    rng = np.random.default_rng(1103)
    out = []
    for name in ROUTE_LAYOUTS:
        out.append((f"{name}_huff1_640x480", _seq(textured_rgb(640, 480, rng), name, quality=85)))
        for route in ("huff3", "huff2"):
            w, h = ROUTE_SIZES[route][name]
            out.append((f"{name}_{route}_{w}x{h}", _seq(_noise(w, h, rng), name, quality=98)))
    return out


def route_of(jpeg: bytes) -> str:
    n = entropy_bytes(jpeg)
    return "huff1" if n <= HUFF1_MAX_BYTES else "huff3" if n <= SEGMENT_BYTES else "huff2"


def mcus_per_row(layout: str, w: int) -> int:
    return -(-w // (8 * max(s[0] for s in LAYOUTS[layout])))


@functools.lru_cache(maxsize=None)
def restart_cases():
    """Restart intervals of 1, 3, one MCU row and 1000 MCUs (more than the small image holds),
    and on a file of the 96 KiB class, whose intervals spread over several 256-lane work items."""
    rng = np.random.default_rng(1104)
    out = []
    for name in ("s440", "s410"):
        img = textured_rgb(70, 50, rng)
        for ri in (1, 3, mcus_per_row(name, 70), 1000):
            out.append((f"{name}_70x50_ri{ri}", _seq(img, name, restart=ri)))
    w, h = ROUTE_SIZES["huff3"]["s440"]
    img = _noise(w, h, rng)
    for ri in (1, 3, mcus_per_row("s440", w), 1000):
        out.append((f"s440_{w}x{h}_ri{ri}", _seq(img, "s440", quality=98, restart=ri)))
    return out


@functools.lru_cache(maxsize=None)
def progressive_cases():
    rng = np.random.default_rng(1105)
    out = []
    for name in ("s440", "s411", "s410", "b12"):
        img = textured_rgb(70, 50, rng)
        for sname, script in (("simple", jw.simple_progression()), ("deep", jw.deep_progression())):
            out.append((f"{name}_70x50_{sname}", jw.encode(img, script, samp=LAYOUTS[name], progressive=True)))
    return out


# ---- colour markers ---------------------------------------------------------------------
RGB_IDS = (82, 71, 66)
_JFIF = b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"


def adobe_segment(transform: int, n: int = 12) -> bytes:
    """APP14 "Adobe" (version 100, flags 0, transform), cut or zero-padded to ``n`` payload bytes."""
    return jw._seg(0xEE, (b"Adobe" + bytes([0, 100, 0, 0, 0, 0, transform]) + b"\0\0")[:n])


def jfif_segment(n: int = 14) -> bytes:
    """APP0 "JFIF\\0..." cut or zero-padded to ``n`` payload bytes."""
    return jw._seg(0xE0, (_JFIF + b"\0\0")[:n])


def after_soi(jpeg: bytes, segment: bytes) -> bytes:
    assert jpeg[:2] == b"\xff\xd8"
    return jpeg[:2] + segment + jpeg[2:]


def with_sof1(jpeg: bytes) -> bytes:
    k = jpeg.index(b"\xff\xc0")
    return jpeg[:k + 1] + b"\xc1" + jpeg[k + 2:]


def with_dqt16(jpeg: bytes, add_hi: int = 0) -> bytes:
    """Every DQT segment (one 8-bit table each, as the writer emits them) rewritten at 16-bit
    precision (Pq = 1) with the same values; ``add_hi`` goes into the high byte of the last
    (zigzag 63) entry, so that a value above 255 is read."""
    out, pos = bytearray(jpeg[:2]), 2
    while jpeg[pos + 1] != 0xDA:
        n = int.from_bytes(jpeg[pos + 2:pos + 4], "big")
        if jpeg[pos + 1] == 0xDB:
            assert n == 67 and jpeg[pos + 4] < 4
            out += jw._seg(0xDB, bytes([0x10 | jpeg[pos + 4]]) + b"".join(bytes([0, v]) for v in jpeg[pos + 5:pos + 68]) + bytes([add_hi, jpeg[pos + 68]]))
        else:
            out += jpeg[pos:pos + 2 + n]
        pos += 2 + n
    return bytes(out + jpeg[pos:])


@functools.lru_cache(maxsize=None)
def marker_cases():
    """The inputs of libjpeg's default_decompress_parms colour-space guess (JFIF APP0, Adobe
    APP14 and its transform, component ids) and their length rules (examine_app0 /
    examine_app14), SOF1 and 16-bit DQT, on 40x24 files at 4:4:4 and 4:2:0."""
    rng = np.random.default_rng(1106)
    out = []
    for sname, samp in (("444", ((1, 1), (1, 1), (1, 1))), ("420", ((2, 2), (1, 1), (1, 1)))):
        img = textured_rgb(40, 24, rng)

        def enc(**kw):
            return jw.encode(img, ONE_SCAN, samp=samp, **kw)

        def add(name, data):
            out.append((f"{name}_{sname}", data))

        plain, nojfif = enc(), enc(jfif=False)
        rgb_nojfif = enc(jfif=False, comp_ids=RGB_IDS)
        add("jfif", plain)
        add("nojfif", nojfif)
        add("rgbids_jfif", enc(comp_ids=RGB_IDS))
        add("rgbids_nojfif", rgb_nojfif)
        add("ids012_jfif", enc(comp_ids=(0, 1, 2)))
        add("ids012_nojfif", enc(jfif=False, comp_ids=(0, 1, 2)))
        for t in (0, 1, 2):
            add(f"adobe{t}_jfif", enc(before_scan={0: adobe_segment(t)}))
            add(f"adobe{t}_nojfif", enc(jfif=False, before_scan={0: adobe_segment(t)}))
            add(f"adobe{t}_first_nojfif", after_soi(nojfif, adobe_segment(t)))
        for n in (5, 6, 7, 11, 12, 14):  # Pillow raises below 7; transform 0: recognised -> RGB, ignored -> YCbCr
            add(f"adobe0_len{n}_nojfif", after_soi(nojfif, adobe_segment(0, n)))
            add(f"adobe1_len{n}_rgbids", after_soi(rgb_nojfif, adobe_segment(1, n)))
        for n in (4, 5, 6, 7, 13, 14, 16):  # Pillow raises below 7; recognised -> YCbCr, ignored -> RGB by the ids
            add(f"app0_len{n}_rgbids", after_soi(rgb_nojfif, jfif_segment(n)))
        add("jfxx_rgbids", after_soi(rgb_nojfif, jw._seg(0xE0, b"JFXX\x00\x10" + bytes(8))))
        add("jfxx_after_jfif", after_soi(nojfif, jfif_segment() + jw._seg(0xE0, b"JFXX\x00\x10" + bytes(8))))
        add("sof1", with_sof1(plain))
        add("sof1_rgbids_nojfif", with_sof1(rgb_nojfif))
        add("dqt16", with_dqt16(plain))
        add("dqt16_q30", with_dqt16(enc(quality=30)))
        add("dqt16_hi", with_dqt16(enc(quality=98), add_hi=1))
    return out


GROUPS = {"small": small_cases, "wide": wide_cases, "route": route_cases, "restart": restart_cases,
          "progressive": progressive_cases, "markers": marker_cases}


@functools.lru_cache(maxsize=None)
def references(group: str):
    """The oracle's decode of every file of a group, computed once: a read-only H x W x 3
    array, or ``None`` where the reference zero-fills."""
    from oracle import cpu_ref
    out = []
    for _, j in GROUPS[group]():
        img = cpu_ref.decode_rgb(j)
        arr = None if img is None else np.asarray(img).copy()
        if arr is not None:
            arr.setflags(write=False)
        out.append(arr)
    return out

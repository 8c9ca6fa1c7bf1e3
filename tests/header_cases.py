"""JPEG files whose headers carry what encoders in the suite never write (TEST INFRASTRUCTURE
ONLY; shared by test_header_cases_cpu.py and test_gpu_header_walk.py).

The header walk is ``parse_jpeg`` (csrc/jpeg_parse.hpp; k_parse and dino_probe run it) and, from
the first SOS on, ``prog_walk`` (csrc/progressive.hpp; k_pwalk).  k_parse walks the file's first
4096 bytes (kParsePrefix) in LDS and only a header longer than that in global memory.  Three
families, all made from five 40 x 24 base files:

  (a) metadata   EXIF, ICC, XMP, MPF / MPO, Photoshop, JFXX, long COM segments, marker bytes
                 inside a payload; every one with the header under 4096 bytes and over
  (b) prefix     one COM sized so that a named byte of the header lands on 4094..4097
  (c) markers    segments with a length below 2, FF 00 between segments, reserved and
                 parameterless markers, DQT precision nibbles, exact lengths; at every place a
                 segment can stand: after APP0, between DQT and SOF, between SOF and SOS and
                 between two scans

A case declares ``"decodes"`` or ``"raises"``: what ``Image.open(...).convert("RGB")`` does with
the bytes.  test_header_cases_cpu.py holds every declaration to Pillow; before the first SOS
Pillow's own marker loop (JpegImagePlugin._open) and libjpeg's read_markers (jdmarker.c) both
have to accept the file, from the first SOS on only libjpeg's.  A decoding case decodes to the
pixels of ``pixels_of``: its base file, or for the MPO the plain JPEG of its first frame.

Nothing is stored in git: the cases are built once per process from seeded images.
"""

from __future__ import annotations

import functools
import io
from dataclasses import dataclass

import numpy as np

from dataloader_amd.synthetic import encode_jpeg, textured_rgb
from tests import jpeg_writer as jw

PREFIX = 4096  # kParsePrefix (csrc/kernels.hip)
W, H = 40, 24
BOUNDARY_OFFSETS = (4094, 4095, 4096, 4097)
MAX_PAYLOAD = 65533  # a segment's length field is 16 bits and counts itself


@dataclass(frozen=True)
class Case:
    name: str
    data: bytes
    expect: str             # "decodes" / "raises"
    pixels_of: str          # a key of references()
    family: str             # "a", "b", "c"
    at: tuple | None = None  # family (b): (what, file offset the named byte is meant to have)


def seg(marker: int, payload: bytes = b"") -> bytes:
    assert len(payload) <= MAX_PAYLOAD
    return jw._seg(marker, payload)


# ---- base files ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bases() -> dict:
    rng = np.random.default_rng(1401)
    img = textured_rgb(W, H, rng)
    return {
        "b420": encode_jpeg(img, subsampling=2),
        "b444": encode_jpeg(img, subsampling=0),
        "gray": encode_jpeg(img, gray=True),
        "prog": encode_jpeg(img, subsampling=2, progressive=True),
        "k1": jw.encode(img, jw.sequential_per_component(), samp=((2, 2), (1, 1), (1, 1))),
    }


def layout(jpeg: bytes) -> list[tuple[int, int, int]]:
    """(marker, offset of its FF, offset after the segment) of every segment of a well-formed
    file up to its EOI; a SOS entry ends with its header, and the entry after it starts at the
    marker that ends the scan's entropy data."""
    out, pos = [], 2
    while True:
        assert jpeg[pos] == 0xFF, pos
        m = jpeg[pos + 1]
        if m == 0xD9:
            return out
        end = pos + 2 + int.from_bytes(jpeg[pos + 2:pos + 4], "big")
        out.append((m, pos, end))
        pos = end
        if m == 0xDA:
            while not (jpeg[pos] == 0xFF and jpeg[pos + 1] != 0 and not 0xD0 <= jpeg[pos + 1] <= 0xD7):
                pos += 1


def first(jpeg: bytes, marker: int) -> tuple[int, int]:
    """(offset, end) of the first segment with this marker."""
    return next((a, b) for m, a, b in layout(jpeg) if m == marker)


def sof_marker(jpeg: bytes) -> int:
    return next(m for m, _, _ in layout(jpeg) if m in (0xC0, 0xC2))


PLACES = ("app0", "dqt_sof", "sof_sos", "scans")


def place(jpeg: bytes, where: str) -> int:
    """File offset of a named place between two segments: after APP0, between the last DQT
    and SOF, right after SOF, and between the first scan's entropy data and what follows it."""
    if where == "app0":
        return first(jpeg, 0xE0)[1]
    if where == "dqt_sof":
        return first(jpeg, sof_marker(jpeg))[0]
    if where == "sof_sos":
        return first(jpeg, sof_marker(jpeg))[1]
    lay = layout(jpeg)
    k = next(i for i, (m, _, _) in enumerate(lay) if m == 0xDA)
    assert k + 1 < len(lay), "a one-scan file has no place between scans"
    return lay[k + 1][1]


def insert(jpeg: bytes, where: str | int, data: bytes) -> bytes:
    k = where if isinstance(where, int) else place(jpeg, where)
    return jpeg[:k] + data + jpeg[k:]


def grow(jpeg: bytes, marker: int, n: int, nth: int = 0, fill: int = 0) -> bytes:
    """The nth segment with this marker made n bytes longer (length field and bytes)."""
    a, b = [(a, b) for m, a, b in layout(jpeg) if m == marker][nth]
    ln = int.from_bytes(jpeg[a + 2:a + 4], "big") + n
    return jpeg[:a + 2] + ln.to_bytes(2, "big") + jpeg[a + 4:b] + bytes([fill]) * n + jpeg[b:]


def com_pad(n: int) -> bytes:
    """COM segments of n bytes in all (n >= 4; several above 65535)."""
    out = b""
    while n:
        take = n if n <= MAX_PAYLOAD + 2 else min(MAX_PAYLOAD + 2, n - 4)
        out += seg(0xFE, bytes((7 * k + 1) % 251 + 1 for k in range(take - 4)))
        n -= take
    return out


def pad_to(jpeg: bytes, target: int, at: int, k: int | None = None) -> bytes:
    """COM segments after APP0 (or at offset k) so that byte ``at`` of the file lands on offset
    ``target``."""
    k = place(jpeg, "app0") if k is None else k
    assert at >= k and target - at >= 4
    out = insert(jpeg, k, com_pad(target - at))
    assert out[target:target + 1] == jpeg[at:at + 1]
    return out


# ---- (a) metadata ----------------------------------------------------------------------------
def _tiff(entries: list[tuple[int, int, int, int]], ifd: int = 8, tail: bytes = b"") -> bytes:
    body = b"II*\x00" + ifd.to_bytes(4, "little") + len(entries).to_bytes(2, "little")
    for tag, typ, count, value in entries:
        body += tag.to_bytes(2, "little") + typ.to_bytes(2, "little") + count.to_bytes(4, "little") \
            + value.to_bytes(4, "little")
    return body + b"\0\0\0\0" + tail


def _noise(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


ICC = b"ICC_PROFILE\x00"
EXIF = b"Exif\x00\x00"
ORIENT6 = _tiff([(0x0112, 3, 1, 6)])


def icc(seq: int, count: int, n: int) -> bytes:
    return seg(0xE2, ICC + bytes([seq, count]) + _noise(n, 1410 + seq))


def metadata_items() -> list[tuple[str, bytes, str]]:
    """(name, segments, expectation when they stand after APP0)."""
    markers = b"\xff\xd9\xff\xda\xff\xd8\xff\x00"
    long_before = seg(0xE2, ICC + b"\x01\x02" + _noise(40, 1421))
    long_after = seg(0xE2, ICC + b"\x02\x02" + _noise(40, 1422))
    return [
        ("exif_orient6", seg(0xE1, EXIF + ORIENT6), "decodes"),  # (the reference does not transpose)
        ("exif_empty", seg(0xE1, EXIF), "decodes"),
        ("exif_garbage", seg(0xE1, EXIF + _noise(64, 1402)), "decodes"),
        ("exif_bad_ifd", seg(0xE1, EXIF + _tiff([(0x0112, 3, 1, 6)], ifd=0xFFFFFF00)), "decodes"),
        ("exif_6k", seg(0xE1, EXIF + _tiff([(0x0112, 3, 1, 6)], tail=_noise(6000, 1403))), "decodes"),
        ("exif_65533", seg(0xE1, (EXIF + ORIENT6 + _noise(MAX_PAYLOAD, 1404))[:MAX_PAYLOAD]), "decodes"),
        ("icc_one", icc(1, 1, 128), "decodes"),
        ("icc_three_full", b"".join(icc(k, 3, MAX_PAYLOAD - 14) for k in (1, 2, 3)), "decodes"),
        ("icc_wrong_count", icc(1, 2, 128), "decodes"),
        # Pillow's SOF handler reads byte 13 of the first of the sorted chunks
        ("icc_short12", seg(0xE2, ICC), "raises"),
        ("icc_short13", seg(0xE2, ICC + b"\x01"), "raises"),
        ("icc_short13_after_long", long_before + seg(0xE2, ICC + b"\x02"), "decodes"),
        ("icc_short13_before_long", seg(0xE2, ICC + b"\x01") + long_after, "raises"),
        ("icc_short13_prefix_of_long", long_before + seg(0xE2, ICC + b"\x01"), "raises"),
        ("icc_short12_beside_long", long_before + seg(0xE2, ICC), "raises"),
        ("xmp", seg(0xE1, b"http://ns.adobe.com/xap/1.0/\x00<x:xmpmeta xmlns:x='adobe:ns:meta/'>"
                    + b"<rdf:li>tiff:Orientation=6</rdf:li>" * 20 + b"</x:xmpmeta>"), "decodes"),
        ("mpf_empty", seg(0xE2, b"MPF\x00"), "decodes"),
        ("mpf_garbage", seg(0xE2, b"MPF\x00" + _noise(90, 1405)), "decodes"),
        ("ps_garbage", seg(0xED, b"Photoshop 3.0\x00" + _noise(70, 1406)), "decodes"),
        ("ps_short", seg(0xED, b"Photoshop 3.0\x008BIM\x03"), "decodes"),
        # the resource walk catches struct.error only: a block that ends with its code leaves
        # an IndexError at the name length
        ("ps_ends_after_code", seg(0xED, b"Photoshop 3.0\x008BIM\x03\xed"), "raises"),
        ("ps_block_then_ends_after_code", seg(0xED, b"Photoshop 3.0\x008BIM\x04\x04\x00\x00\x00\x00\x00\x03abc\x00"
                                              b"8BIM\x04\x05"), "raises"),
        ("ps_block", seg(0xED, b"Photoshop 3.0\x008BIM\x04\x04\x00\x00\x00\x00\x00\x03abc\x00"), "decodes"),
        ("jfxx", seg(0xE0, b"JFXX\x00\x13" + bytes([2, 2]) + _noise(12, 1407)), "decodes"),
        ("com_65533", seg(0xFE, _noise(MAX_PAYLOAD, 1408)), "decodes"),
        ("three_app1_65533", b"".join(seg(0xE1, _noise(MAX_PAYLOAD, 1430 + k)) for k in range(3)), "decodes"),
        ("adobe_in_app13", seg(0xED, b"Adobe\x00d\x00\x00\x00\x00\x00\x00"), "decodes"),
        ("app1_of_markers", seg(0xE1, markers * 40), "decodes"),
    ]


@functools.lru_cache(maxsize=None)
def mpo_files() -> tuple[bytes, bytes]:
    """(a two-frame MPO written by Pillow, the plain JPEG of its first frame)."""
    from PIL import Image
    rng = np.random.default_rng(1409)
    frames = [Image.fromarray(textured_rgb(W, H, rng), "RGB") for _ in range(2)]
    buf, plain = io.BytesIO(), io.BytesIO()
    frames[0].save(buf, format="MPO", save_all=True, append_images=frames[1:], quality=85, subsampling=2)
    frames[0].save(plain, format="JPEG", quality=85, subsampling=2)
    assert b"MPF\x00" in buf.getvalue()
    return buf.getvalue(), plain.getvalue()


@functools.lru_cache(maxsize=None)
def metadata_cases() -> list[Case]:
    b = bases()
    out = []
    for name, segs, expect in metadata_items():
        if len(segs) + len(b["b420"]) < PREFIX - 200:
            out.append(Case(f"{name}_under", insert(b["b420"], "app0", segs), expect, "b420", "a"))
            over = com_pad(5000) + segs
        else:
            over = segs
        out.append(Case(f"{name}_over", insert(b["b444"], "app0", over), expect, "b444", "a"))
    items = dict((n, (s, e)) for n, s, e in metadata_items())
    out.append(Case("icc_short12_after_sof", insert(b["b420"], "sof_sos", items["icc_short12"][0]), "decodes", "b420", "a"))
    out.append(Case("icc_short13_after_sof_gray", insert(b["gray"], "sof_sos", items["icc_short13"][0]), "decodes",
                    "gray", "a"))
    out.append(Case("icc_one_after_sof", insert(b["b444"], "sof_sos", items["icc_one"][0]), "decodes", "b444", "a"))
    out.append(Case("exif_orient6_gray", insert(b["gray"], "app0", items["exif_orient6"][0]), "decodes", "gray", "a"))
    for name in ("exif_orient6", "icc_short13", "exif_6k"):
        out.append(Case(f"{name}_prog", insert(b["prog"], "app0", items[name][0]), items[name][1], "prog", "a"))
    out.append(Case("icc_one_k1", insert(b["k1"], "app0", com_pad(5000) + items["icc_one"][0]), "decodes", "k1", "a"))
    out.append(Case("mpo_two_frames", mpo_files()[0], "decodes", "mpo", "a"))
    return out


# ---- (b) the prefix boundary -----------------------------------------------------------------
def boundary_bytes(jpeg: bytes) -> dict:
    """What -> offset in the file, for the bytes family (b) puts on the boundary."""
    sof = sof_marker(jpeg)
    out = {}
    for tag, marker in (("sos", 0xDA), ("dht", 0xC4), ("dqt", 0xDB), ("sof", sof)):
        a, e = first(jpeg, marker)
        out[f"{tag}_ff"] = a
        out[f"{tag}_len"] = a + 2
        out[f"{tag}_mid"] = (a + e) // 2
    out["sos_last"] = first(jpeg, 0xDA)[1] - 1  # (scan_off is one past it)
    out["sof_end"] = first(jpeg, sof)[1]        # the first byte after SOF: SOF ends exactly at the offset
    del out["sos_mid"]
    return out


@functools.lru_cache(maxsize=None)
def boundary_cases() -> list[Case]:
    out = []
    for bname in ("b420", "k1"):
        j = bases()[bname]
        for what, at in boundary_bytes(j).items():
            for target in BOUNDARY_OFFSETS:
                out.append(Case(f"{bname}_{what}_at{target}", pad_to(j, target, at), "decodes", bname, "b", (what, target)))
        for total in (PREFIX - 1, PREFIX, PREFIX + 1):
            out.append(Case(f"{bname}_length{total}", pad_to(j, total, len(j)), "decodes", bname, "b", ("length", total)))
    return out


# ---- (c) markers and lengths -----------------------------------------------------------------
def _dqt16(jpeg: bytes, nibble: int) -> bytes:
    """The file's table 0 again with 16-bit entries under this precision nibble."""
    a, _ = first(jpeg, 0xDB)
    assert jpeg[a + 4] == 0x00  # 8-bit table 0 comes first
    return seg(0xDB, bytes([nibble << 4]) + b"".join(bytes([0, v]) for v in jpeg[a + 5:a + 69]))


def marker_items(jpeg: bytes) -> list[tuple[str, bytes, str, str]]:
    """(name, bytes, expectation before the first SOS, expectation between two scans).  Before
    the first SOS Pillow's marker loop and libjpeg both read the bytes; between scans libjpeg
    alone (Pillow's loop has stopped at the first SOS)."""
    D, R = "decodes", "raises"
    return [
        # skip_variable / get_interesting_appn and Pillow's _safe_read of a size <= 0: only the
        # two length bytes are consumed
        ("app5_len0", b"\xff\xe5\x00\x00", D, D),
        ("com_len1", b"\xff\xfe\x00\x01", D, D),
        ("app0_len0", b"\xff\xe0\x00\x00", D, D),
        ("app14_len1", b"\xff\xee\x00\x01", D, D),
        ("dnl_len0", b"\xff\xdc\x00\x00", D, D),
        ("dnl", b"\xff\xdc\x00\x04" + H.to_bytes(2, "big"), D, D),
        ("ff00", b"\xff\x00", D, D),
        ("ff00_twice_then_fill", b"\xff\x00\xff\x00\xff\xff", D, D),
        ("junk", b"\x12\x34\x56", D, D),
        ("ff_fill", b"\xff\xff\xff", D, D),
        ("rst0", b"\xff\xd0", D, D),
        ("dri0", b"\xff\xdd\x00\x04\x00\x00", D, D),
        ("dqt_pq1", _dqt16(jpeg, 1), D, D),
        ("dqt_pq2", _dqt16(jpeg, 2), D, D),
        ("dqt_pq15", _dqt16(jpeg, 15), D, D),
        # Pillow's loop: "no marker found"; libjpeg: a parameterless marker
        ("tem", b"\xff\x01", R, D),
        ("soi2", b"\xff\xd8", R, R),
        ("res02", seg(0x02, b"\x00\x00"), R, R),
        ("resbf", seg(0xBF, b"\x00\x00"), R, R),
        ("jpg_c8", seg(0xC8, b"\x00\x00"), R, R),
        ("jpg0_f0", seg(0xF0, b"\x00\x00"), R, R),
        ("jpg13_fd", seg(0xFD, b"\x00\x00"), R, R),
        ("dhp_de", seg(0xDE, b"\x08\x00\x18\x00\x28\x01\x01\x11\x00"), R, R),
        ("exp_df", seg(0xDF, b"\x11"), R, R),
        ("dri_len6", b"\xff\xdd\x00\x06\x00\x00\x00\x00", R, R),
        # the neighbours that keep failing: get_dqt / get_dht / get_dri / get_sof / get_sos leave
        # a length other than 0 (JERR_BAD_LENGTH) or read past the segment
        ("dqt_len0", b"\xff\xdb\x00\x00", R, R),
        ("dqt_len1", b"\xff\xdb\x00\x01", R, R),
        ("dht_len0", b"\xff\xc4\x00\x00", R, R),
        ("dht_len1", b"\xff\xc4\x00\x01", R, R),
        ("dri_len0", b"\xff\xdd\x00\x00", R, R),
        ("dri_len1", b"\xff\xdd\x00\x01", R, R),
        ("sof_len0", b"\xff\xc0\x00\x00", R, R),
        ("sof_len1", b"\xff\xc0\x00\x01", R, R),
        ("sos_len0", b"\xff\xda\x00\x00", R, R),
        ("sos_len1", b"\xff\xda\x00\x01", R, R),
    ]


@functools.lru_cache(maxsize=None)
def marker_cases() -> list[Case]:
    b = bases()
    out = []
    for bname, places in (("b420", PLACES[:3]), ("k1", PLACES[3:]), ("prog", PLACES[3:])):
        j = b[bname]
        for name, data, pre, between in marker_items(j):
            if bname == "prog" and name not in ("app5_len0", "ff00", "tem", "res02", "dqt_pq2", "exp_df"):
                continue
            for where in places:
                out.append(Case(f"{name}_{where}_{bname}", insert(j, where, data), between if where == "scans" else pre,
                                bname, "c"))
    # exact lengths of SOF and SOS (get_sof: 8 + 3 Nf, get_sos: 6 + 2 Ns), every base
    for bname, j in b.items():
        out.append(Case(f"sof_plus1_{bname}", grow(j, sof_marker(j), 1), "raises", bname, "c"))
        out.append(Case(f"sos_plus1_{bname}", grow(j, 0xDA, 1), "raises", bname, "c"))
    out.append(Case("sos2_plus1_k1", grow(b["k1"], 0xDA, 1, nth=1), "raises", "k1", "c"))
    out.append(Case("sos3_plus1_prog", grow(b["prog"], 0xDA, 1, nth=2), "raises", "prog", "c"))
    # a short segment as the last thing before a header byte on the boundary
    j = insert(b["b420"], "dqt_sof", b"\xff\xe5\x00\x00")
    out.append(Case("app5_len0_at4092_b420", pad_to(j, PREFIX - 4, place(b["b420"], "dqt_sof"), place(b["b420"], "app0")), "decodes", "b420", "c"))
    j = insert(b["b420"], "dqt_sof", b"\xff\x01")
    out.append(Case("tem_at4095_b420", pad_to(j, PREFIX - 1, place(b["b420"], "dqt_sof"), place(b["b420"], "app0")), "raises", "b420", "c"))
    return out


# ---- the list --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases() -> list[Case]:
    out = metadata_cases() + boundary_cases() + marker_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


@functools.lru_cache(maxsize=None)
def references() -> dict:
    """name -> the oracle's pixels (read-only H x W x 3) of every base file and of the MPO's
    first frame, computed once."""
    from oracle import cpu_ref
    out = {}
    for name, j in {**bases(), "mpo": mpo_files()[1]}.items():
        arr = np.asarray(cpu_ref.decode_rgb(j)).copy()
        arr.setflags(write=False)
        out[name] = arr
    return out

"""PNG format layer on the host: the host model (tests/emu/emu_png.cpp: png_parse.hpp and
inflate.hpp with one lane, the code k_pngwalk / k_inflate / k_unfilter run) and ``dino_probe``
against zlib and Pillow on every file of ``tests/png_cases.py``.
"""

from __future__ import annotations

import ctypes
import zlib
from pathlib import Path

import numpy as np
import pytest

from dataloader_amd import _lib, fallback
from tests import png_cases as pc

EMU = Path(__file__).parent / "emu" / "libdino_emu_png.so"


@pytest.fixture(scope="module")
def emu():
    if not EMU.exists():
        pytest.fail(f"{EMU} missing: run __graft_entry__.build()")
    return ctypes.CDLL(str(EMU))


def model_decode(emu, b: bytes):
    """(info[6], zlib stream, inflated rows, rgb) of the host model."""
    n = len(b)
    info = np.zeros(6, np.int32)
    cap = 1 << 20
    zs, inf, rgb = np.zeros(n + 16, np.uint8), np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    src = np.frombuffer(b, np.uint8)
    vp = ctypes.c_void_p
    emu.emu_png_decode(src.ctypes.data_as(vp), ctypes.c_int64(n), 65535, zs.ctypes.data_as(vp), inf.ctypes.data_as(vp),
                       rgb.ctypes.data_as(vp), ctypes.c_int64(cap), ctypes.c_int64(cap), info.ctypes.data_as(vp))
    return info, zs[:info[4]], inf[:info[5]], rgb


def probe(files: list):
    buf = np.frombuffer(b"".join(files) + b"\0" * 16, np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    return fallback.probe(buf.ctypes.data, off, len(files), 0)


CASES = pc.cases()


@pytest.mark.parametrize("name,data,expect", [c for c in CASES if c[2] != "gap"], ids=[c[0] for c in CASES if c[2] != "gap"])
def test_model_matches_pillow(emu, name, data, expect):
    ref = pc.pillow_rgb(data)
    info, zs, inf, rgb = model_decode(emu, data)
    if expect == "dev":
        assert ref is not None and info[0] == 0 and info[3] == 4, info
        assert (info[1], info[2]) == (ref.shape[1], ref.shape[0])
        # the inflated bytes against zlib (which may hold more than the rows: the model stops there)
        full = zlib.decompressobj().decompress(bytes(zs))
        assert bytes(inf) == full[:len(inf)], "inflate"
        assert np.array_equal(rgb[:ref.size].reshape(ref.shape), ref), "pixels"
    elif expect == "raise":
        assert ref is None and info[0] == -1 and info[3] == 4, info
    elif expect == "corrupt":
        assert ref is None and info[0] == -1 and info[3] == -1, info
    else:
        assert info[3] == 5 and info[0] == 1, info


@pytest.mark.xfail(strict=True, reason="adler_mismatch: DESIGN.md §8, the zlib trailer after the last row is not read")
def test_adler_mismatch_known_gap(emu):
    data = [c[1] for c in CASES if c[0] == "adler_mismatch"][0]
    assert pc.pillow_rgb(data) is None  # Pillow raises when the trailer lies in the chunk of the last row
    assert model_decode(emu, data)[0][0] == -1


@pytest.mark.xfail(strict=True, reason="stream_ends_at_row_3: DESIGN.md §8, a stream ending validly before the last "
                                       "row is an error here; Pillow returns the rows it has and zeros below")
def test_stream_ending_on_a_row_boundary_known_gap(emu):
    data = [c[1] for c in CASES if c[0] == "stream_ends_at_row_3"][0]
    ref = pc.pillow_rgb(data)
    assert ref is not None and not ref[3].any() and ref[:3].any()
    info, _, _, rgb = model_decode(emu, data)
    assert info[0] == 0 and np.array_equal(rgb[:ref.size].reshape(ref.shape), ref)


def test_declined_files_decode_through_the_hand_over():
    """Every declined file goes to Pillow under "host" and "device": the container holds Pillow's
    pixels, or nothing where Pillow raises (then the device reports -1 and zero-fills)."""
    dec = [c for c in CASES if c[2] == "declined"]
    info, _, _ = probe([c[1] for c in dec])
    for mode in ("host", "device"):
        out, n, rm = fallback.hand_over([c[1] for c in dec], info[:, 0], kind=info[:, 3], png=mode)
        assert n == len(dec)
        for (name, data, _), cont, raw in zip(dec, out, rm):
            ref = pc.pillow_rgb(data)
            if ref is None:
                assert cont == b"" and raw == 0, name
            else:
                assert raw == 1 and cont == fallback.raw_container(ref), name
    out, n, _ = fallback.hand_over([c[1] for c in dec], info[:, 0], kind=info[:, 3], png="off")
    assert n == 0


def test_probe_rows_and_workspace(emu):
    """Status -1 for every PNG; kind 4 / 5 / -1 as the model says; ws_need is the sum of the
    kind-4 files' chunk sizes as the layout gives them (ent, carry row, rows, palette, rgb)."""
    from dataloader_amd.synthetic import make_jpeg
    files = [c[1] for c in CASES]
    jpg = make_jpeg(32, 24, 1)
    info, ws, _ = probe(files + [jpg])
    alone, ws_jpg, _ = probe([jpg])
    assert np.array_equal(info[-1], alone[0])  # a non-PNG row is unchanged
    need = 0
    for (name, data, expect), row in zip(CASES, info):
        m = model_decode(emu, data)[0]
        want_kind = {"dev": 4, "raise": 4, "gap": 4, "corrupt": -1, "declined": 5}[expect]
        assert row[0] == -1 and row[3] == want_kind, (name, row)
        if want_kind == 4:
            assert (row[1], row[2]) == (m[1], m[2]), name
            lay = np.zeros(10, np.int64)
            src = np.frombuffer(data, np.uint8)
            assert emu.emu_png_layout(src.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(data)), 65535,
                                      lay.ctypes.data_as(ctypes.c_void_p)) == 0
            total, ent, carry, plane, pal, rgb, use_ent, use_carry, use_plane, use_rgb = lay.tolist()
            # what the kernels touch fits the regions image_chunk_bytes gives them
            assert use_ent <= ent and use_carry <= carry and use_plane <= plane and 768 <= pal and use_rgb <= rgb, name
            assert total >= ent + carry + plane + pal + rgb and total % 256 == 0, name
            need += total
        else:
            assert (row[1], row[2]) == (0, 0), name
    assert ws == need + ws_jpg


def test_accept_png_modes():
    info = np.array([[-1, 5, 7, 4], [-1, 0, 0, 5], [-1, 0, 0, -1], [0, 8, 8, 0]], np.int32)
    assert np.array_equal(fallback.accept_png(info, "off"), info)
    dev = fallback.accept_png(info, "device")
    assert dev[:, 0].tolist() == [0, 1, -1, 0] and dev[0, 3] == 1
    host = fallback.accept_png(info, "host")
    assert host[:, 0].tolist() == [1, 1, -1, 0]
    assert fallback.route_mask(info, True, "device", 0, png="device").tolist() == [False, True, False, False]
    assert fallback.route_mask(info, True, "device", 0, png="host").tolist() == [True, True, False, False]
    assert not fallback.route_mask(info, True, "device", 0).any()
    with pytest.raises(ValueError):
        fallback.accept_png(info, "bogus")
    out, n, rm = fallback.hand_over([CASES[0][1], CASES[0][1], b"x", b"y"], info[:, 0], kind=info[:, 3], png="device")
    assert n == 1 and rm.tolist() == [0, 1, 0, 0]

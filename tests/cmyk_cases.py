"""Four-component (Adobe CMYK / YCCK) JPEG test files and the emulator that decodes them
(TEST INFRASTRUCTURE ONLY).

Pillow writes Adobe CMYK only (transform 0, every component 1x1 whatever ``subsampling`` is
asked for: libjpeg's jpeg_set_colorspace gives JCS_CMYK no subsampling), baseline or
progressive.  Everything else — YCCK, subsampled layouts, other markers and scan scripts —
comes from ``encode4``, a four-plane wrapper around ``tests/jpeg_writer.py``'s scan coder.
The expectation for every file is Pillow on the same bytes (``pillow_rgb``), so the encoder
only has to be valid.
"""

from __future__ import annotations

import ctypes
import io
import os
from pathlib import Path

import numpy as np

from tests import jpeg_writer as jw

ROOT = Path(__file__).resolve().parent.parent
EMU4_SO = ROOT / "tests" / "emu" / "libdino_emu4.so"
P = ctypes.c_void_p

SIZES = [(1, 1), (8, 8), (17, 9), (33, 31), (70, 50)]  # (width, height)
S11 = ((1, 1),) * 4
S10 = ((2, 2), (1, 1), (1, 1), (2, 2))     # 10 blocks per MCU: libjpeg's limit
SK1 = ((2, 2), (1, 1), (1, 1), (1, 1))     # K at 1x1 under a 2x2 Y
S12 = ((2, 2), (2, 1), (2, 1), (2, 2))     # 12 blocks: only in per-component scans


def build_emu4() -> ctypes.CDLL:
    """tests/emu/emu4.cpp by the recipe of helpers.build_emu (host-only hipcc)."""
    src = ROOT / "tests" / "emu" / "emu4.cpp"
    deps = [src, *sorted((ROOT / "dataloader_amd" / "csrc").glob("*.hpp")), ROOT / "include" / "dino_ingest.h"]
    if not EMU4_SO.exists() or EMU4_SO.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        cmd = f"hipcc --cuda-host-only -O2 -ffp-contract=off -fPIC -shared -o {EMU4_SO} {src}"
        if os.system(cmd) != 0:
            raise RuntimeError(f"emulator build failed: {cmd}")
    lib = ctypes.CDLL(str(EMU4_SO))
    lib.emu4_decode.argtypes = [P, ctypes.c_int64, P]
    lib.emu4_parse.argtypes = [P, ctypes.c_int64, ctypes.c_int, P]
    lib.emu4_four_to_rgb.argtypes = [P, ctypes.c_int64, ctypes.c_int, P]
    return lib


def planes4(w: int, h: int, seed: int) -> np.ndarray:
    """H x W x 4 uint8: smooth gradients plus noise, so that every plane has DC and AC content."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((h, w, 4), np.float64)
    for c in range(4):
        a, b, p = rng.uniform(-3, 3, 3)
        out[..., c] = 128 + 90 * np.sin(a * x / 9.0 + b * y / 7.0 + p) + rng.normal(0, 12, (h, w))
    return np.clip(np.round(out), 0, 255).astype(np.uint8)


def adobe_segment(transform: int | None, short: bool = False) -> bytes:
    """APP14: "Adobe", version 100, flags0, flags1, transform (12 bytes); ``short``: 11 bytes, which
    libjpeg does not take for an Adobe marker (examine_app14: APP14_DATA_LEN)."""
    body = b"Adobe" + (100).to_bytes(2, "big") + b"\x00\x00\x00\x00"
    return jw._seg(0xEE, body if short else body + bytes([transform]))


def encode4(img: np.ndarray, scans: list[dict], samp=S11, quality: int = 90, progressive: bool = False, restart=0,
            adobe: int | None = 0, adobe_short: bool = False, jfif: bool = False, comp_ids=(1, 2, 3, 4), table_hook=None) -> bytes:
    """A four-component JPEG of the planes ``img`` (H x W x 4, stored as they are: what they mean is
    the decoder's business) with an explicit scan script (``jpeg_writer.scan``); ``table_hook`` as
    in ``jpeg_writer.encode``."""
    H, W, _ = img.shape
    mh, mv = max(s[0] for s in samp), max(s[1] for s in samp)
    mx, my = -(-W // (8 * mh)), -(-H // (8 * mv))
    dims, coefs, qts = [], [], []
    for c in range(4):
        h, v = samp[c]
        dw, dh = -(-W * h // mh), -(-H * v // mv)
        p = img[..., c].astype(np.float64)
        fh, fv = mh // h, mv // v
        if fh > 1 or fv > 1:
            pp = np.pad(p, ((0, (-H) % fv), (0, (-W) % fh)), mode="edge")
            p = pp.reshape(pp.shape[0] // fv, fv, pp.shape[1] // fh, fh).mean(axis=(1, 3))
        p = np.clip(np.round(p), 0, 255)[:dh, :dw]
        q = jw.quant_table(jw.STD_LUMA_Q if c in (0, 3) else jw.STD_CHROMA_Q, quality)
        coefs.append(jw._component_coefs(p, mx * h, my * v, q))
        dims.append((dw, dh))
        qts.append(q)
    frame = {"dims": dims, "samp": list(samp), "mcus": (mx, my), "progressive": progressive}
    out = bytearray(b"\xff\xd8")
    if jfif:
        out += jw._seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if adobe is not None or adobe_short:
        out += adobe_segment(adobe, adobe_short)
    for t in range(2):
        out += jw._seg(0xDB, bytes([t]) + bytes(int(qts[t][jw.ZIGZAG[z]]) for z in range(64)))
    payload = bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([4])
    for c in range(4):
        payload += bytes([comp_ids[c], (samp[c][0] << 4) | samp[c][1], 0 if c in (0, 3) else 1])
    out += jw._seg(0xC2 if progressive else 0xC0, payload)
    if restart:
        out += jw._seg(0xDD, int(restart).to_bytes(2, "big"))
    for sc in scans:
        counter = jw._ScanCoder(False)
        jw._code_scan(frame, coefs, sc, counter, restart)
        tables, dht, slot_ids = {}, bytearray(), {}
        for slot in sorted(counter.freq):
            kind, k = slot
            slot_ids[slot] = k
            bits, vals = (jw.optimal_table(counter.freq[slot]) if table_hook is None
                          else table_hook(kind, k, counter.freq[slot]))
            dht += bytes([(0 if kind == "dc" else 16) | k]) + bytes(bits) + bytes(vals)
            tables[slot] = jw.canonical_codes(bits, vals)
        if dht:
            out += jw._seg(0xC4, bytes(dht))
        segs = jw._code_scan(frame, coefs, sc, jw._ScanCoder(True, tables), restart)
        comps = sc["comps"]
        sos = bytes([len(comps)])
        for k, c in enumerate(comps):
            sos += bytes([comp_ids[c], (slot_ids.get(("dc", k), 0) << 4) | slot_ids.get(("ac", 0 if progressive else k), 0)])
        sos += bytes([sc["ss"], sc["se"], (sc["ah"] << 4) | sc["al"]]) if progressive else bytes([0, 63, 0])
        out += jw._seg(0xDA, sos)
        for i, s in enumerate(segs):
            out += s
            if i + 1 < len(segs):
                out += bytes([0xFF, 0xD0 + (i % 8)])
    out += b"\xff\xd9"
    return bytes(out)


ONE_SCAN = [jw.scan((0, 1, 2, 3))]
PER_COMP = [jw.scan((c,)) for c in range(4)]


def progression4(interleaved_dc: bool = True) -> list[dict]:
    """Successive approximation refined to full precision (no block smoothing): DC al 1 then
    refined, every component's AC in two bands at al 1 then refined."""
    dc = [(0, 1, 2, 3)] if interleaved_dc else [(c,) for c in range(4)]
    s = [jw.scan(c, 0, 0, 0, 1) for c in dc]
    for c in range(4):
        s += [jw.scan((c,), 1, 5, 0, 1), jw.scan((c,), 6, 63, 0, 1)]
    s += [jw.scan(c, 0, 0, 1, 0) for c in dc]
    s += [jw.scan((c,), 1, 63, 1, 0) for c in range(4)]
    return s


def pillow_cmyk(w: int, h: int, seed: int, **save) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(planes4(w, h, seed), "CMYK").save(buf, format="JPEG", quality=90, **save)
    return buf.getvalue()


def pillow_rgb(jpeg: bytes) -> np.ndarray | None:
    """``Image.open(b).convert("RGB")`` (reference cpu.py:251), None where it raises."""
    from PIL import Image
    try:
        return np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))
    except Exception:  # noqa: BLE001 - mirrors cpu.py:252
        return None


_CASES: dict | None = None


def cases() -> dict[str, bytes]:
    """name -> file.  Built once per process."""
    global _CASES
    if _CASES is not None:
        return _CASES
    c: dict[str, bytes] = {}
    for i, (w, h) in enumerate(SIZES):
        c[f"pil_base_{w}x{h}"] = pillow_cmyk(w, h, 10 + i)
        c[f"ycck_11_{w}x{h}"] = encode4(planes4(w, h, 20 + i), ONE_SCAN, adobe=2)
        c[f"ycck_10blk_{w}x{h}"] = encode4(planes4(w, h, 30 + i), ONE_SCAN, samp=S10, adobe=2)
    c["pil_prog_33x31"] = pillow_cmyk(33, 31, 40, progressive=True)
    c["pil_prog_70x50"] = pillow_cmyk(70, 50, 41, progressive=True)
    c["pil_sub2_70x50"] = pillow_cmyk(70, 50, 42, subsampling=2)
    c["cmyk_10blk_70x50"] = encode4(planes4(70, 50, 50), ONE_SCAN, samp=S10, adobe=0)
    c["ycck_k1_33x31"] = encode4(planes4(33, 31, 51), ONE_SCAN, samp=SK1, adobe=2)
    c["cmyk_k1_70x50"] = encode4(planes4(70, 50, 52), ONE_SCAN, samp=SK1, adobe=0)
    c["ycck_12blk_one_scan_33x31"] = encode4(planes4(33, 31, 53), ONE_SCAN, samp=S12, adobe=2)  # Pillow raises
    c["ycck_12blk_per_comp_33x31"] = encode4(planes4(33, 31, 53), PER_COMP, samp=S12, adobe=2)
    c["ycck_12blk_per_comp_70x50"] = encode4(planes4(70, 50, 54), PER_COMP, samp=S12, adobe=2)
    # markers
    c["adobe_t1_33x31"] = encode4(planes4(33, 31, 60), ONE_SCAN, adobe=1)
    c["no_adobe_33x31"] = encode4(planes4(33, 31, 61), ONE_SCAN, adobe=None)
    c["jfif_no_adobe_33x31"] = encode4(planes4(33, 31, 62), ONE_SCAN, adobe=None, jfif=True)
    c["jfif_adobe_t2_17x9"] = encode4(planes4(17, 9, 63), ONE_SCAN, adobe=2, jfif=True)
    c["adobe_11_bytes_33x31"] = encode4(planes4(33, 31, 64), ONE_SCAN, adobe=None, adobe_short=True)
    # scripts
    c["cmyk_per_comp_70x50"] = encode4(planes4(70, 50, 70), PER_COMP, adobe=0)
    c["ycck_prog_sa_10blk_70x50"] = encode4(planes4(70, 50, 71), progression4(), samp=S10, adobe=2, progressive=True)
    c["cmyk_prog_sa_17x9"] = encode4(planes4(17, 9, 72), progression4(False), adobe=0, progressive=True)
    c["ycck_prog_sa_12blk_33x31"] = encode4(planes4(33, 31, 73), progression4(False), samp=S12, adobe=2,
                                             progressive=True)
    c["ycck_rst1_10blk_70x50"] = encode4(planes4(70, 50, 74), ONE_SCAN, samp=S10, adobe=2, restart=1)
    c["ycck_rst_row_10blk_70x50"] = encode4(planes4(70, 50, 75), ONE_SCAN, samp=S10, adobe=2, restart=5)  # 5 MCUs a row
    c["cmyk_rst_row_per_comp_70x50"] = encode4(planes4(70, 50, 76), PER_COMP, adobe=0, restart=9)  # 9 blocks a row
    base = c["pil_base_70x50"]
    c["truncated_mid_scan_70x50"] = base[: len(base) * 2 // 3]  # Pillow raises (LOAD_TRUNCATED_IMAGES unset)
    _CASES = c
    return c


def emu4_decode(lib, jpeg: bytes, w: int, h: int):
    """(status, H x W x 3) from the host model with the four-component option on."""
    buf = np.frombuffer(jpeg, np.uint8)
    out = np.zeros(max(h * w * 3, 1), np.uint8)
    r = lib.emu4_decode(buf.ctypes.data_as(P), len(jpeg), out.ctypes.data_as(P))
    return r, out[: h * w * 3].reshape(h, w, 3)


def size_of(jpeg: bytes) -> tuple[int, int]:
    """(width, height) from the SOF marker (Pillow may refuse the file)."""
    i = 2
    while i + 9 < len(jpeg):
        if jpeg[i] == 0xFF and jpeg[i + 1] in (0xC0, 0xC1, 0xC2):
            return int.from_bytes(jpeg[i + 7:i + 9], "big"), int.from_bytes(jpeg[i + 5:i + 7], "big")
        i += 2 + int.from_bytes(jpeg[i + 2:i + 4], "big") if jpeg[i] == 0xFF and jpeg[i + 1] not in (0xD8,) else 1
    raise ValueError("no SOF")

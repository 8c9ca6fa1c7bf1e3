"""Shared test helpers: oracle <-> ABI record conversion, emulator binding."""

from __future__ import annotations

import ctypes
import io
import os
from pathlib import Path

import numpy as np

from dataloader_amd.params import VIEW_PARAMS_DTYPE
from oracle.cpu_ref import ViewParams

ROOT = Path(__file__).resolve().parent.parent
EMU_SO = ROOT / "tests" / "emu" / "libdino_emu.so"
P = ctypes.c_void_p


def record_to_params(rec) -> ViewParams:
    names = rec.dtype.names or ()

    def opt(k):  # records saved before the window fields existed (golden fixtures) have none
        return int(rec[k]) if k in names else 0

    return ViewParams(
        out_size=int(rec["out_size"]), crop_top=int(rec["crop_top"]), crop_left=int(rec["crop_left"]),
        crop_h=int(rec["crop_h"]), crop_w=int(rec["crop_w"]), flip=bool(rec["flip"]),
        jitter=bool(rec["jitter"]), order=tuple(int(x) for x in rec["order"]),
        brightness=float(rec["brightness"]), contrast=float(rec["contrast"]),
        saturation=float(rec["saturation"]), hue=float(rec["hue"]), gray=bool(rec["gray"]),
        blur=bool(rec["blur"]), sigma=float(rec["sigma"]), ksize=int(rec["ksize"]),
        solarize=bool(rec["solarize"]), resize_w=opt("resize_w"), resize_h=opt("resize_h"),
        out_x=opt("out_x"), out_y=opt("out_y"))


def params_to_record(p: ViewParams) -> np.ndarray:
    r = np.zeros((), VIEW_PARAMS_DTYPE)
    r["out_size"] = p.out_size
    r["crop_top"], r["crop_left"], r["crop_h"], r["crop_w"] = p.crop_top, p.crop_left, p.crop_h, p.crop_w
    r["flip"], r["jitter"], r["gray"], r["blur"], r["solarize"] = p.flip, p.jitter, p.gray, p.blur, p.solarize
    r["order"] = np.asarray(p.order, np.uint8)
    r["brightness"], r["contrast"], r["saturation"], r["hue"] = p.brightness, p.contrast, p.saturation, p.hue
    r["sigma"], r["ksize"] = p.sigma, p.ksize
    r["resize_w"], r["resize_h"], r["out_x"], r["out_y"] = p.resize_w, p.resize_h, p.out_x, p.out_y
    return r


def build_emu() -> ctypes.CDLL:
    src = ROOT / "tests" / "emu" / "emu.cpp"
    deps = [src, ROOT / "tests" / "emu" / "models.hpp", *sorted((ROOT / "dataloader_amd" / "csrc").glob("*.hpp"))]
    if not EMU_SO.exists() or EMU_SO.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        # host-only: the emulator runs the device functions on the CPU (no device pass)
        cmd = (f"hipcc --cuda-host-only -O2 -ffp-contract=off -fPIC -shared -o {EMU_SO} {src}")
        if os.system(cmd) != 0:
            raise RuntimeError(f"emulator build failed: {cmd}")
    return ctypes.CDLL(str(EMU_SO))


def emu_decode(lib, jpeg: bytes, mode: int = 0, lanes: int = 1):
    from PIL import Image
    buf = np.frombuffer(jpeg, np.uint8)
    # the emulator writes width x height of its own parse (and nothing when that fails): a file
    # that Pillow refuses but the parser accepts still gets a buffer of its real size
    info = np.zeros(8, np.int32)
    if lib.emu_parse(buf.ctypes.data_as(P), ctypes.c_int64(len(jpeg)), info.ctypes.data_as(P)) == 0:
        w, h = int(info[1]), int(info[2])
    else:
        try:
            w, h = Image.open(io.BytesIO(jpeg)).size
        except Exception:  # noqa: BLE001
            w, h = 1, 1
    out = np.zeros(h * w * 3, np.uint8)
    st = np.zeros(4, np.int32)
    r = lib.emu_decode(buf.ctypes.data_as(P), ctypes.c_int64(len(jpeg)), mode, lanes,
                       out.ctypes.data_as(P), st.ctypes.data_as(P))
    return r, out.reshape(h, w, 3), st


def emu_augment(lib, rgb: np.ndarray, rec, mean, std, out_dtype: int = 0):
    import torch
    H, W, _ = rgb.shape
    S = int(rec["out_size"])
    rgb = np.ascontiguousarray(rgb)
    m = np.asarray(mean, np.float32)
    s = np.asarray(std, np.float32)
    recarr = np.asarray(rec, VIEW_PARAMS_DTYPE).reshape(1)
    if out_dtype == 0:
        out = np.zeros(3 * S * S, np.uint16)
    elif out_dtype == 1:
        out = np.zeros(3 * S * S, np.float32)
    else:
        out = np.zeros(3 * S * S, np.uint8)
    lib.emu_augment_view(rgb.ctypes.data_as(P), W, H, recarr.ctypes.data_as(P), m.ctypes.data_as(P),
                         s.ctypes.data_as(P), out_dtype, out.ctypes.data_as(P))
    t = torch.from_numpy(out.reshape(3, S, S).copy())
    if out_dtype == 0:
        return t.view(torch.bfloat16)
    if out_dtype == 2:
        return t.view(torch.float8_e4m3fn)
    return t


def emu_resized_crop(lib, rgb: np.ndarray, rec) -> np.ndarray:
    H, W, _ = rgb.shape
    S = int(rec["out_size"])
    rgb = np.ascontiguousarray(rgb)
    recarr = np.asarray(rec, VIEW_PARAMS_DTYPE).reshape(1)
    out = np.zeros(S * S * 3, np.uint8)
    lib.emu_resized_crop(rgb.ctypes.data_as(P), W, H, recarr.ctypes.data_as(P), out.ctypes.data_as(P))
    return out.reshape(S, S, 3)


def hresize_tile(lib, S: int, cw: int, ch: int = 1):
    """k_hresize's tile shape for a cw x ch crop at view size S, from the kernel's own
    functions: (sw, pitch, R, R3p, work items, tap groups).  R == 0 is the direct path."""
    kh = lib.emu_resample_ksize(cw, S)
    out = (ctypes.c_int32 * 5)()
    lib.emu_hresize_tile(S, cw, ch, kh, out)
    return (*out, (kh + 3) // 4)


VIEW_SCRATCH_FIELDS = ("htmp", "hb", "vb", "ht", "vt", "hx", "hg", "total")
DEC_SCRATCH_FIELDS = ("hb", "ht", "vb", "vt", "htmp", "total")


def view_scratch(lib, S: int, crop_h: int, kh: int, kv: int) -> dict[str, int]:
    """A view's augment scratch layout (plan.hpp view_scratch): byte offsets from its base."""
    out = (ctypes.c_int64 * 8)()
    lib.emu_view_scratch(S, crop_h, kh, kv, out)
    return dict(zip(VIEW_SCRATCH_FIELDS, out))


def view_vcoefs(lib, S: int, kh: int, kv: int) -> tuple[int, int]:
    """Byte offsets (vb, vt) of the vertical pass's tables as vert_apply takes them
    (plan.hpp view_vcoefs), from the start of the view's coefficient block."""
    out = (ctypes.c_int64 * 2)()
    lib.emu_view_vcoefs(S, kh, kv, out)
    return int(out[0]), int(out[1])


def dec_scratch(lib, ow: int, oh: int, H: int, kh: int, kv: int) -> dict[str, int]:
    """A decode-only image's scratch layout (plan.hpp dec_scratch): byte offsets from its base."""
    out = (ctypes.c_int64 * 6)()
    lib.emu_dec_scratch(ow, oh, H, kh, kv, out)
    return dict(zip(DEC_SCRATCH_FIELDS, out))


def dec_scratch_total(lib, w: int, h: int, ow: int, oh: int) -> int:
    """Exact scratch bytes of a w x h image resized to ow x oh by the decode-only recipe."""
    return dec_scratch(lib, ow, oh, h, lib.emu_resample_ksize(w, ow), lib.emu_resample_ksize(h, oh))["total"]


SWEEP_SIZES = (30, 96, 128, 132, 224, 518, 1024)
SWEEP_MAX_WIDTH = 2048          # widest raw image of the two large view sizes
SWEEP_DIRECT_SIZES = (30, 96, 224)  # view sizes whose list goes on to the direct-path pair
SWEEP_WALK_LIMIT = 20000        # the view sizes <= 256 are on the direct path well before


def hresize_shape_table(lib, S: int):
    """[(first width, last width, sw, R)] of every (sw, R) shape as the crop width rises from
    1 to the first direct-path width (whose entry, R == 0, ends the table; for S > 256 the
    walk ends at SWEEP_MAX_WIDTH instead, the last entry cut there), and the first width with
    more than 8 tap groups (the generic group loop).  crop_w == S has no horizontal pass and
    belongs to no shape."""
    table, first_ng = [], None
    for cw in range(1, SWEEP_MAX_WIDTH + 1 if S > 256 else SWEEP_WALK_LIMIT):
        if cw == S:
            continue
        sw, _, R, _, _, ng = hresize_tile(lib, S, cw)
        if first_ng is None and ng > 8 and R > 0:
            first_ng = cw
        if not table or table[-1][2:] != (sw, R):
            table.append((cw, cw, sw, R))
        else:
            table[-1] = (table[-1][0], cw, sw, R)
        if R == 0:
            return table, first_ng
    assert S > 256, f"S={S}: no direct-path width below {SWEEP_WALK_LIMIT}"
    return table, first_ng


def resample_sweep_widths(lib, S: int) -> list[int]:
    """Crop widths that pin every tile shape of k_hresize at view size S: the first and the
    last width of each (sw, R) shape and the first width with more than 8 tap groups;
    up to SWEEP_MAX_WIDTH for S > 256, up to the last staged shape for the others, and the
    direct-path pair (last staged width, first direct width) for SWEEP_DIRECT_SIZES."""
    table, first_ng = hresize_shape_table(lib, S)
    ws = set()
    for first, last, _, R in table:
        if R == 0:
            if S in SWEEP_DIRECT_SIZES:
                ws.add(first)
            continue
        ws.update((first, last))
    if first_ng is not None:
        ws.add(first_ng)
    return sorted(ws)


def saturating_rgb(w: int, h: int, rng) -> np.ndarray:
    """Content whose bicubic resample overshoots 0 and 255 (it must clip), in four bands of
    rows: independent 0/255 bits per channel, a 1-px checkerboard, 0/255 stripes of period 3
    along x, and uniform u8 noise."""
    img = np.empty((h, w, 3), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    q = [h * k // 4 for k in range(5)]
    img[q[0]:q[1]] = rng.integers(0, 2, size=(q[1] - q[0], w, 3), dtype=np.uint8) * 255
    img[q[1]:q[2]] = (((xx + yy) & 1) * 255).astype(np.uint8)[q[1]:q[2], :, None]
    img[q[2]:q[3]] = ((xx % 3 == 0) * 255).astype(np.uint8)[q[2]:q[3], :, None]
    img[q[3]:q[4]] = rng.integers(0, 256, size=(q[4] - q[3], w, 3), dtype=np.uint8)
    return img


def pillow_bicubic_row_unclipped(row: np.ndarray, out_size: int) -> np.ndarray:
    """One row through Pillow's BICUBIC coefficient formula (Resample.c precompute_coeffs,
    a = -0.5, normalised weights) in float64, without the 8-bit clip."""
    def f(x):
        x = np.abs(x)
        return np.where(x < 1.0, ((1.5 * x - 2.5) * x) * x + 1.0,
                        np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5, 0.0))
    n = len(row)
    scale = n / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    out = np.empty(out_size)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        x0 = max(0, int(center - support + 0.5))
        x1 = min(n, int(center + support + 0.5))
        k = f((np.arange(x0, x1) - center + 0.5) / fs)
        out[xx] = float(np.dot(k / k.sum(), row[x0:x1].astype(np.float64)))
    return out


def dc_extremes_rgb(w: int, h: int, rng, cell: int = 16) -> np.ndarray:
    """Saturated colour cells (black/white/blue/yellow/red/cyan) in cell x cell squares:
    neighbouring blocks differ by DC categories 10-11 in luma and chroma, whose chroma
    codes are longer than the DC lookahead (the decoder's slow path)."""
    pal = np.array([[0, 0, 0], [255, 255, 255], [0, 0, 255], [255, 255, 0], [255, 0, 0], [0, 255, 255]], np.uint8)
    idx = rng.integers(0, len(pal), size=((h + cell - 1) // cell, (w + cell - 1) // cell))
    img = pal[np.repeat(np.repeat(idx, cell, axis=0), cell, axis=1)[:h, :w]]
    return np.ascontiguousarray(img)

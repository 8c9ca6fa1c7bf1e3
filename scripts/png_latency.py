"""Latency of the PNG kernels (``dino_set_timing``, kernel id "k_png": k_pnghead + k_pngwalk +
k_inflate + k_unfilter): one 640 x 480 RGB PNG at Pillow's default compression decoded alone,
and a pool of 512 distinct such files in one batch.  Prints one JSON line.

    python scripts/png_latency.py [--reps 20]
"""

import argparse
import io
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from dataloader_amd.engine import IngestEngine, pack_jpegs  # noqa: E402
from dataloader_amd.synthetic import textured_rgb  # noqa: E402


def png_of(seed: int) -> bytes:
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(textured_rgb(640, 480, np.random.default_rng(seed))).save(b, "PNG")
    return b.getvalue()


def timed(eng, files, reps):
    buf, off = pack_jpegs(files, pin=True)
    d_bytes, d_off = buf.to(eng.device), off.to(eng.device)
    eng.reserve(len(files) * (8 << 20), 0)
    info = eng.decode(d_bytes, d_off, len(files))  # warm-up
    torch.cuda.synchronize()
    assert (info[:, 0] == 0).all().item()
    eng.set_timing(True)
    for _ in range(reps):
        eng.decode(d_bytes, d_off, len(files))
    torch.cuda.synchronize()
    ms, n = eng.kernel_times()["k_png"]
    eng.set_timing(False)
    return ms / reps, n // reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pool", type=int, default=512)
    a = ap.parse_args()
    files = [png_of(s) for s in range(a.pool)]
    eng = IngestEngine(0, max_batch=a.pool, max_views=10, max_crop_size=224)
    eng.set_png(True)
    one_ms, launches = timed(eng, files[:1], a.reps)
    pool_ms, _ = timed(eng, files, max(2, a.reps // 4))
    eng.close()
    print(json.dumps({"png_640x480_mean_bytes": int(np.mean([len(f) for f in files])), "one_image_ms": round(one_ms, 3),
                      "pool": a.pool, "pool_ms": round(pool_ms, 3), "pool_ms_per_image": round(pool_ms / a.pool, 4),
                      "launches_per_decode": launches}))


if __name__ == "__main__":
    main()

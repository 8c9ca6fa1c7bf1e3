"""Latency of one 640x480 image through the lossless-WebP kernels beside the same pixels as a PNG
through the PNG kernels, on one build: the "k_png" timer slot (every kernel of the format, HIP
events) per decode call.  python scripts/webp_latency.py [reps]
With --lossy: the same image as a quality-75 lossy WebP through the VP8 kernels instead
(webp_forms), checked against Pillow's decode of that file."""

import io
import sys
from pathlib import Path

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from dataloader_amd import fallback  # noqa: E402
from dataloader_amd.engine import IngestEngine, pack_jpegs  # noqa: E402
from dataloader_amd.tario import spans_of  # noqa: E402


def main():
    lossy = "--lossy" in sys.argv[1:]
    args = [a for a in sys.argv[1:] if a != "--lossy"]
    reps = int(args[0]) if args else 20
    dev = torch.device("cuda", 0)
    im = Image.open(Path(__file__).resolve().parents[1] / "tests" / "golden" / "prog_640x480.jpg").convert("RGB")
    files = {}
    for fmt, kw in ((("WEBP", {"quality": 75}),) if lossy else (("WEBP", {"lossless": True, "method": 4}), ("PNG", {}))):
        f = io.BytesIO()
        im.save(f, fmt, **kw)
        files[fmt] = f.getvalue()
    for fmt, data in files.items():
        eng = IngestEngine(dev, max_batch=1, max_views=1, max_crop_size=8)
        eng.set_webp(True) if fmt == "WEBP" else eng.set_png(True)
        ptrs, lens, _keep = spans_of([data])
        if lossy:
            eng.set_webp_forms(True)
        probe = fallback.probe_webp_forms if lossy else fallback.probe_webp
        eng.reserve(int(probe(ptrs, lens)[1].sum()) + (64 << 20), 0)
        buf, off = pack_jpegs([data], pin=True)
        d_bytes, d_off = buf.to(dev), off.to(dev)
        eng.set_timing(True)
        times = []
        for r in range(reps + 3):
            info = eng.decode(d_bytes, d_off, 1).cpu().numpy()
            torch.cuda.synchronize()
            t = eng.kernel_times()["k_png"][0]
            if r >= 3:
                times.append(t)
        got = eng.copy_rgb(0, 640, 480).cpu().numpy()
        ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB")) if lossy else np.asarray(im)
        assert info[0, 0] == 0 and np.array_equal(got, ref), fmt
        eng.close()
        print(f"{fmt}: {len(data)} bytes, k_png slot per decode: median {np.median(times):.3f} ms, "
              f"min {min(times):.3f}, max {max(times):.3f} over {reps} decodes")


if __name__ == "__main__":
    main()

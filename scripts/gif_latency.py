"""Latency of one 640x480 GIF (256 colours, Pillow's encoder) through the GIF kernels, the "k_png"
timer slot (every kernel of the format, HIP events) per decode call, beside Pillow's decode of the
same bytes on the host.  python scripts/gif_latency.py [reps]"""

import io
import sys
import time
from pathlib import Path

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from dataloader_amd import fallback  # noqa: E402
from dataloader_amd.engine import IngestEngine, pack_jpegs  # noqa: E402
from dataloader_amd.tario import spans_of  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda", 0)
    im = Image.open(Path(__file__).resolve().parents[1] / "tests" / "golden" / "prog_640x480.jpg").convert("RGB")
    f = io.BytesIO()
    im.quantize(256).save(f, "GIF")
    data = f.getvalue()
    ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        host.append((time.perf_counter() - t0) * 1e3)
    eng = IngestEngine(dev, max_batch=1, max_views=1, max_crop_size=8)
    eng.set_gif(True)
    ptrs, lens, _keep = spans_of([data])
    eng.reserve(int(fallback.probe_gif(ptrs, lens)[1].sum()) + (64 << 20), 0)
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
    assert info[0, 0] == 0 and np.array_equal(got, ref)
    eng.close()
    print(f"GIF: {len(data)} bytes, k_png slot per decode: median {np.median(times):.3f} ms, "
          f"min {min(times):.3f}, max {max(times):.3f} over {reps} decodes; "
          f"Pillow on the host: median {np.median(host):.3f} ms, min {min(host):.3f}")


if __name__ == "__main__":
    main()

"""bench.py with the PNG option forced on: every context the benchmark creates gets
``dino_ctx_set_png(1)``, so each decode launches the four PNG kernels over a batch that holds no
PNG.  Shows what those empty launches cost (RESULTS.md); the arguments are bench.py's.

    python scripts/png_forced_on.py --gpus 1 --steps 40 --warmup 10 [--mixed]
"""

import runpy
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from dataloader_amd import engine  # noqa: E402

_init = engine.IngestEngine.__init__


def _init_png(self, *a, **kw):
    _init(self, *a, **kw)
    self.set_png(True)


engine.IngestEngine.__init__ = _init_png
sys.argv[0] = str(ROOT / "bench.py")
runpy.run_path(sys.argv[0], run_name="__main__")

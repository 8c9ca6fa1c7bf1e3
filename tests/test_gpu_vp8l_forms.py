"""VP8L stream forms libwebp's encoder never emits, on the device (``webp="device"``): the files
of tests/vp8l_form_cases.py against Pillow bit for bit with damaged files between sound ones, and
the 3 KiB payload at every alignment of the input ring.  (The two files the probe declines for
their group count are pinned on the CPU, in test_vp8l_forms_cpu.py.)"""

import faulthandler

import numpy as np
import pytest

from tests import png_cases as pc
from tests import vp8l_form_cases as fc
from tests.test_gpu_webp import _decode

pytestmark = pytest.mark.gpu

CASES = fc.cases()
LIMIT_S = 120  # a test here takes a few seconds


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with every thread's stack) instead of the run's time."""
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _mismatches(eng, form, info, files, refs):
    """Status first, then width and height, then the pixels: every mismatch of the batch."""
    bad = []
    for i, (data, ref) in enumerate(zip(files, refs)):
        want = {0: -1, 1: 1, 2: 0 if ref is not None else -1}[int(form[i, 0])]
        if int(info[i, 0]) != want:
            bad.append((i, "status", int(info[i, 0]), want))
        elif want == 0 and tuple(info[i, 1:3]) != ref.shape[1::-1]:
            bad.append((i, "size", tuple(info[i, 1:3]), ref.shape[1::-1]))
        elif want == 0:
            got = eng.copy_rgb(i, ref.shape[1], ref.shape[0]).cpu().numpy()
            if not np.array_equal(got, ref):
                bad.append((i, "pixels", int((got != ref).sum())))
    return bad


def test_every_form_bit_exact_with_pillow(gpu_device):
    """Every case the device takes in one batch, with three files damaged past their prologue
    (a back-reference before the first pixel, one past the last, a stream one bit short) between
    sound ones: status -1 for those, Pillow's pixels for all others."""
    names = [c[0] for c in CASES if c[2] == "dev"]
    files = [c[1] for c in CASES if c[2] == "dev"]
    broken = [d for d in fc.bad() if d[0] in fc.BODY_ERRORS]
    assert len(broken) == 3
    for at, d in zip((3, 30, 61), broken):
        files[at:at] = [d[1]]
        names[at:at] = [d[0]]
    refs = [pc.pillow_rgb(f) for f in files]
    assert [n for n, r in zip(names, refs) if r is None] == [d[0] for d in broken]
    eng, form, info = _decode(gpu_device, files)
    assert (form[:, 0] == 2).all(), "the damage must lie where only the decode finds it"
    bad = _mismatches(eng, form, info, files, refs)
    eng.close()
    assert not bad, [(names[b[0]],) + b[1:] for b in bad]


def test_ring_refills_at_every_alignment(gpu_device):
    """The 3 KiB payload (several refills of the 1 KiB input ring) at byte offsets 0 to 15 mod 16
    of the batch's buffer, files that are no image between the copies."""
    files = fc.ring_batch()
    refs = [pc.pillow_rgb(f) for f in files]
    assert sum(r is not None for r in refs) == 16
    eng, form, info = _decode(gpu_device, files)
    bad = _mismatches(eng, form, info, files, refs)
    eng.close()
    assert not bad, bad

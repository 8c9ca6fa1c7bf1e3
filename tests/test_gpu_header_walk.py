"""GPU parity of the header walk on the files of ``tests/header_cases.py``: one
``IngestEngine.decode`` batch of the whole list per buffer layout.

k_parse walks a file's first 4096 bytes in an LDS image shifted by the file's address mod 16 and
re-walks a longer header in global memory; near the end of the caller's buffer it copies
bytewise; the spans form takes true lengths.  None of that exists in ``dino_probe``, which runs
the same ``parse_jpeg`` on the host: per file the device status has to equal the probe's status
for the same bytes, its sign has to be Pillow's (0 where the reference decodes, negative where
it raises), and ``copy_rgb`` has to equal Pillow's pixels bit for bit where it decodes.
"""

from __future__ import annotations

import warnings

import numpy as np
import pytest
import torch

from dataloader_amd import fallback
from dataloader_amd.config import DINOAugConfig
from dataloader_amd.engine import IngestEngine, pack_jpegs
from oracle import cpu_ref
from tests import header_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected():
    """Per case of the list, computed once: (Pillow's pixels or None, dino_probe's status)."""
    cases = hc.cases()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the malformed MPF segments Pillow warns about and ignores)
        pix = [cpu_ref.decode_rgb(c.data) for c in cases]
    pix = [None if p is None else np.asarray(p) for p in pix]
    buf, off = pack_jpegs([c.data for c in cases], pin=False)
    info, _, _ = fallback.probe(buf.data_ptr(), off.numpy(), len(cases), 0)
    return {c.name: (p, int(info[i, 0])) for i, (c, p) in enumerate(zip(cases, pix))}


def _differences(eng, info, cases, first, expected):
    """[(name, what, ...)] for every file of the decoded batch (case k is image first + k)."""
    bad = []
    for k, c in enumerate(cases):
        i = first + k
        ref, probe = expected[c.name]
        st = int(info[i, 0])
        if st != probe:
            bad.append((c.name, "status", st, "probe", probe))
        elif ref is None:
            if st >= 0:
                bad.append((c.name, "reference raises; status", st))
        elif st != 0:
            bad.append((c.name, "reference decodes; status", st))
        elif (int(info[i, 1]), int(info[i, 2])) != (ref.shape[1], ref.shape[0]):
            bad.append((c.name, "size", (int(info[i, 1]), int(info[i, 2]))))
        else:
            got = eng.copy_rgb(i, ref.shape[1], ref.shape[0]).cpu().numpy()
            if not np.array_equal(got, ref):
                bad.append((c.name, "bytes differing", int((got != ref).sum())))
    return bad


def _by_name(name):
    return next(c for c in hc.cases() if c.name == name)


# (bytes of the leading pad file, exact-size buffer, name of the case that goes last)
LAYOUTS = [(0, False, "k1_sos_last_at4095"), (1, False, "b420_sos_ff_at4095"), (15, False, "k1_dht_len_at4096"),
           (5, True, "b420_length4095"), (0, True, "b420_length4097")]


@pytest.mark.parametrize("pad,exact,last", LAYOUTS)
def test_whole_list_one_batch(gpu_device, expected, pad, exact, last):
    """The first file at address 0, 1 and 15 mod 16 (a leading pad file, as in
    test_decode_marker_edge_cases), and exact-size buffers whose last file ends inside the last
    prefix chunk, so that k_parse's copy takes its bytewise branch."""
    cases = hc.cases() + [_by_name(last)]
    files = [b"\0" * pad] + [c.data for c in cases]
    buf, off = pack_jpegs(files, pin=False)
    d_bytes = buf.to(gpu_device)
    if exact:
        d_bytes = d_bytes[: int(off[-1])].clone()  # no slack after the last image
        assert len(files[-1]) <= hc.PREFIX + 16
    assert d_bytes.data_ptr() % 16 == 0 and int(off[1]) % 16 == pad
    eng = IngestEngine(gpu_device, max_batch=len(files), max_views=1, max_crop_size=32)
    info = eng.decode(d_bytes, off.to(gpu_device), len(files)).cpu().numpy()
    assert info[0, 0] < 0  # the pad file
    bad = _differences(eng, info, cases, 1, expected)
    eng.close()
    assert not bad, f"{len(bad)} of {len(cases)}: {bad[:12]}"


def test_whole_list_as_spans_with_junk_between(gpu_device, expected):
    """dino_decode_spans: 1..40 bytes of junk (marker bytes among them) between the files and true
    lengths; a walk that read past a file's length would find the next bytes."""
    cases = hc.cases()
    rng = np.random.default_rng(1440)
    chunks, offs, lens, pos = [], [], [], 0
    for c in cases:
        junk = rng.choice(np.frombuffer(b"\xff\xd8\xda\xc0\x00\x10\xe1\xd9", np.uint8), int(rng.integers(1, 41))).tobytes()
        chunks += [junk, c.data]
        offs.append(pos + len(junk))
        lens.append(len(c.data))
        pos += len(junk) + len(c.data)
    offs.append(pos)
    d_bytes = torch.frombuffer(bytearray(b"".join(chunks)), dtype=torch.uint8).to(gpu_device)
    assert {o % 16 for o in offs[:-1]} == set(range(16))
    d_off = torch.tensor(offs, dtype=torch.int64, device=gpu_device)
    d_len = torch.tensor(lens, dtype=torch.int64, device=gpu_device)
    eng = IngestEngine(gpu_device, max_batch=len(cases), max_views=1, max_crop_size=32)
    info = eng.decode(d_bytes, d_off, len(cases), lengths=d_len).cpu().numpy()
    bad = _differences(eng, info, cases, 0, expected)
    eng.close()
    assert not bad, f"{len(bad)} of {len(cases)}: {bad[:12]}"


@pytest.mark.parametrize("lane", [False, True])
def test_multi_scan_cases_under_both_progressive_decoders(gpu_device, expected, lane):
    """Every case on the three-scan sequential and the progressive base under both settings of
    dino_ctx_set_prog_decoder: prog_walk runs in k_pwalk for both."""
    cases = [c for c in hc.cases() if c.pixels_of in ("k1", "prog")]
    assert len(cases) >= 100 and any(c.expect == "raises" for c in cases)
    buf, off = pack_jpegs([c.data for c in cases], pin=False)
    eng = IngestEngine(gpu_device, max_batch=len(cases), max_views=1, max_crop_size=32)
    eng.set_prog_decoder(lane)
    info = eng.decode(buf.to(gpu_device), off.to(gpu_device), len(cases)).cpu().numpy()
    bad = _differences(eng, info, cases, 0, expected)
    eng.close()
    assert not bad, f"{len(bad)} of {len(cases)}: {bad[:12]}"


PIPE_DECODES = ("exif_orient6_under", "icc_three_full_over", "app5_len0_app0_b420", "dqt_pq15_dqt_sof_b420",
                "tem_scans_k1", "b420_sos_last_at4095")
PIPE_RAISES = ("icc_short13_under", "tem_app0_b420", "soi2_sof_sos_b420", "res02_scans_k1", "dri_len6_dqt_sof_b420",
               "ps_ends_after_code_over")


def test_pipeline_views_zero_exactly_where_pillow_raises(gpu_device, expected):
    from dataloader_amd.pipeline import MI355XAugPipeline
    names = [n for pair in zip(PIPE_DECODES, PIPE_RAISES) for n in pair]
    assert all(expected[n][0] is not None for n in PIPE_DECODES) and all(expected[n][0] is None for n in PIPE_RAISES)
    files = [_by_name(n).data for n in names]
    cfg = DINOAugConfig(global_crop_size=32, local_crop_size=16, n_local_crops=2)
    pipe = MI355XAugPipeline(lambda: files, cfg, batch_size=len(files), seed=3, out_dtype="fp32")
    out = pipe.run_one_batch()
    torch.cuda.synchronize()
    bad = []
    for i, n in enumerate(names):
        for v in range(cfg.n_views):
            nz = bool(out[f"view_{v}"][i].any())
            if nz != (n in PIPE_DECODES):
                bad.append((n, v, "non-zero" if nz else "zero"))
    pipe.close()
    assert not bad, bad

"""The C++ adapters with a waterfall detector, end to end on the GPU: tests/level2_mock/run_level2_wf_detector.cpp is
run_level2_gpu.cpp (hip_level2.h's server loop on the real HipFanout) with HipFanout::Params::waterfall_detector set.
The mock waterfall encoder must receive ONE packet per sent frame and client, with the labels the reference sends and
the detector's bytes; with the default Params (run_level2_gpu.cpp itself) it receives the sampled rows, as before.

Expectation: tests/wf_detector_model.py on the per-frame pyramids of a Python-side context that transforms the same raw
stream frame by frame, compared bit for bit."""
import os

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_level2 import _build, _mkdtemp, _parse
from test_gpu_wf_detector import keyed_stream, tone_bin

import wf_detector_model as M

pytestmark = pytest.mark.gpu


def _run(d, exe, N, nfr, wfs, sps):
    with open(os.path.join(d, "script.txt"), "w") as f:
        f.write(f"config 16 0 {sps} s16 0 0 12000 1024 0 0\n")
        for l, r in wfs:
            f.write(f"wf {l} {r}\n")
    import subprocess
    out = os.path.join(d, os.path.basename(exe) + ".out")
    r = subprocess.run([exe, os.path.join(d, "script.txt"), os.path.join(d, "raw.bin"), out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return _parse(out)


def test_level2_adapter_with_peak_detector():
    from oracle import oracle as O
    from phantomsdr_amd import Context
    d = _mkdtemp()
    src = os.path.join(ROOT, "tests", "level2_mock")
    exe_peak = _build(d, os.path.join(src, "run_level2_wf_detector.cpp"), "run_level2_peak", extra=("-DPSDR_TEST_WF_DETECTOR=PSDR_WF_PEAK",))
    exe_default = _build(d, os.path.join(src, "run_level2_gpu.cpp"), "run_level2_default")
    N, nfr, sps = 1 << 16, 40, 2_048_000
    p = O.derived_params(sps, N, False)
    levels, skip = p["downsample_levels"], p["skip_num"]
    assert skip == 6
    raw = keyed_stream(N, False, nfr, 31, keyed_halves=(8, 9, 21))     # bursts inside windows (6, 12] and (18, 24]
    raw.tofile(os.path.join(d, "raw.bin"))
    tb = tone_bin(N, False)
    wfs = [(0, N), (tb - 500, tb + 524)]
    owf = []
    for l, r in wfs:
        lv, nl, nr = O.waterfall_pick_level(levels, 1024, l, r)
        owf.append((lv, nl, min(nr, N >> lv)))
    # the per-frame pyramids, from a context that runs the frames one by one like the adapter
    ctx = Context(N, 0, levels, additional_size=p["audio_fft_size"], audio_fft_size=p["audio_fft_size"], audio_rate=12000,
                  input_format="s16", max_batch=1, max_clients=16, max_waterfall_clients=8, skip_num=skip, waterfall_size=1024)
    try:
        dev = ctx.dev_alloc(raw.nbytes)
        ctx.h2d(dev, raw)
        rows = [[] for _ in owf]
        for f in range(nfr):
            ctx.process_batch(dev, 1, offset_bytes=f * ctx.half_frame_bytes())
            q = ctx.read_quantized(0)
            for i, (lv, l, r) in enumerate(owf):
                rows[i].append(ctx.quantized_level(q, lv)[l:r].copy())
        ctx.dev_free(dev)
    finally:
        ctx.close()
    calls = [(f, 1) for f in range(nfr)]
    sent = [f for f in range(nfr) if f % skip == 0]
    differ = 0
    for exe, det in ((exe_peak, M.PEAK), (exe_default, M.SAMPLE)):
        gn, glevels, gframes, gskip, recs = _run(d, exe, N, nfr, wfs, sps)
        assert (glevels, gframes, gskip) == (levels, nfr, skip)
        wrecs = [q for q in recs if q["kind"] == 1]
        assert sorted((q["client"], q["frame"]) for q in wrecs) == sorted((i, f) for i in range(len(owf)) for f in sent), \
            "one packet per waterfall client and sent frame"
        for i, (lv, l, r) in enumerate(owf):
            want = np.concatenate(M.expected_rows(np.stack(rows[i]), calls, skip, det))
            samp = np.concatenate(M.expected_rows(np.stack(rows[i]), calls, skip, M.SAMPLE))
            for si, f in enumerate(sent):
                g = next(q for q in wrecs if q["client"] == i and q["frame"] == f)
                assert (g["l"], g["r"]) == (l << lv, r << lv)
                assert np.array_equal(g["data"].astype(np.int8), want[si]), (DETN[det], i, f)
                if det == M.PEAK:
                    differ += int(not np.array_equal(want[si], samp[si]))
    assert differ >= 4, "PEAK never differed from SAMPLE: the run would prove nothing"


DETN = {M.SAMPLE: "sample", M.PEAK: "peak"}

"""The CW decoder on the GPU at every hop length, at long frames and at frames that complete no hop (the cases, the input, the
batches and the conditions: tests/decoder_shapes.py).

Per case one context with that audio_rate and audio_fft_size, a filler AM client in slot 0 and the decoded USB client in slot 1, run
whole and split.  Expected, without a tolerance: the two runs' rows and NaN flags are the same bits, and every frame's record, the
text and its length are tests/cw_model.py's records() on those rows and flags - anchored to the host program at these shapes by
tests/test_decoder_shapes_host.py.  The table's conditions are evaluated on the model's records.  At every case but h = 6 the
text read is the text sent and the pitch is within one lane of the carrier's."""
import functools

import numpy as np
import pytest

import cw_model as M
import decoder_shapes as S
from helpers import assert_same_bits, read_client
from test_gpu_cw_decoder import rec_of

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def run(rate, n, whole):
    nf = S.cw_timing(rate, n)[0]
    batches = (nf,) if whole else S.split_of(nf, n // 2)
    A = S.open_ctx(rate, n, max(batches), S.cw_raw(rate, n))
    try:
        A.add("AM")
        g = A.add("USB", cw=S.CW_CFG)
        A.ctx.set_profiling(1)
        a, t = [], []
        for F in batches:
            A.batch(F)
            a.append(read_client(g, "USB", F)), t.append(g.read_cw(F))
        return S.cat(a), S.cat(t), g.read_cw_text(), A.ctx.kernel_stats(), batches
    finally:
        A.close()


@pytest.mark.parametrize("rate,n", S.CW_CASES)
def test_records_and_text_are_the_models_at_every_hop_and_frame_length(rate, n):
    h = n // 2
    nf = S.cw_timing(rate, n)[0]
    (rows, _, nan), _, _, _, _ = run(rate, n, True)
    assert rows.shape == (nf, h) and nan.any()
    want, wtext = M.records(rows, nan, h, rate, **S.CW_CFG)
    figures = {}
    for whole in (True, False):
        (r, _, f), t, (text, total), stats, batches = run(rate, n, whole)
        assert_same_bits((r, f), (rows, nan), "the rows of the two runs", ("audio", "nan"))
        got = rec_of(t)
        ms, cnt = stats["audio_cw"]
        print(f"rate {rate} n {n} batches {batches}: text {text!r} wpm {got['wpm'][-1]:.2f} pitch {got['pitch_hz'][-1]} level {got['level'].max():.4g}; "
              f"{cnt} launches, {1e3 * ms / max(cnt, 1):.1f} us each")
        figures.update({("whole" if whole else "split") + "_launches": int(cnt), ("whole" if whole else "split") + "_us_per_launch": 1e3 * ms / max(cnt, 1)})
        bad = [k for k in range(nf) if got[k].tobytes() != want[k].tobytes()]
        assert not bad, (batches, bad[:8], got[bad[:4]], want[bad[:4]])
        assert text == wtext and total == len(wtext) == got["nchars"][-1] and cnt == len(batches)
    S.record("cw", rate=rate, n=n, frames=nf, **figures)
    broken = S.cw_rules(rate, h, batches, want, wtext, nan)
    assert not broken, broken
    if (rate, n) in S.CW_TRUTH:
        assert wtext == S.TEXT and abs(want["pitch_hz"][-1] - S.PITCH) <= M.DF

"""The tone decoder on the GPU at its shortest and longest window, at long frames and at frames that complete no block (the cases,
the input, the batches and the conditions: tests/decoder_shapes.py).

Per case one context with that audio_rate and audio_fft_size, a filler AM client in slot 0 and the decoded USB client in slot 1, run
whole and split.  Expected, without a tolerance: the two runs' rows and NaN flags are the same bits, and every frame's record is
tests/tone_model.py's records() on those rows and flags - anchored to the host program at these shapes by
tests/test_decoder_shapes_host.py.  In one case per rate the decoder gates the post chain (gate = 1): the PCM is the oracle's chain
over the frames the model's drop flags keep, and zeros in the others.  The table's conditions are evaluated on the model's records.
Where a decision's window holds the carrier alone - no flagged frame, nothing behind the carrier's end - the tone named is the tone
sent, and from the second such decision in a row the gate is open.  The case with the shortest ring has a twin without the decoder in a second context: its rows are the same bits."""
import functools

import numpy as np
import pytest

import decoder_shapes as S
import tone_model as M
from helpers import assert_same_bits, read_client, row_names
from test_gpu_tone_decoder import rec_of

pytestmark = pytest.mark.gpu


def cfg_of(case):
    return dict(S.TONE_CFG, gate=1 if case in S.TONE_GATED else 0)


@functools.lru_cache(maxsize=None)
def run(rate, n, whole):
    nf = S.tone_timing(rate, n)[0]
    batches = (nf,) if whole else S.split_of(nf, n // 2)
    gated = (rate, n) in S.TONE_GATED
    twin = (rate, n) == S.TWIN and not whole
    raw = S.tone_raw(rate, n)
    A = S.open_ctx(rate, n, max(batches), raw, post=gated)
    B = S.open_ctx(rate, n, max(batches), raw, post=gated) if twin else None
    try:
        A.add("AM")
        g = A.add("USB", tone=cfg_of((rate, n)))
        if B:
            B.add("AM")
            gb = B.add("USB")
        A.ctx.set_profiling(1)
        a, t, b = [], [], []
        for F in batches:
            A.batch(F)
            a.append(read_client(g, "USB", F, pcm=gated)), t.append(g.read_tone(F))
            if B:
                B.batch(F)
                b.append(read_client(gb, "USB", F))
        return S.cat(a), S.cat(t), A.ctx.kernel_stats(), batches, (S.cat(b) if B else None)
    finally:
        A.close()
        if B:
            B.close()


def oracle_pcm(audio, keep, h, rate):
    """tests/test_gpu_squelch.py's oracle_pcm at the case's rate"""
    from oracle import oracle as O
    ch = O.PostChain(rate)
    want = np.zeros((len(audio), h), np.int32)
    for f in range(len(audio)):
        if keep[f]:
            want[f] = ch.process(audio[f])
    return want


def carrier_alone(rate, h, nf, off, nan):
    """(the frames whose last decision's window holds the carrier and no flagged frame, those of them whose decision before is such a
    one too: the second hit in a row, which attack_blocks = 2 opens the gate on)"""
    nb = M.nb_of(rate)
    bad = np.repeat(np.asarray(nan) != 0, h)
    bad[off * h:] = True
    done = ((np.arange(nf) + 1) * h) // M.B

    def clean(d):
        return d >= nb and not bad[(d - nb) * M.B:d * M.B].any()

    return np.array([clean(d) for d in done]), np.array([clean(d) and clean(d - 1) for d in done])


@pytest.mark.parametrize("rate,n", S.TONE_CASES)
def test_records_are_the_models_at_every_window_and_frame_length(rate, n):
    h = n // 2
    nf, off, _ = S.tone_timing(rate, n)
    gated = (rate, n) in S.TONE_GATED
    rows, _, nan = run(rate, n, True)[0][:3]
    assert rows.shape == (nf, h) and nan.any()
    want, wdrop = M.records(rows, nan, h, rate, gate=int(gated), hang=S.TONE_CFG["hang_blocks"], prev_drop=nan)
    figures = {}
    for whole in (True, False):
        a, t, stats, batches, twin = run(rate, n, whole)
        assert_same_bits((a[0], a[2]), (rows, nan), "the rows of the two runs", ("audio", "nan"))
        got = rec_of(t)
        ms, cnt = stats["audio_tone"]
        print(f"rate {rate} n {n} batches {batches}: open {int(got['open'].sum())} of {nf} frames, level {got['level'].max():.4g}; {cnt} launches, "
              f"{1e3 * ms / max(cnt, 1):.1f} us each")
        figures.update({("whole" if whole else "split") + "_launches": int(cnt), ("whole" if whole else "split") + "_us_per_launch": 1e3 * ms / max(cnt, 1)})
        bad = [k for k in range(nf) if got[k].tobytes() != want[k].tobytes()]
        assert not bad, (batches, bad[:8], got[bad[:4]], want[bad[:4]])
        assert cnt == len(batches)
        if gated:  # the drop flags, as the chain took them
            keep = wdrop == 0
            pcm = a[3]
            wpcm = oracle_pcm(rows, keep, h, rate)
            assert keep.any() and (~keep & (nan == 0)).any() and not pcm[~keep].any()
            assert [k for k in range(nf) if not np.array_equal(pcm[k], wpcm[k])] == [] and np.count_nonzero(wpcm) > 1000
        if twin is not None:
            assert_same_bits(a[:3], twin, "the twin without the decoder", row_names("USB"))
    assert ((rate, n) != S.TWIN) or twin is not None
    S.record("tone", rate=rate, n=n, frames=nf, **figures)
    broken = S.tone_rules(rate, h, batches, want, nan)
    assert not broken, broken
    alone, second = carrier_alone(rate, h, nf, off, nan)
    assert alone.sum() >= 3 and (want["tone"][alone] == S.TONE).all() and second.any() and (want["open"][second] == 1).all()

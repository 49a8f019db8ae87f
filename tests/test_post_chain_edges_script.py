"""The scripted signal of tests/test_gpu_post_chain_edges.py reaches every regime it is meant to - checked here without a GPU,
the oracle's demodulator in the GPU's place, at every (rate, n) of the GPU module's matrix.  The GPU test asserts the same
figures on the GPU's own audio; this one says, on any machine, whether an amplitude of the script needs another decade."""
import numpy as np
import pytest

import post_chain_edges as E
from oracle import oracle as O


@pytest.mark.parametrize("rate,n", [(12000, 360), (12000, 252), (44100, 248), (48000, 248), (192000, 248)])
def test_the_script_reaches_every_regime(rate, n):
    s = E.Script(rate, n)
    tw = E.Twins(s)
    cl = []
    for mode in ("USB", "AM", "FM"):
        o = O.AudioClient(False, n, rate, E.N)
        o.set_audio_demodulation(mode)
        o.set_audio_range(*s.windows[mode])
        cl.append(o)
    spec = np.zeros(E.N + n + 8, np.complex64)
    for f in range(s.nframes):
        spec[:E.N] = np.roll(s.rows(f, 1)[0], E.N // 2 + 1)  # the reference's bin order; the rows are in a client's own
        spec[E.N:] = spec[:n + 8]
        if f == s.reset_at:
            cl[0].set_audio_demodulation("LSB")
            cl[0].set_audio_range(*s.windows["LSB"])
        audio = []
        for ci, o in enumerate(cl):
            if ci == 1 and s.paused(f):
                audio.append(None)
                continue
            a, _, _, dropped = o.send_audio(spec, f, stats=False)
            assert not dropped
            audio.append(a)
        tw.feed(f, audio)
    for what, (value, least) in tw.regimes().items():
        print(f"{rate} Hz n {n}: {what}: {value} (at least {least})")
        assert value >= least, f"{rate} Hz n {n}: {what}: {value}, needs {least}"


def test_the_batch_plans_cut_where_the_events_are():
    for rate, n, F in [(12000, 360, 7), (12000, 360, 33), (12000, 252, 7), (44100, 248, 33), (48000, 248, 33), (192000, 248, 128)]:
        s = E.Script(rate, n)
        single = range(s.start["e"] - 3, s.start["e"] + 4) if F == 33 and rate == 12000 else ()
        plan = s.batches(F, single)
        starts = [a for a, _ in plan]
        assert sum(k for _, k in plan) == s.nframes and all(0 < k <= F for _, k in plan)
        assert {s.reset_at, s.pause_from, s.pause_to} <= set(starts)
        assert sum(1 for a, _ in plan if s.paused(a)) >= 2, "the pause is not a run of batches"
        assert s.start["d"] < s.reset_at < s.pause_from and s.pause_to <= s.start["e"]
        assert all(k == 1 for a, k in plan if a in single[:-1]) and (not single or plan != s.batches(7))

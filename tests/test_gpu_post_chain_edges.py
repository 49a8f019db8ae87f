"""The post chain at the signal edges: digital silence, bursts behind silence, int16 saturation with the conversion's argument
inside and far outside int32, denormal audio, a DC step, an AGC reset and a paused client in mid-silence.  Every other post
chain test feeds the chain stationary noise, under which the AGC sits at its target and the PCM stays within +-3300 counts.

Mechanism: test_gpu_state_freeze.py's / test_gpu_nonfinite_modes.py's.  A caller-owned linear spectrum (2^14-point IQ context)
goes through psdr_demod_batch_from, so the audio is fully scripted (post_chain_edges.py: a unit pattern times a per-frame
amplitude, three clients - USB tone, AM carrier, FM on the same carrier); the GPU's own float audio rows go through the
oracle's chain, and the PCM is compared bit for bit.  No tolerance anywhere.  What keeps a case from passing without having
tested anything is computed from the reference chain alone (Twins.regimes): counts of samples at either rail, of AGC outputs
beyond +-2^31 / 16384, a denormal frame, the zeros behind the reset, the pause that mattered.

Beyond int32 the reference's conversion is undefined (its x86 build gives +32767 for both signs); the library and the oracle
saturate by sign (include/psdr.h, psdr_set_post_chain) - the one definition, pc_to_int16, that every output kernel uses."""
import ctypes as C
import functools

import numpy as np
import pytest

import post_chain_edges as E
from test_gpu_parity import levels_for

pytestmark = pytest.mark.gpu

BATCH = {12000: 7, 44100: 33, 48000: 33, 192000: 128}
# (rate, n, AGC form, PCM16).  form 1: k_pc_agc where the rate and n allow it (n = 252: frames that are not whole row groups -
# the scalar gather and k_pc_out; 44100: a look-ahead that is not whole chunks, the generic division path, k_pc_out4), 0: the
# five-kernel form (k_pc_out4), 2: the form flips with every batch; 192000: look-ahead 38400, the chunked scan
CASES = [(12000, 360, 1, False), (12000, 360, 1, True), (12000, 360, 0, False), (12000, 360, 2, False), (12000, 252, 1, False),
         (12000, 252, 1, True), (44100, 248, 1, False), (48000, 248, 1, False), (48000, 248, 0, False), (192000, 248, 1, False)]


@functools.lru_cache(maxsize=2)
def play(rate, n, form, pcm16, F, single=()):
    """the script in batches of at most F frames -> (per client {frame: PCM row}, differing samples [(client, frame, index,
    want, got)], how many samples were compared, the Twins)"""
    from phantomsdr_amd import AudioClient, Context
    s = E.Script(rate, n)
    tw = E.Twins(s)
    ctx = Context(E.N, False, levels_for(E.N), additional_size=n, audio_fft_size=n, audio_rate=rate, input_format="s16", max_batch=F,
                  max_clients=3)
    try:
        ctx.set_option(ctx.OPT_POST_CHAIN_AGC, form & 1)
        if pcm16:
            ctx.set_option(ctx.OPT_POST_CHAIN_PCM16, 1)
        ctx.set_post_chain(True)
        d = ctx.dev_alloc(F * E.N * 8)
        cl = []
        for mode in ("USB", "AM", "FM"):
            g = AudioClient(ctx)
            g.set_audio_demodulation(mode)
            g.set_audio_range(*s.windows[mode])
            cl.append(g)
        got = [{} for _ in cl]
        bad, compared = [], 0
        for b, (f0, nb) in enumerate(s.batches(F, single)):
            if form == 2:
                ctx.set_option(ctx.OPT_POST_CHAIN_AGC, b & 1)
            if f0 == s.reset_at:
                cl[0].set_audio_demodulation("LSB")
                cl[0].set_audio_range(*s.windows["LSB"])
            cl[1].set_paused(s.paused(f0))
            ctx.h2d(d, s.rows(f0, nb))
            rc = ctx.lib.psdr_demod_batch_from(ctx.h, C.c_void_p(d.value), E.N, nb, f0)
            assert rc == 0, ctx.lib.psdr_last_error()
            if pcm16:
                ctx.fetch_begin(ctx.FETCH_PCM)
                ctx.fetch_end()
            audio, pcm = [], []
            for ci, g in enumerate(cl):
                if ci == 1 and s.paused(f0):
                    audio.append(None), pcm.append(None)
                    continue
                a, _, nan = g.read_audio(F)
                assert not nan[:nb].any(), f"client {ci} batch at frame {f0}: a frame was flagged"
                audio.append(a), pcm.append(g.read_pcm(F))
                if pcm16:  # exact: every value is clamped
                    for f in range(nb):
                        row = ctx.fetched_pcm16(g.id, f)
                        assert row.dtype == np.int16 and np.array_equal(row.astype(np.int32), pcm[ci][f]), \
                            f"client {ci} frame {f0 + f}: the int16 row is not the int32 row of psdr_read_pcm narrowed"
            for f in range(nb):
                want = tw.feed(f0 + f, [None if a is None else a[f] for a in audio])
                for ci, w in enumerate(want):
                    if w is None:
                        continue
                    g_row = pcm[ci][f]
                    got[ci][f0 + f] = g_row.copy()
                    compared += w.size
                    for i in np.nonzero(g_row != w)[0]:
                        bad.append((ci, f0 + f, int(i), int(w[i]), int(g_row[i])))
        ctx.dev_free(d)
        return got, bad, compared, tw
    finally:
        ctx.close()


def report(bad, compared, s):
    """the first differing sample by where it is - its position against chunk, block and batch boundaries names the kernel -
    and which values went wrong into which"""
    ci, f, i, w, g = bad[0]
    seg = [name for name, _, _ in E.SEGMENTS if f in s.segment(name)][0]
    pairs = {}
    for _, _, _, w_, g_ in bad:
        pairs[(w_, g_)] = pairs.get((w_, g_), 0) + 1
    top = sorted(pairs.items(), key=lambda kv: -kv[1])[:6]
    return (f"{len(bad)} of {compared} PCM samples differ; the first: client {ci} frame {f} (segment {seg}) sample {i}, "
            f"want {w}, got {g}; (want, got): count {top}")


@pytest.mark.parametrize("rate,n,form,pcm16", CASES, ids=[f"{r}-n{n}-agc{a}{'-pcm16' if p else ''}" for r, n, a, p in CASES])
def test_post_chain_through_silence_bursts_and_saturation(rate, n, form, pcm16):
    got, bad, compared, tw = play(rate, n, form, pcm16, BATCH[rate])
    regimes = tw.regimes()
    for what, (value, least) in regimes.items():
        print(f"{rate} Hz n {n} form {form}: {what}: {value} (at least {least})")
    print(f"{rate} Hz n {n} form {form}: {len(bad)} of {compared} samples differ" + (": " + report(bad, compared, tw.s) if bad else ""))
    for what, (value, least) in regimes.items():
        assert value >= least, f"the case did not reach its regime: {what}: {value}, needs {least}"
    assert not bad, report(bad, compared, tw.s)
    s = tw.s
    assert all(f not in got[1] for f in range(s.pause_from, s.pause_to)) and s.pause_to in got[1]


def test_another_batch_split_gives_the_same_pcm():
    """Batches of 33 frames instead of 7, and one-frame batches across the end of the long silence and the burst: the chain's
    carried gain and histories do not care where a batch ends"""
    rate, n = 12000, 360
    s = E.Script(rate, n)
    a, bad_a, _, _ = play(rate, n, 1, False, BATCH[rate])
    b, bad_b, compared, tw = play(rate, n, 1, False, 33, tuple(range(s.start["e"] - 3, s.start["e"] + 4)))
    assert not bad_b, report(bad_b, compared, tw.s)
    for ci in range(3):
        assert sorted(a[ci]) == sorted(b[ci])
        differ = [f for f in a[ci] if a[ci][f].tobytes() != b[ci][f].tobytes()]
        assert not differ, f"client {ci}: frames {differ[:10]} differ between the two splits"
    assert not bad_a

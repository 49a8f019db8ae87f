"""The post chain (DC blocker, AGC, int16) on every form its plan can take without a tuning knob: the five moving-average
kernels, both AGC pipelines, the lane = slot and the scalar gather / output, 32 and 64 slots per recurrence work-group, waves
that own a SIMD and waves that do not - and clients in the high slots of 600, 1600 and 2000, with holes between them.

Mechanism: test_gpu_parity.py::test_post_chain_bit_exact's.  The GPU's own float audio rows go through the oracle's chain
(oracle.PostChain) and psdr_read_pcm is compared bit for bit; there is no tolerance anywhere.  The cases, the plan each must
resolve to and the rules their streams follow are tests/post_chain_forms.py's; tests/test_post_chain_forms_cover.py checks on
the host that they cover every form a sweep of rates, frame sizes and slot counts resolves to, and that each case's input
drives the chain far enough.  The same counts are asserted here on the expected rows, so a case cannot pass on zeros.

Not covered: rates of 384 kHz and up with more than 512 slots (D >= 1024, 64 lanes: the fall-back to MA_POW2) - see
post_chain_forms.py."""
import numpy as np
import pytest

import post_chain_forms as PF
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def configure(g, case, k, slot):
    assert g.id == slot, f"client {k} sits in slot {g.id}, not {slot}"
    mode, l, m, r = PF.client_spec(case, k)
    g.set_audio_demodulation(mode)
    g.set_audio_range(l, m, r)
    return g


def add_client_at(ctx, case, k, slot):
    """a new client in `slot`: a new client takes the lowest free slot, so the holes below are filled for the moment"""
    from phantomsdr_amd import AudioClient
    fillers = []
    while True:
        g = AudioClient(ctx)
        if g.id == slot:
            break
        assert g.id < slot, f"slot {slot} is taken"
        fillers.append(g)
    for f in fillers:
        f.on_close()
    return configure(g, case, k, slot)


@pytest.mark.parametrize("name", list(PF.CASES))
def test_post_chain_form_is_bit_exact(name):
    from phantomsdr_amd import AudioClient, Context
    case = PF.CASES[name]
    n, h, F = case.n, case.n // 2, case.max_batch
    raw = PF.raw_stream(case)
    slots = PF.slots_of(case)
    ctx = Context(PF.N, False, PF.LEVELS, additional_size=n, audio_fft_size=n, audio_rate=case.rate, input_format="s16", max_batch=F,
                  max_clients=case.slots)
    try:
        ctx.set_option(ctx.OPT_POST_CHAIN_AGC, PF.agc_option(case, 0))
        if case.pcm16:
            ctx.set_option(ctx.OPT_POST_CHAIN_PCM16, 1)
        ctx.set_post_chain(True)
        d = ctx.dev_alloc(raw.nbytes)
        ctx.h2d(d, raw)
        clients = {}  # k -> (AudioClient, its chain)
        if case.slots > 64:
            # every slot taken, then all but the wanted ones removed: the survivors sit where they are meant to, between holes
            everyone = [AudioClient(ctx) for _ in range(case.slots)]
            assert [g.id for g in everyone] == list(range(case.slots))
            for g in everyone:
                if g.id not in case.occupied:
                    g.on_close()
            for k, slot in enumerate(slots):
                if slot != case.late:
                    clients[k] = (configure(everyone[slot], case, k, slot), O.PostChain(case.rate))
        else:
            for k, slot in enumerate(slots):
                clients[k] = (configure(AudioClient(ctx), case, k, slot), O.PostChain(case.rate))
        hb = ctx.half_frame_bytes()
        nonzero, in_last, pos = {k: 0 for k in range(len(slots))}, {k: 0 for k in range(len(slots))}, {k: 0 for k in range(len(slots))}
        f0 = 0
        for b, nb in enumerate(case.batches):
            if case.agc == 2:
                ctx.set_option(ctx.OPT_POST_CHAIN_AGC, PF.agc_option(case, b))
            if b == PF.LATE_BATCH and case.late is not None:
                k = slots.index(case.late)
                clients[k] = (add_client_at(ctx, case, k, case.late), O.PostChain(case.rate))
            ctx.process_batch(d, nb, offset_bytes=f0 * hb)
            ctx.demod_batch(f0)
            if case.pcm16:
                ctx.fetch_begin(ctx.FETCH_PCM)
                ctx.fetch_end()
            for k, (g, chain) in sorted(clients.items()):
                assert g.id == slots[k]
                audio, _, nan = g.read_audio(F)
                pcm = g.read_pcm(F)
                assert len(audio) == nb and len(pcm) == nb
                assert not nan[:nb].any(), f"client {k} slot {g.id} batch {b}: a frame was flagged"
                for f in range(nb):
                    want = chain.process(audio[f])
                    assert np.array_equal(pcm[f], want), PF.mismatch(case, k, g.id, b, f, pos[k], want, pcm[f])
                    if case.pcm16:  # exact: every value is clamped
                        row = ctx.fetched_pcm16(g.id, f)
                        assert row.dtype == np.int16 and np.array_equal(row.astype(np.int32), pcm[f]), \
                            f"client {k} slot {g.id} batch {b} frame {f}: the int16 row is not the int32 row of psdr_read_pcm narrowed"
                    c = int(np.count_nonzero(want))
                    nonzero[k] += c
                    in_last[k] += c if b == len(case.batches) - 1 else 0
                    pos[k] += h
            f0 += nb
        assert sorted(clients) == list(range(len(slots)))
        assert min(nonzero.values()) >= 1000 and min(in_last.values()) >= 1, \
            f"the AGC never opened for a client (non-zero expected samples {nonzero}, in the last batch {in_last}): the case did not exercise the chain"
        ctx.dev_free(d)
    finally:
        ctx.close()

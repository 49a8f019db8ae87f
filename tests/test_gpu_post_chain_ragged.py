"""The post chain's forms with ragged streams: frames flagged non-finite, frames a squelch closes and paused clients give the
lanes of one recurrence work-group streams of different lengths in the same batch - through every moving-average kernel, both
AGC pipelines with and without the AGC profile table, 32 and 64 lanes, waves that own their SIMD and waves that do not, the
scalar gather / output, batches of more than 64 frames (the later ballots of k_pc_index) and a launch of k_pc_ma2 with a DIRECT
work-group beside a gathered one.  The audio filter sits in front of the chain on one client, AGC profiles (one the oracle can
express, one capped, one manual) on about a third of them, in the high slots too.

Cases, drop script, features and the rules they follow: tests/post_chain_ragged.py; tests/test_post_chain_ragged_cover.py checks
them on the host.  Mechanism: test_gpu_post_chain_forms.py's with test_gpu_post_chain_edges.py's input - a caller-owned spectrum
per frame through psdr_demod_batch_from, a NaN in one bin of a client's window per dropped (client, frame).  The kept rows (alive
& open & not paused) of the GPU's own float audio go, in stream order, through the oracle's chain - clients with a profile:
the oracle's DC blocker, the host program over agcplan.h that test_agc_profile_host.py and the cover test pin to the oracle's AGC
(the oracle's own AGC where it can express the profile), the oracle's int16 conversion - and psdr_read_pcm is compared bit for
bit.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import agc_profile_model as M
import post_chain_forms as PF
import post_chain_ragged as R
from conftest import ROOT
from oracle import oracle as O

pytestmark = pytest.mark.gpu
NO_DATA = -7   # PSDR_ERR_NO_DATA


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_post_chain_ragged")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


def configure(g, case, k, slot):
    """window, mode and features of the case's k-th client, in front of its first batch"""
    from phantomsdr_amd import design_audio_filter as d
    assert g.id == slot, f"client {k} sits in slot {g.id}, not {slot}"
    ft = R.features(case)
    mode, l, m, r = R.client_spec(case, k)
    g.set_audio_demodulation(mode)
    g.set_audio_range(l, m, r)
    if k in ft.profiles:
        g.set_agc_profile(ft.profiles[k])
    if k == ft.squelch:
        g.set_squelch(True, *R.squelch_params(case))
    if k == ft.filter:
        g.set_audio_filter([d("highpass", case.rate, 300.0), d("deemphasis", case.rate, 212.0)])   # test_gpu_audio_filter.py's "two"
    return g


def add_client_at(ctx, slot):
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
    return g


@pytest.mark.parametrize("name", list(R.CASES))
def test_ragged_streams_are_bit_exact(name, exe, tmp):
    from phantomsdr_amd import AudioClient, Context, PsdrError
    case = R.CASES[name]
    n, h, F = case.n, case.n // 2, case.max_batch
    slots, st, ft = PF.slots_of(case), R.starts(case), R.features(case)
    nc, nb_all = len(slots), len(case.batches)
    spec, alive, present = R.spectra(name), R.alive(name), R.present(name)
    ctx = Context(R.N, False, R.LEVELS, additional_size=n, audio_fft_size=n, audio_rate=case.rate, input_format="s16", max_batch=F,
                  max_clients=case.slots)
    try:
        ctx.set_option(ctx.OPT_POST_CHAIN_AGC, PF.agc_option(case, 0))
        if case.pcm16:
            ctx.set_option(ctx.OPT_POST_CHAIN_PCM16, 1)
        ctx.set_post_chain(True)
        d = ctx.dev_alloc(F * R.N * 8)
        clients = {}
        if case.slots > 64:
            # every slot taken, then all but the wanted ones removed: the survivors sit where they are meant to, between holes
            everyone = [AudioClient(ctx) for _ in range(case.slots)]
            assert [g.id for g in everyone] == list(range(case.slots))
            for g in everyone:
                if g.id not in case.occupied:
                    g.on_close()
            for k, slot in enumerate(slots):
                if slot != case.late:
                    clients[k] = configure(everyone[slot], case, k, slot)
        else:
            for k, slot in enumerate(slots):
                clients[k] = configure(AudioClient(ctx), case, k, slot)
        gate, opened = (0, 0), np.ones(st[-1], bool)
        audio = [np.zeros((st[-1], h), np.float32) for _ in range(nc)]
        pcm = [np.zeros((st[-1], h), np.int32) for _ in range(nc)]
        for b, nb in enumerate(case.batches):
            f0 = st[b]
            if b == R.LATE_BATCH and case.late is not None:
                k = slots.index(case.late)
                clients[k] = configure(add_client_at(ctx, case.late), case, k, case.late)
            for k, g in clients.items():   # the pause lands at its batch boundary
                if R.paused(case, k, b) or (b and R.paused(case, k, b - 1)):
                    g.set_paused(R.paused(case, k, b))
            ctx.h2d(d, np.ascontiguousarray(spec[f0:f0 + nb]))
            rc = ctx.lib.psdr_demod_batch_from(ctx.h, C.c_void_p(d.value), R.N, nb, f0)
            assert rc == 0, ctx.lib.psdr_last_error()
            ctx.last_demod_frames = nb
            if case.pcm16:
                ctx.fetch_begin(ctx.FETCH_PCM)
                ctx.fetch_end()
            for k, g in sorted(clients.items()):
                tag = f"{name} client {k} slot {g.id} batch {b}"
                if R.paused(case, k, b):   # (include/psdr.h, psdr_client_set_paused: its results read as PSDR_ERR_NO_DATA)
                    for read in (g.read_audio, g.read_pcm, g.read_squelch):
                        with pytest.raises(PsdrError) as e:
                            read(F)
                        assert e.value.code == NO_DATA, tag
                    continue
                a, pwr, nan = g.read_audio(F)
                p = g.read_pcm(F)
                assert len(a) == nb and len(p) == nb, tag
                want = ~alive[k, f0:f0 + nb]
                assert np.array_equal(nan != 0, want), f"{tag}: the NaN flags are not the script's, frames {np.nonzero((nan != 0) != want)[0].tolist()}"
                flags = g.read_squelch(F)
                if k == ft.squelch:   # the model fed the GPU's own pwr bits
                    model, gate = R.squelch_flags(case, pwr, gate)
                    assert np.array_equal(flags, model), f"{tag}: squelch flags {flags.tolist()}, the model's {model.tolist()}"
                    opened[f0:f0 + nb] = flags == 1
                else:
                    assert flags.all(), tag
                audio[k][f0:f0 + nb], pcm[k][f0:f0 + nb] = a, p
                if case.pcm16:   # exact: every value is clamped
                    for f in range(nb):
                        row = ctx.fetched_pcm16(g.id, f)
                        assert row.dtype == np.int16 and np.array_equal(row.astype(np.int32), p[f]), f"{tag} frame {f}: the int16 row is not the int32 row narrowed"
        assert sorted(clients) == list(range(nc))
        gains = {k: clients[k].read_agc_gain() for k in ft.profiles}
        ctx.dev_free(d)
    finally:
        ctx.close()

    keep = R.keep_mask(name, opened)
    assert np.array_equal(keep[ft.squelch], alive[ft.squelch] & opened & present[ft.squelch])
    d_open = np.diff(opened[present[ft.squelch]].astype(int))
    assert (d_open > 0).any() and (d_open < 0).any(), "the squelch client never opened or never closed"
    e = R.expected_pcm(name, audio, keep, exe, tmp, "gpu" + name)
    want, model_gain = e.pcm, e.gain
    assert e.uncapped and not R.cap_binds(e), f"{name}: the cap does not act for clients {R.cap_binds(e)} (largest gains {e.peak_gain})"
    nonzero, in_last, bad = [], [], []   # bad: the first differing batch of every client that differs
    for k in range(nc):
        assert not pcm[k][~keep[k]].any(), f"{name} client {k}: PCM in a frame that is dropped, closed or paused: frames {np.nonzero(pcm[k][~keep[k]].any(axis=1))[0].tolist()}"
        for b in range(nb_all):
            rows = slice(int(keep[k][:st[b]].sum()), int(keep[k][:st[b + 1]].sum()))
            w, got = want[k][rows].reshape(-1), pcm[k][st[b]:st[b + 1]][keep[k][st[b]:st[b + 1]]].reshape(-1)
            if not np.array_equal(w, got):
                bad.append(R.mismatch(name, k, b, w, got) + (f" [profile: {R.profile_kind(case, k)}]" if k in ft.profiles else ""))
                break
        nonzero.append(int(np.count_nonzero(want[k])))
        in_last.append(int(np.count_nonzero(want[k][int(keep[k][:st[-2]].sum()):])))
    assert not bad, f"{len(bad)} of {nc} clients differ:\n" + "\n".join(bad)
    print(f"{name}: non-zero expected PCM samples per client {nonzero}, in the last batch {in_last}")
    assert min(nonzero) >= 1000 and min(in_last) >= 1, (nonzero, in_last)
    # the filter acted in front of the chain: other rows than the twin's wherever both have one, and (above) the chain over them
    both = keep[ft.filter] & keep[ft.twin]
    assert both.sum() > 4 and all(audio[ft.filter][f].tobytes() != audio[ft.twin][f].tobytes() for f in np.nonzero(both)[0]), "the filter client's rows are the twin's"
    # the profiles acted, and the gain each left behind is the model's
    for k in ft.profiles:
        rows = np.ascontiguousarray(audio[k][keep[k]])
        plain = O.PostChain(case.rate).process(rows.reshape(-1)).reshape(rows.shape)
        assert not np.array_equal(want[k], plain), f"{name} client {k}: the profile gives the context's PCM"
        assert gains[k].view(np.uint32) == model_gain[k].view(np.uint32), f"{name} client {k} slot {slots[k]}: psdr_read_agc_gain {gains[k]!r} is not the model's carried gain {model_gain[k]!r}"

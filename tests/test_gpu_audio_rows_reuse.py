"""A slot that psdr_client_remove frees and psdr_client_add hands out again: the new occupant inherits nothing.

The first occupant of slot 1 is a SAM client that carries per-slot state of every kind - audio blanker and noise reduction on
"strong", two audio filter sections, an open squelch, the noise floor, auto-notch with automatic entries, a manual-gain AGC
profile under the post chain - and runs four batches of 6 frames at n = 360, past every delay (audio_rate = 8 x audio_fft_size:
the auto-notch and the noise floor evaluate every 8 frames).  Then it is removed, and psdr_client_add returns its id to a new
client; a twin is added at the same moment into slot 2, which was never used.  Three new occupants - (a) sets nothing, (b) sets
blanker, noise reduction, filter and squelch by explicit calls, (c) gets blanker and noise reduction from PSDR_OPT_AUDIO_BLANKER /
PSDR_OPT_NOISE_REDUCTION - each with no batch between remove and add and with the slot empty for one batch.

Expected, without a tolerance: (a) equals the twin in every word, PCM included; (b) and (c) equal the host table programs
started from zero on the twin's rows from the add on, the blanker's totals theirs; before the new occupant's first batch every
read call of a feature answers PSDR_ERR_NO_DATA or the fresh value; a fetch begun for the first occupant does not answer for the
second (AudioSlot::born).  The first occupant's squelch is open: in (a) and (c) the new occupant has none and reads open too, so
an inherited gate shows in (b) alone, whose gate must start from closed."""
import functools

import numpy as np
import pytest

import anb_model as ANB
import audio_filter_model as AF
import audio_rows_shapes as S
import nr_model as NR
from conftest import ROOT
from helpers import assert_same_bits, read_client, row_names, set_client_kind
from test_gpu_audio_blanker import cat, expect, same_words
from test_gpu_audio_rows_long import sections
from test_gpu_squelch import STD, Gate, stream

pytestmark = pytest.mark.gpu

N_AUDIO, F, PERIOD = 360, 6, 8
RATE = PERIOD * N_AUDIO
FIRST, SECOND = 4, 3                      # batches of the first occupant, of the second
ALWAYS = (-300.0, -300.0, 1, 0)
STRONG_NB, STRONG_NR = (3.5, 11), (22.0, 2.0)
NO_DATA = -7
KIND = "SAM"
SPIKES = ((3, 100), (4, 777), (5, 1500))   # (half-frame, sample): about 100 times the audio's rms, in frames 2 .. 5


def no_data_or(fn, fresh):
    """a read call in front of the client's first batch: PSDR_ERR_NO_DATA, or the value a fresh client has"""
    from phantomsdr_amd import PsdrError
    try:
        v = fn()
    except PsdrError as e:
        assert e.code == NO_DATA, (fn, e.code)
        return
    assert fresh(v), (fn, v)


@functools.lru_cache(maxsize=None)
def run(variant, gap):
    from phantomsdr_amd import AudioClient, Context, PsdrError
    nf = (FIRST + gap + SECOND) * F
    raw = stream(S.SHAPE, key=(1,) * (nf + 1), nan_half=(FIRST + gap + 1) * F + 2, seed=11).copy()
    for half, at in SPIKES:   # wideband clicks inside the first occupant's first 8 frames: its blanker finds them at any threshold
        raw[2 * (half * (S.N // 2) + at)] += 1000.0
    ctx = Context(S.N, False, S.LEVELS, additional_size=N_AUDIO, audio_fft_size=N_AUDIO, audio_rate=RATE, input_format="f32", max_batch=F, max_clients=3)
    d = ctx.dev_alloc(raw.nbytes)
    try:
        ctx.h2d(d, raw)
        ctx.set_post_chain(True)
        frame = 0

        def batch():
            nonlocal frame
            ctx.process_batch(d, F, offset_bytes=frame * ctx.half_frame_bytes())
            ctx.demod_batch(frame)
            frame += F

        def client():
            g = AudioClient(ctx)
            set_client_kind(g, KIND)
            g.set_audio_range(S.L0, S.L0 + 50.3, S.L0 + 100)
            return g

        by = client()   # a bystander in slot 0: the context is never without a client
        first = client()
        assert (by.id, first.id) == (0, 1)
        first.set_audio_blanker("strong"), first.set_noise_reduction("strong"), first.set_audio_filter(sections())
        first.set_squelch(True, *ALWAYS), first.set_noise_floor(True), first.set_auto_notch(True)
        first.set_agc_profile("reference", manual=True, manual_gain=3.0)
        for _ in range(FIRST):
            batch()
        # the state the new occupant must not inherit is there
        before = dict(notches=first.notches(), noise=first.read_noise(F).copy(), counts=first.audio_blanker_counts(), gain=float(first.read_agc_gain()),
                      squelch=first.read_squelch(F).copy(), rows=first.read_audio(F)[0].copy(), by=by.read_audio(F)[0].copy())
        ctx.fetch_begin(ctx.FETCH_AUDIO | ctx.FETCH_PCM)   # ... of the first occupant's last batch; ended behind the add
        first.on_close()
        for _ in range(gap):
            batch()
        if variant == "c":
            ctx.set_option(ctx.OPT_AUDIO_BLANKER, 3), ctx.set_option(ctx.OPT_NOISE_REDUCTION, 3)
        new = client()
        if variant == "c":
            ctx.set_option(ctx.OPT_AUDIO_BLANKER, 0), ctx.set_option(ctx.OPT_NOISE_REDUCTION, 0)
        twin = client()
        assert (new.id, twin.id) == (1, 2)
        if variant == "b":
            new.set_audio_blanker("normal", *S.PARITY), new.set_noise_reduction("normal", *S.NRP), new.set_audio_filter(sections())
            new.set_squelch(True, *STD)
        ctx.fetch_end()
        fetched_by = ctx.fetched_audio(by.id, 0)[0] if gap == 0 else None
        with pytest.raises(PsdrError) as e:
            ctx.fetched_audio(new.id, 0)
        assert e.value.code == NO_DATA, "the first occupant's fetched rows answer for the second"
        with pytest.raises(PsdrError) as e:
            ctx.fetched_squelch(new.id, 0)
        assert e.value.code == NO_DATA
        # in front of its first batch: nothing of the predecessor's
        no_data_or(lambda: new.read_audio(F), lambda v: False)
        no_data_or(lambda: new.read_pcm(F), lambda v: False)
        no_data_or(lambda: new.read_squelch(F), lambda v: False)
        no_data_or(lambda: new.read_noise(F), lambda v: False)
        no_data_or(new.audio_blanker_counts, lambda v: v == (0, 0))
        no_data_or(new.notches, lambda v: v == [(0, 0)] * 4)
        no_data_or(new.read_agc_gain, lambda v: float(v) != before["gain"])
        parts = ([], [])
        extra = dict(squelch=[], noise=[], notches=[], counts=[])
        for _ in range(SECOND):
            batch()
            parts[0].append(read_client(new, KIND, F, pcm=True)), parts[1].append(read_client(twin, KIND, F, pcm=True))
            extra["squelch"].append(new.read_squelch(F).copy()), extra["noise"].append(new.read_noise(F).copy()), extra["notches"].append(new.notches())
            if variant != "a":
                extra["counts"].append(new.audio_blanker_counts())
        if variant == "a":
            with pytest.raises(PsdrError) as e:
                new.audio_blanker_counts()
            assert e.value.code == NO_DATA
        return dict(new=cat(parts[0]), twin=cat(parts[1]), before=before, fetched_by=fetched_by, **extra)
    finally:
        ctx.dev_free(d)
        ctx.close()


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_audio_rows_reuse")


@pytest.fixture(scope="module")
def progs(tmp):
    return ANB.build_table(tmp, ROOT), NR.build_table(tmp, ROOT), AF.build_table(tmp, ROOT)


def check_first_occupant(r):
    b = r["before"]
    assert any(e != (0, 0) for e in b["notches"][2:]), ("no automatic entry", b["notches"])
    assert b["noise"].all() and b["squelch"].all() and b["counts"][0] > 0 and b["counts"][1] > 0 and b["gain"] > 0
    assert not np.array_equal(b["rows"], b["by"]), "the first occupant's features changed nothing"
    if r["fetched_by"] is not None:
        assert r["fetched_by"].tobytes() == b["by"][0].tobytes(), "the fetch is the first occupant's batch"


@pytest.mark.parametrize("gap", (0, 1))
def test_a_new_occupant_that_sets_nothing_is_its_twin(gap):
    r = run("a", gap)
    check_first_occupant(r)
    assert_same_bits(r["new"], r["twin"], f"gap {gap}", row_names(KIND, pcm=True))
    assert r["twin"][-1].any() and (r["twin"][2] != 0).any() and not (r["twin"][2] != 0).all()
    assert all(s.all() for s in r["squelch"]) and not any(w.any() for w in r["noise"]) and all(nt == [(0, 0)] * 4 for nt in r["notches"])


@pytest.mark.parametrize("gap", (0, 1))
@pytest.mark.parametrize("variant", ("b", "c"))
def test_a_new_occupant_with_features_starts_them_from_zero(progs, tmp, variant, gap):
    anb, nr, af = progs
    r = run(variant, gap)
    check_first_occupant(r)
    new, twin = r["new"], r["twin"]
    h, sizes = N_AUDIO // 2, [F] * SECOND
    nbp, nrp = (S.PARITY, S.NRP) if variant == "b" else (STRONG_NB, STRONG_NR)
    flagged = twin[2] != 0
    assert flagged.any() and not flagged.all()
    ((blanked, st, tr),) = expect(lambda jobs: ANB.run_streams(anb, tmp, jobs), [nbp + (twin[0], twin[2], sizes)])
    ((want, _, _),) = NR.run_streams(nr, tmp, [nrp + (blanked.reshape(-1), twin[2], h, sizes)], rate=RATE)
    if variant == "b":
        ((want, _),) = AF.run_blocked(af, tmp, [(sections(), want, twin[2], h, sizes)])
    T = h * sum(sizes)
    assert T >= ANB.D + 2 * ANB.B and T % ANB.B != 0
    S.record("gpu_reuse", n=N_AUDIO, h=h, variant=variant, gap=gap, batches=sizes, slots=3, centres=len(tr["centres"]), unusable_blocks=S.unusable_blocks(tr))
    same_words(new[0], want.reshape(twin[0].shape), (variant, gap, "the host programs from zero"))
    assert new[0][flagged].tobytes() == twin[0][flagged].tobytes()
    assert_same_bits(new[1:-1], twin[1:-1], f"{variant} gap {gap}: pwr, flags, carrier records", row_names(KIND)[1:])
    # the totals start from 0: after every batch they are the host program's, which started there
    total = (int(st["impulses"]), int(st["samples"]))
    assert r["counts"][-1] == total and total[0] == len(tr["centres"]), (r["counts"], total)
    assert r["counts"][0][0] <= r["counts"][1][0] <= r["counts"][2][0] and r["counts"][0][0] <= total[0]
    if variant == "b":
        assert len(tr["centres"]) >= 8
        gate, sq = Gate(STD), np.concatenate(r["squelch"])
        assert np.array_equal(sq, gate.batch(new[1])), "the gate started from closed"
        assert sq[0] == 0 and sq.any()
    else:
        assert all(s.all() for s in r["squelch"])
    assert not any(w.any() for w in r["noise"]) and all(nt == [(0, 0)] * 4 for nt in r["notches"])

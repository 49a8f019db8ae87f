"""The host table programs at frames longer than a block, without a GPU: tests/test_anb_host.py's, tests/test_nr_host.py's and
tests/test_audio_filter_host.py's split and float64-model tests at h = 256, 360, 518 and 1200, with their inputs, their models and
their bounds - nothing here has a tolerance of its own.  The three programs are what tests/test_gpu_audio_rows_*.py expect of the
GPU at these frame lengths, so they are anchored here first: every cut of a stream into batches of 1, 2, 3 and 4 frames gives the
unsplit bits (the blanker and the noise reduction; the audio filter's split tests hold each split to the float64 bound - a
batch boundary moves its 1024-sample blocks, and with them the rounding -, and so do these), and the independent float64 models
(tests/anb_model.py, tests/nr_model.py, tests/audio_filter_model.py) agree with them on streams that hold flagged frames.

At h = 1200 two flagged frames side by side zero 2400 samples: whole blocks of the blanker and of the noise reduction see nothing
but zeros.  include/psdr.h says what happens there - a block whose R[0] is not above 1e-20 has no detections; the gain is g_min
where Ps <= 0 and stays inside [g_min, 1] - and test_blocks_of_zeros_at_h_1200 holds both programs and the blanker's float64 model
to that.

test_the_case_table checks tests/audio_rows_shapes.py: every n has an accepted IDFT plan, and the GPU cases' streams - with the
CPU oracle's demodulator in the GPU's place - are long enough, hold a batch of one frame, flagged frames, unusable blocks, and at
least 8 centres with a gap across a block boundary and one across a batch boundary.  The figures go to
build/records/audio_rows_shapes.jsonl."""
import numpy as np
import pytest

import anb_model as ANB
import audio_filter_model as AF
import audio_rows_shapes as S
import create_plan_table
import nr_model as NR
from conftest import ROOT
from test_anb_host import MARGIN, NORMAL, coloured, spiked
from test_audio_filter_host import RATE, ok, rel_rms
from test_nr_host import noise

HS = tuple(n // 2 for n in S.LONG_N)
F = 2 * sum(S.BATCHES)                                    # frames of a host stream: twice the GPU case's
SPLITS = [(F,), S.BATCHES, (4, 2, 3, 1), (1,), (2,), (3,), (4,)]
BAD = (F // 2 - 1, F // 2)                                # two flagged frames side by side, in the middle


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("audio_rows_shapes")


@pytest.fixture(scope="module")
def anb(tmp):
    return ANB.build_table(tmp, ROOT)


@pytest.fixture(scope="module")
def nr(tmp):
    return NR.build_table(tmp, ROOT)


@pytest.fixture(scope="module")
def af(tmp):
    return AF.build_table(tmp, ROOT)


def flagged(x, h, bad=BAD):
    """x with the frames `bad` flagged: (rows - a NaN and NaN payloads in the flagged frames -, flags, the kept samples' mask,
    the stream as the kernels take it in: zeros there)"""
    x = np.array(x, np.float32)
    flags = np.zeros(len(x) // h, np.int32)
    flags[list(bad)] = 1
    for f in bad:
        x[f * h] = np.nan
        x[f * h + 1:(f + 1) * h].view(np.uint32)[:] = 0x7FC01234
    keep = np.repeat(flags, h) == 0
    return x, flags, keep, np.where(keep, x, np.float32(0))


def spikes_for(h):
    """centres at block edges, at frame edges and beside the flagged frames"""
    n = h * F
    c = {0, 255, 300, 511, 513, 769, 1000, 1004, h - 1, h, 3 * h - 2, BAD[0] * h - 3, (BAD[1] + 1) * h + 2, n - 700, n - 300}
    return sorted(v for v in c if 0 <= v < n)


# ---- every cut into batches of 1, 2, 3 and 4 frames gives the unsplit bits --------------------------------------------------------
@pytest.mark.parametrize("h", HS)
def test_blanker_any_split_gives_the_same_bits(anb, tmp, h):
    x, flags, keep, _ = flagged(spiked(h * F, spikes_for(h)), h)
    res = ANB.run_streams(anb, tmp, [(4.5, 7, x, flags, h, AF.batches_of(s, F)) for s in SPLITS], "split%d_" % h)
    rows0, st0, tr0 = res[0]
    assert len(tr0["order"]) == ANB.blocks_done(h * F) and int(st0[-1]["pos"]) == h * F and len(tr0["centres"]) >= 9
    assert rows0[~keep].tobytes() == x[~keep].tobytes(), "a flagged frame keeps its row"
    first = rows0[:ANB.D][keep[:ANB.D]]
    assert not first.view(np.uint32).any() and rows0[ANB.D:][keep[ANB.D:]].any()
    for s, (rows, st, tr) in zip(SPLITS[1:], res[1:]):
        assert rows.tobytes() == rows0.tobytes(), s
        assert tr["centres"].tobytes() == tr0["centres"].tobytes() and tr["m"].tobytes() == tr0["m"].tobytes() and tr["order"].tobytes() == tr0["order"].tobytes(), s
        assert (int(st[-1]["impulses"]), int(st[-1]["samples"])) == (int(st0[-1]["impulses"]), int(st0[-1]["samples"])) and int(st0[-1]["impulses"]) == len(tr0["centres"])
        assert st[-1]["hist"][int(st[-1]["cur"]) & 1].tobytes() == st0[-1]["hist"][int(st0[-1]["cur"]) & 1].tobytes(), s


@pytest.mark.parametrize("h", HS)
def test_noise_reduction_any_split_gives_the_same_bits(nr, tmp, h):
    x = (noise(h * F) + 4 * np.cos(2 * np.pi * 0.11 * np.arange(h * F))).astype(np.float32)
    x, flags, keep, _ = flagged(x, h)
    res = NR.run_streams(nr, tmp, [S.NRP + (x, flags, h, AF.batches_of(s, F)) for s in SPLITS], "split%d_" % h)
    rows0, st0, g0 = res[0]
    assert len(g0) == (h * F - NR.M) // NR.R + 1 and int(st0[-1]["pos"]) == h * F
    assert rows0[~keep].tobytes() == x[~keep].tobytes() and np.isfinite(rows0[keep]).all()
    for s, (rows, st, g) in zip(SPLITS[1:], res[1:]):
        assert rows.tobytes() == rows0.tobytes(), s
        assert g.tobytes() == g0.tobytes() and st[-1].tobytes() == st0[-1].tobytes(), s
    assert g0.min() >= 10 ** (-S.NRP[0] / 20) * (1 - 1e-7) and g0.max() <= 1.0 and g0.min() < 0.9


def sections(af):
    return [ok(af, AF.HIGHPASS, 300.0), ok(af, AF.DEEMPHASIS, 212.0)]


# ---- the float64 models -----------------------------------------------------------------------------------------------------------
# At the threshold's minimum about one sample in 2300 lies within MARGIN of the threshold, where f32 and float64 may decide
# differently - a property of the input.  So that input is short (the frames that hold 2304 samples, four at least, and one more:
# its middle frame is flagged) and its seed is the first from 7 on that keeps every sample 2e-3 away; the two inputs with spikes run
# all F frames, the two frames BAD flagged
NOISE_SEED = {256: 7, 360: 17, 518: 8, 1200: 46}


def noise_frames(h):
    return max(4, -(-2304 // h)) + 1


MODEL_INPUTS = {
    "spikes": lambda h: (spiked(h * F, spikes_for(h)), NORMAL, BAD),
    "noise at 2 sigma": lambda h: (coloured(h * noise_frames(h), NOISE_SEED[h]), S.PARITY, (noise_frames(h) // 2,)),
    "strong": lambda h: (spiked(h * F, spikes_for(h), 40.0, 11), (3.5, 11), BAD),
}


@pytest.mark.parametrize("h", HS)
def test_blanker_against_the_float64_model(anb, tmp, h):
    """tests/test_anb_host.py's test_the_float64_model_finds_the_same_centres_and_the_same_repairs with its bound of 2e-4 (derived
    there), on streams that hold flagged frames, cut into the GPU cases' batches"""
    worst = 0.0
    for name, make in MODEL_INPUTS.items():
        x0, par, bad = make(h)
        x, flags, keep, clean = flagged(x0, h, bad)
        assert flags.any() and not flags.all()
        (rows, st, tr), = ANB.run_streams(anb, tmp, [par + (x, flags, h, AF.batches_of(S.BATCHES, len(flags)))], "model")
        y, centres, ratio, orders = ANB.model(clean.astype(np.float64), *par)
        off = float(np.abs(ratio[ratio > 0] - 1).min())
        assert off >= MARGIN, (name, off)
        assert tr["centres"].tolist() == centres.tolist(), name
        assert tr["order"].tolist() == orders
        n = len(x)
        want = ANB.delayed(y, n)
        final = ANB.D + (ANB.blocks_done(n) - 1) * ANB.B - 8
        k = keep[:final]
        err = float(np.abs(rows[:final][k] - want[:final][k]).max())
        pl = (par[1] - 1) // 2
        gap = np.zeros(n, bool)
        for c in centres:
            gap[max(c - pl, 0):c + pl + 1] = True
        through = ~ANB.delayed(gap, n)[:final] & k
        assert rows[:final][through].tobytes() == ANB.delayed(clean, n)[:final][through].tobytes(), (name, "a sample outside every gap passes through")
        assert rows[~keep].tobytes() == x[~keep].tobytes()
        print(f"h {h} {name}: centres {len(centres)} unusable blocks {orders.count(-1)} nearest |m|/T to 1: {off:.2e}; repaired samples max abs diff {err:.3e}")
        S.record("anb_model", h=h, input=name, centres=len(centres), unusable_blocks=orders.count(-1), repaired_max_abs_diff=err, bound=2e-4)
        worst = max(worst, err)
        assert len(centres) >= 5
    assert worst <= 2e-4, worst


@pytest.mark.parametrize("h", HS)
def test_noise_reduction_against_the_float64_restatement(nr, tmp, h):
    """tests/test_nr_host.py's test_unit_gain_is_the_input_delayed_by_256 with its bound - 4 x what the float64 restatement over
    the same f32 tables shows against the delayed input - on streams with two flagged frames, cut into the GPU cases' batches"""
    win, tw = NR.tables(nr, tmp)
    t = np.arange(h * F)
    inputs = {"noise": noise(h * F), "tone": np.cos(2 * np.pi * 1000.0 * t / RATE + 0.3).astype(np.float32)}
    for name, x0 in inputs.items():
        x, flags, keep, clean = flagged(x0, h)
        want = np.zeros(len(x))
        want[NR.M:] = clean[:-NR.M]
        full = np.zeros(len(x), bool)
        full[NR.M + NR.R:] = True
        full &= keep
        own = float(np.abs(NR.restated_unit_gain(clean, win, tw) - want)[full].max())
        (got, states, gains), = NR.run_streams(nr, tmp, [(0.0, 1.0, x, flags, h, AF.batches_of(S.BATCHES, F))], "unit")
        err = float(np.abs(got.astype(np.float64) - want)[full].max())
        print(f"h {h} {name}: restatement {own:.3e} nr_stream {err:.3e} ratio {err / own:.2f}")
        S.record("nr_unit_gain", h=h, input=name, restatement_max_abs=own, nr_stream_max_abs=err, bound=4 * own)
        assert np.all(gains == 1.0) and got[~keep].tobytes() == x[~keep].tobytes()
        head = got[:NR.M][keep[:NR.M]]
        assert not head.any() and not np.signbit(head).any()
        assert err <= 4 * own, (name, err, own)


@pytest.mark.parametrize("h", HS)
def test_audio_filter_against_float64(af, tmp, h):
    """tests/test_audio_filter_host.py's test_blocked_against_float64 and test_blocked_with_a_flagged_frame with their bound - the
    blocked form's error against float64 is at most 4 x the sequential f32 form's - for every split"""
    t = np.arange(h * F)
    inputs = {"noise": noise(h * F), "tone": np.cos(2 * np.pi * 1000.0 * t / RATE + 0.3).astype(np.float32)}
    filters = {"highpass 300 + deemphasis 212": sections(af), "peak 700 q20": [ok(af, AF.PEAK, 700.0, 20.0)],
               "AF_POLE_MAX": [AF.pole_section(AF.POLE_MAX, 2 * np.pi * 700.0 / RATE, 1 - AF.POLE_MAX)]}
    for fname, secs in filters.items():
        for iname, x0 in inputs.items():
            x, flags, keep, clean = flagged(x0, h)
            T, Sq = AF.truth(secs, clean[None])[0], AF.sequential(secs, clean[None])[0]
            es = rel_rms(Sq[keep], T[keep])
            worst = 0.0
            for s, (got, states) in zip(SPLITS, AF.run_blocked(af, tmp, [(secs, x, flags, h, AF.batches_of(s, F)) for s in SPLITS], "model")):
                assert got[~keep].tobytes() == x[~keep].tobytes()
                assert np.isfinite(got[keep]).all() and np.isfinite(states).all()
                eb = rel_rms(got[keep], T[keep])
                worst = max(worst, eb)
                assert eb <= 4 * es, (fname, iname, h, s, eb, es)
            print(f"h {h} {fname:32s} {iname:6s} blocked {worst:.3e} sequential {es:.3e}")
            S.record("af_blocked", h=h, filter=fname, input=iname, blocked_rel_rms=worst, sequential_rel_rms=es, bound=4 * es)


# ---- whole blocks of zeros --------------------------------------------------------------------------------------------------------
def test_blocks_of_zeros_at_h_1200(anb, nr, tmp):
    """two flagged frames of 1200 samples: [BAD[0] h, (BAD[1] + 1) h) enters as zeros"""
    h = 1200
    z0, z1 = BAD[0] * h, (BAD[1] + 1) * h
    # the blanker: a block [256 q, 256 q + 256) inside the zeros has R[0] = 0, which anb_usable rejects: order -1, and - psdr.h -
    # no detections; the float64 model says the same
    x, flags, keep, clean = flagged(coloured(h * F, 7), h)
    (rows, st, tr), = ANB.run_streams(anb, tmp, [S.PARITY + (x, flags, h, AF.batches_of(S.BATCHES, F))], "zeros")
    y, centres, ratio, orders = ANB.model(clean.astype(np.float64), *S.PARITY)
    inside = [q for q in range(ANB.blocks_done(h * F)) if z0 <= q * ANB.B and (q + 1) * ANB.B <= z1]
    assert len(inside) > ANB.B * 4 // ANB.B and len(inside) * ANB.B > 1024, "more than one whole group of four blocks"
    assert all(tr["order"][q] == -1 for q in inside) and [q for q, o in enumerate(tr["order"]) if o == -1] == inside
    assert [q for q, o in enumerate(orders) if o == -1] == inside
    got = tr["centres"]
    assert not np.any((got >= inside[0] * ANB.B) & (got < (inside[-1] + 1) * ANB.B)), "a detection in a block of zeros"
    assert got.tolist() == centres.tolist() and len(got) >= 8
    assert not ratio[inside].any()
    # ... and what leaves the zeros' blocks is the zeros, delayed: the rows behind the flagged frames start with them
    out = rows[z1:z1 + ANB.D - 2 * ANB.B]
    assert not out.view(np.uint32).any()
    # the noise reduction: a block [128 q, 128 q + 256) inside the zeros has zero power in every bin (the windowed zeros'
    # transform); Ps decays towards 0 and never reaches it, N follows: the gain is the rule's and stays inside [g_min, 1]
    x, flags, keep, clean = flagged(noise(h * F), h)
    (rows, st, gains), = NR.run_streams(nr, tmp, [S.NRP + (x, flags, h, AF.batches_of(S.BATCHES, F))], "zeros")
    nb = (h * F - NR.M) // NR.R + 1
    assert len(gains) == nb
    zq = [q for q in range(nb) if z0 <= q * NR.R and q * NR.R + NR.M <= z1]
    assert len(zq) > 1 and not clean[zq[0] * NR.R:zq[-1] * NR.R + NR.M].any()
    win, tw = NR.tables(nr, tmp)
    for q in zq:
        assert not np.abs(np.fft.rfft(clean[q * NR.R:q * NR.R + NR.M].astype(np.float64) * win)).any(), "power is zero in every bin"
    g_min = np.float32(10 ** (-S.NRP[0] / 20))
    assert np.all((gains[zq] >= g_min) & (gains[zq] <= 1.0)), (gains[zq].min(), gains[zq].max())
    assert np.all((gains >= g_min) & (gains <= 1.0))
    # the rows that the zero blocks alone make up are zeros: any gain times nothing
    quiet = slice(zq[0] * NR.R + NR.R + NR.M, zq[-1] * NR.R + NR.R + NR.M)
    assert not rows[quiet][keep[quiet]].any() and np.isfinite(rows[keep]).all()
    S.record("zeros_h1200", h=h, anb_unusable_blocks=len(inside), nr_zero_power_blocks=len(zq), nr_gain_min=float(gains[zq].min()), nr_gain_max=float(gains[zq].max()), g_min=float(g_min))


# ---- the case table ---------------------------------------------------------------------------------------------------------------
def test_the_case_table(anb, tmp):
    assert S.LONG_N == (512, 720, 1036, 2400) and S.BATCHES == (1, 3, 2, 4) and S.MAX_BATCH == max(S.BATCHES)
    kinds = {n: create_plan_table.idft(n)[1] for n in S.LONG_N + S.SLOT_N}   # (idft asserts that the plan is accepted)
    assert kinds[720] == "fixed" and (1036 // 2) % 4 == 2 and all((n // 2) % 4 == 0 for n in (512, 720, 2400))
    for n in S.LONG_N:
        h, batches = n // 2, S.BATCHES
        assert S.window()[2] - S.window()[0] == 100 and max(batches) <= S.MAX_BATCH
        for kind in S.CPU_KINDS:
            rows, flags = S.oracle_rows(n, kind)
            assert flags[S.NAN_HALF - 1] and flags[S.NAN_HALF] and not flags[:S.NAN_HALF - 1].any() and not flags.all()
            (_, st, tr), = ANB.run_streams(anb, tmp, [S.PARITY + (rows.reshape(-1), flags, h, list(batches))], "case")
            broken = S.stream_rules(h, batches, tr)
            print(f"n {n} {kind}: frames flagged {int(flags.sum())} centres {len(tr['centres'])} unusable blocks {S.unusable_blocks(tr)} {broken}")
            S.record("case_table", n=n, h=h, kind=kind, batches=list(batches), centres=len(tr["centres"]), unusable_blocks=S.unusable_blocks(tr))
            assert not broken, (n, kind, broken)
            if h == 1200:
                assert S.unusable_blocks(tr) > 4, "the flagged frames hold more than a group of blocks"
    # the rules notice what they are there for
    assert "no batch of one frame" in S.stream_rules(360, (3, 2, 4), dict(centres=np.arange(0, 3000, 250)))
    assert "ends on a block boundary" in S.stream_rules(384, (1, 1), dict(centres=np.arange(0, 700, 250)))
    assert "no gap crosses a batch boundary" in S.stream_rules(360, (1, 3, 2, 4), dict(centres=np.array([20 + 256 * k for k in range(9)])))
    # high and sparse slots: the kept slots come in neighbouring pairs, the late one goes through the holes below it
    assert all(b == a + 1 for a, b in zip(S.KEPT[::2], S.KEPT[1::2])) and S.KEPT[-1] == S.SLOTS - 1
    assert S.LATE_SLOT not in S.KEPT and S.LATE_SLOT < S.SLOTS and any(s not in S.KEPT for s in range(S.LATE_SLOT))

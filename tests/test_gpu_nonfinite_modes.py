"""NaN and +-Inf through the client kinds that have kernels of their own: PSDR_IQ, PSDR_SAM, sideband SAM, tuned USB / LSB / IQ
(AM beside them as a control).  include/psdr.h states one NaN rule per kind - the flag is 1 if any sample of the row is NaN, the
state moves before the guard, no frame is replayed, the post chain skips flagged frames - and each of the kernels has its own
isnan / __any / flag store and its own tails around a bad frame.

Mechanism: test_gpu_state_freeze.py's.  A caller-owned linear spectrum (2^14-point IQ context, PSDR_DEMOD_K=4, 74 frames of 1e-3
Gaussian bins) goes through psdr_demod_batch_from; each client has a window of its own with a carrier of amplitude 1 in bin
floor(audio_mid), its sign following the frame's flip sign, so that SAM's C is 2 + noise.  Poisoned bins are ordinary data.

The references are independent of the kernels' arithmetic:
  * flags: a NaN bin of frame f inside the range a kind places makes EVERY output of that frame's transform NaN (NaN times any
    twiddle is NaN), so the row of f is NaN, the tail carries it into f + 1 once, and f + 2 is clean: the flag vector around
    isolated NaN frames is known in advance;
  * recovery: the same run on the clean spectrum; the state a frame starts from is one frame deep, so from f + 2 on every bit
    must be the clean twin's (rows, pwr, carrier records: the tuned phase, the carrier tail, the B' tail, AM's tail under IQ);
  * batching: the run of one frame per batch.
No tolerance anywhere: bit identity, exact flags, exact counts."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import test_gpu_sam_sideband as SB
from helpers import read_client, set_client_kind
from oracle import oracle as O
from test_gpu_parity import levels_for

pytestmark = pytest.mark.gpu

N, NFR, RATE = 1 << 14, 74, 12000
PATHS = [(360, "1"), (360, "0"), (720, "1"), (256, "1"), (1024, "1")]  # (n, PSDR_DEMOD_CHAIN)
PATH_IDS = [f"{n}-chain{c}" for n, c in PATHS]
KINDS = ("IQ", "SAM", "SAMU", "SAML", "TUSB", "TLSB", "TIQ", "AM")
MIDS = (3001, 4100, 5201, 6300, 7401, 8500, 9601, 10700)  # floor(audio_mid): odd and even (an IQ context flips odd frames of even ones)
FRACS = {"TUSB": 0.37, "TLSB": 0.81, "TIQ": 0.63}
NAN_FRAMES = (3, 12, 20, 29, 40, 52)   # client ci: + ci.  Isolated: the nearest other bad frame is four frames away
INF_FRAMES = (7, 16, 24, 33, 45, 58)   # client ci: + ci; the fourth is a run of two
RUN = 3
NANS = (complex(np.nan, 0), complex(0, np.nan), complex(np.nan, np.nan))
VALS = (complex(np.inf, 0), complex(0, np.inf), complex(-np.inf, 0), complex(np.inf, np.inf), complex(np.nan, 0), complex(np.inf, -np.inf))
SPLITS = (5, 8, 37)


def cutoff(n):
    return 500 * n // RATE


def clients(n, kinds=KINDS):
    w = n // 2 - 2
    return [(k, (m - w, m + FRACS.get(k, 0.0), m + w)) for k, m in zip(KINDS, MIDS) if k in kinds]


def side(kind):
    """+1 / -1: the kind places only the bins at and above / at and below floor(audio_mid); 0: the whole window"""
    return {"SAMU": 1, "TUSB": 1, "SAML": -1, "TLSB": -1}.get(kind, 0)


def placed_bin(kind, m, off, k):
    s = side(kind) or (1 if k % 2 == 0 else -1)
    return m + s * off


def nan_frames(ci):
    return [f + ci for f in NAN_FRAMES]


def bad_frames(ci, what):
    """every frame of client ci that holds a poisoned bin"""
    if what == "clean":
        return []
    bad = nan_frames(ci)
    if what == "placed":
        bad += [f + ci for f in INF_FRAMES] + [INF_FRAMES[RUN] + ci + 1]
    return sorted(bad)


def affected(ci, what):
    """... and the frame behind each: the tail carries a bad frame once"""
    b = bad_frames(ci, what)
    return sorted(set(b) | {f + 1 for f in b})


@functools.lru_cache(maxsize=None)
def spectrum(n, what):
    """what = "clean"; "placed": per client six isolated NaN frames and six +-Inf / mixed ones (one a run of two) in bins the
    kind places; "nan": the NaN frames alone, AM's window left clean; "unread": the NaN frames in a bin of the window that the
    kind does NOT read -
    SAM-U / tuned USB: below floor(mid) by more than the carrier's cutoff, SAM-L / tuned LSB: the mirror case, SAM (both): in
    the carrier's zeroed range (B still reads it); IQ, tuned IQ and AM are left clean"""
    rng = np.random.default_rng(77)
    spec = ((rng.standard_normal((NFR, N)) + 1j * rng.standard_normal((NFR, N))) * 1e-3).astype(np.complex64)
    odd = (np.arange(NFR) % 2 == 1)
    for m in MIDS:
        spec[:, m] = np.where(odd & (m % 2 == 0), -1.0, 1.0)  # times the flip sign: + 1 in every frame
    w = n // 2 - 2
    offs = (0, 3, 17, 40, 100, w - 1)
    for ci, (kind, m) in enumerate(zip(KINDS, MIDS)):
        if what == "clean" or (what == "nan" and kind == "AM"):
            continue
        for k, f in enumerate(nan_frames(ci)):
            if what == "unread":
                if kind in ("IQ", "TIQ", "AM"):
                    continue
                b = m + (cutoff(n) + 5) * (-side(kind) or 1)
            else:
                b = placed_bin(kind, m, offs[k], k)
            spec[f, b] = NANS[(k + ci) % len(NANS)]
        if what == "placed":
            for k, f in enumerate(f + ci for f in INF_FRAMES):
                b = placed_bin(kind, m, 5 * k + 1, k + 1)
                spec[f, b] = VALS[(k + ci) % len(VALS)]
                if k == RUN:
                    spec[f + 1, b] = VALS[(k + ci + 3) % len(VALS)]
    spec.setflags(write=False)
    return spec


def test_the_schedule_is_what_the_tests_need():
    for ci in range(len(KINDS)):
        bad, aff = bad_frames(ci, "placed"), affected(ci, "placed")
        assert max(bad) < NFR - 6 and len(nan_frames(ci)) >= 6
        for f in nan_frames(ci):  # isolated: f + 1 and f + 2 hold no poison, f - 1 and f - 2 none either
            assert not {f - 2, f - 1, f + 1, f + 2} & set(bad)
        assert 2 * len(nan_frames(ci)) >= 12 and NFR - len(aff) >= 30
        assert any((f + 1) % F == 0 for f in bad for F in SPLITS), "no bad frame ends a batch"
        assert any(f % F == 0 for f in bad for F in SPLITS), "no bad frame starts a batch"
        assert any(f % 8 % 4 == 3 for f in bad), "no chain's warm-up frame is a bad one (K = 4, batches of 8)"
    for n, _ in PATHS:
        for (kind, (l, mid, r)), m in zip(clients(n), MIDS):
            assert int(np.floor(mid)) == m and l < m - cutoff(n) - 5 and m + cutoff(n) + 5 < r and 0 < 2 * cutoff(n) < n


@functools.lru_cache(maxsize=None)
def run(n, chain, F, what, kinds=KINDS, post=False, agc=None):
    """the 74 frames in batches of F through psdr_demod_batch_from -> per client the arrays of read_client over all frames"""
    from phantomsdr_amd import AudioClient, Context
    spec = spectrum(n, what)
    saved = {k: os.environ.get(k) for k in ("PSDR_DEMOD_CHAIN", "PSDR_DEMOD_K")}
    os.environ["PSDR_DEMOD_CHAIN"], os.environ["PSDR_DEMOD_K"] = chain, "4"
    try:
        ctx = Context(N, False, levels_for(N), additional_size=n, audio_fft_size=n, audio_rate=RATE, input_format="s16", max_batch=F,
                      max_clients=len(kinds) + 3)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        if post:
            ctx.set_option(ctx.OPT_POST_CHAIN_AGC, agc)
            ctx.set_post_chain(True)
        d = ctx.dev_alloc(spec.nbytes)
        ctx.h2d(d, spec)
        cl = []
        for kind, win in clients(n, kinds):
            g = AudioClient(ctx)
            set_client_kind(g, kind)
            g.set_audio_range(*win)
            cl.append((g, kind))
        out = [[] for _ in cl]
        f = 0
        while f < NFR:
            nb = min(F, NFR - f)
            rc = ctx.lib.psdr_demod_batch_from(ctx.h, C.c_void_p(d.value + f * N * 8), N, nb, f)
            assert rc == 0, ctx.lib.psdr_last_error()
            for k, (g, kind) in enumerate(cl):
                out[k].append(tuple(x[:nb].copy() for x in read_client(g, kind, F, pcm=post)))
            f += nb
        ctx.dev_free(d)
        return [tuple(np.concatenate([b[i] for b in o]) for i in range(len(o[0]))) for o in out]
    finally:
        ctx.close()


def eq_nan(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def frames_differ(a, b):
    """indices of the rows (or entries) whose bytes differ"""
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return [f for f in range(len(a)) if a[f].tobytes() != b[f].tobytes()]


# ---- 1. flags, by definition -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,chain", PATHS, ids=PATH_IDS)
def test_flags_around_isolated_nan_frames_are_the_definitions(n, chain):
    got = run(n, chain, 1, "placed")
    for ci, (kind, _) in enumerate(clients(n)):
        nan = got[ci][2]
        aff = affected(ci, "placed")
        tag = f"n {n} chain {chain} client {ci} {kind}: flags {np.nonzero(nan)[0].tolist()}, NaN frames {nan_frames(ci)}, affected {aff}"
        assert set(np.unique(nan)) <= {0, 1}, tag
        for f in nan_frames(ci):
            assert nan[f] == 1 and nan[f + 1] == 1 and nan[f + 2] == 0, (tag, f)
        for f in range(NFR):
            if f not in aff:
                assert nan[f] == 0, (tag, f)
        # conditions on the input, not measurements: what the schedule must give every client
        assert int(nan.sum()) >= 12 and int((nan == 0).sum()) >= 30, tag
        # pwr is the frame's own sum over [l, r): NaN where a bin is NaN, untouched by the tail
        for f in nan_frames(ci):
            assert np.isnan(got[ci][1][f]) and np.isfinite(got[ci][1][f + 1]), (tag, f)


# ---- 2. bins a kind does not read ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 8])
@pytest.mark.parametrize("n,chain", PATHS, ids=PATH_IDS)
def test_a_nan_bin_outside_what_a_kind_places_reaches_pwr_alone(n, chain, F):
    """B' is built from the CLIPPED window and the carrier from bins with [cutoff, n - cutoff) ZEROED - assigned 0, not
    multiplied by 0: a NaN bin there leaves rows, flags and carrier records bit for bit the clean twin's and makes pwr NaN.  In
    a SAM (both) client the carrier's zeroed range is still part of B: the frame is flagged, the carrier records are the twin's"""
    got, clean = run(n, chain, F, "unread"), run(n, chain, F, "clean")
    for ci, (kind, _) in enumerate(clients(n)):
        g, c = got[ci], clean[ci]
        tag = f"n {n} chain {chain} F {F} client {ci} {kind}"
        nf = nan_frames(ci)
        if kind in ("IQ", "TIQ", "AM"):
            for x, y, what in zip(g, c, ("rows", "pwr", "nan flags")):
                assert x.tobytes() == y.tobytes(), f"{tag}: {what} differ though no bin of the window was touched"
            continue
        assert not c[2].any() and np.isfinite(c[0]).all(), tag
        for f in range(NFR):
            assert bool(np.isnan(g[1][f])) == (f in nf), (tag, f, "pwr")
        ok = [f for f in range(NFR) if f not in nf]
        assert g[1][ok].tobytes() == c[1][ok].tobytes(), f"{tag}: pwr"
        if len(g) > 3:
            assert g[3].tobytes() == c[3].tobytes() and g[4].tobytes() == c[4].tobytes(), \
                f"{tag}: carrier records differ in frames {frames_differ(g[3], c[3])}: the carrier read a bin it zeroes"
        if kind == "SAM":
            want = np.zeros(NFR, np.int32)
            want[affected(ci, "unread")] = 1
            assert np.array_equal(g[2], want), (tag, np.nonzero(g[2])[0].tolist())
            ok = want == 0
            assert g[0][ok].tobytes() == c[0][ok].tobytes(), f"{tag}: unflagged rows"
        else:
            assert not g[2].any(), f"{tag}: flags {np.nonzero(g[2])[0].tolist()} for NaN bins {nf} the kind does not place"
            assert g[0].tobytes() == c[0].tobytes(), f"{tag}: rows differ in frames {frames_differ(g[0], c[0])}"


# ---- 3. recovery -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 8])
@pytest.mark.parametrize("n,chain", PATHS, ids=PATH_IDS)
def test_two_frames_behind_a_bad_frame_every_bit_is_the_clean_twins(n, chain, F):
    got, clean = run(n, chain, F, "placed"), run(n, chain, F, "clean")
    for ci, (kind, _) in enumerate(clients(n)):
        ok = np.array([f not in affected(ci, "placed") for f in range(NFR)])
        assert ok[-6:].all() and ok.sum() >= 30
        assert not clean[ci][2].any() and np.abs(clean[ci][0]).max() > 0
        for x, y, what in zip(got[ci], clean[ci], ("rows", "pwr", "nan flags", "carrier level", "carrier offset")):
            bad = [f for f in frames_differ(x, y) if ok[f]]
            assert not bad, f"n {n} chain {chain} F {F} client {ci} {kind}: {what} differ from the clean twin in frames {bad}; bad frames {bad_frames(ci, 'placed')}"
        if len(clean[ci]) > 3:
            assert clean[ci][3][1:].min() > 1.5, "the clean carrier is not well away from zero"


# ---- 4. batching -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,chain", PATHS, ids=PATH_IDS)
def test_batches_give_the_flags_pwr_and_served_rows_of_one_frame_per_batch(n, chain):
    want = run(n, chain, 1, "placed")
    for F in SPLITS:
        got = run(n, chain, F, "placed")
        for ci, (kind, _) in enumerate(clients(n)):
            tag = f"n {n} chain {chain} F {F} client {ci} {kind} (bad frames {bad_frames(ci, 'placed')})"
            g, w = got[ci], want[ci]
            assert np.array_equal(g[2], w[2]), (tag, "flags", np.nonzero(g[2] != w[2])[0].tolist())
            assert eq_nan(g[1], w[1]), (tag, "pwr")
            ok = w[2] == 0  # (the row of a flagged frame is not served)
            assert g[0][ok].tobytes() == w[0][ok].tobytes(), (tag, "rows", [f for f in frames_differ(g[0], w[0]) if ok[f]])
            for i in range(3, len(g)):
                assert eq_nan(g[i][ok], w[i][ok]), (tag, "carrier records")


# ---- 5. post chain ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chain,agc", [("1", 1), ("1", 0), ("0", 1)])
def test_post_chain_skips_the_flagged_frames_of_the_new_kinds(chain, agc):
    """SAM, SAM-U and tuned USB with NaN frames, a clean AM client in the same wave of the chain's kernels: flagged frames have
    zero PCM rows and leave no trace - the oracle's chain fed the SURVIVING float rows alone gives the PCM, bit for bit"""
    n, kinds = 360, ("SAM", "SAMU", "TUSB", "AM")
    got = run(n, chain, 8, "nan", kinds=kinds, post=True, agc=agc)
    total = 0
    for (kind, _), g in zip(clients(n, kinds), got):
        ci = KINDS.index(kind)
        audio, nan, pcm = g[0], g[2], g[-1]
        want = np.zeros(NFR, np.int32)
        if kind != "AM":
            want[affected(ci, "nan")] = 1
        assert np.array_equal(nan, want), (kind, np.nonzero(nan)[0].tolist())
        assert kind == "AM" or int(nan.sum()) >= 5
        ch = O.PostChain(RATE)
        for f in range(NFR):
            if nan[f]:
                assert not pcm[f].any(), f"{kind} frame {f}: a flagged frame has PCM"
                continue
            ref = ch.process(audio[f])
            assert np.array_equal(pcm[f], ref), f"chain {chain} agc {agc} {kind} frame {f}: {np.count_nonzero(pcm[f] != ref)} samples differ"
            total += int(np.count_nonzero(ref))
    assert total > 1000, "the AGC never opened: the test did not exercise the chain"


# ---- 6. the whole path on a real context -----------------------------------------------------------------------------------

BAD_HALVES = ((3, 17, np.inf), (7, 100, -np.inf), (11, 5, np.nan), (14, 9, np.inf), (18, 1, -np.inf), (22, 4000, np.nan))


@functools.lru_cache(maxsize=None)
def run_real(n, F):
    """the 2^13-point real shape, f32 input: test_gpu_sam_sideband.py's stream with +-Inf / NaN SAMPLES in six half-frames (a
    half-frame is part of two frames), all eight kinds on the carrier, 25 frames in batches of F"""
    from phantomsdr_amd import AudioClient, Context
    halves = SB.stream(1, n)[1].astype(np.float32).copy()
    for h, k, v in BAD_HALVES:
        halves[h, k] = v
    raw = halves.reshape(-1).copy()
    wins = SB.windows(n)[:2]
    saved = os.environ.get("PSDR_DEMOD_K")
    os.environ["PSDR_DEMOD_K"] = "4"
    try:
        ctx = Context(SB.SHAPES[1], True, SB.LEVELS, additional_size=n, audio_fft_size=n, audio_rate=RATE, input_format="f32",
                      max_batch=F, max_clients=len(KINDS))
    finally:
        os.environ.pop("PSDR_DEMOD_K") if saved is None else os.environ.__setitem__("PSDR_DEMOD_K", saved)
    try:
        d = ctx.dev_alloc(raw.nbytes)
        ctx.h2d(d, raw)
        cl = []
        for i, kind in enumerate(KINDS):
            l, mid, r = wins[i % 2]
            g = AudioClient(ctx)
            set_client_kind(g, kind)
            g.set_audio_range(l, float(np.floor(mid)) + FRACS.get(kind, mid - np.floor(mid)), r)
            cl.append((g, kind))
        out = [[] for _ in cl]
        f = 0
        while f < SB.NF:
            nb = min(F, SB.NF - f)
            ctx.process_batch(d, nb, offset_bytes=f * ctx.half_frame_bytes())
            ctx.demod_batch(f)
            for k, (g, kind) in enumerate(cl):
                out[k].append(tuple(x[:nb].copy() for x in read_client(g, kind, F)))
            f += nb
        ctx.dev_free(d)
        return [tuple(np.concatenate([b[i] for b in o]) for i in range(len(o[0]))) for o in out]
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [360, 256])
def test_inf_and_nan_samples_on_a_real_context_batched_equals_frame_by_frame(n):
    want = run_real(n, 1)
    for kind, w in zip(KINDS, want):
        print(f"n {n} {kind}: flagged frames {np.nonzero(w[2])[0].tolist()}")
        assert int(w[2].sum()) >= 10 and not w[2][:2].any(), kind
    for F in (6, 19):
        got = run_real(n, F)
        for kind, g, w in zip(KINDS, got, want):
            tag = f"n {n} F {F} {kind}"
            assert np.array_equal(g[2], w[2]), (tag, "flags", np.nonzero(g[2] != w[2])[0].tolist())
            assert eq_nan(g[1], w[1]), (tag, "pwr")
            ok = w[2] == 0
            assert ok.any() and g[0][ok].tobytes() == w[0][ok].tobytes(), (tag, "rows", [f for f in frames_differ(g[0], w[0]) if ok[f]])

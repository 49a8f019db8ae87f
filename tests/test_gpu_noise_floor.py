"""Per-client noise floor on the GPU (include/psdr.h: psdr_client_set_noise_floor, psdr_client_set_squelch_reference,
psdr_read_noise, psdr_fetched_noise).

Truth: the GPU's own spectrum, read with psdr_read_spectrum, goes through the host table program (tests/noise_plan_table.cpp: the
header's own definitions and std::fmaf); psdr_read_noise must equal its W rows bit for bit, and the relative squelch's flags its
walk over the GPU's own pwr and W bits.  There is no tolerance anywhere.

Shapes: 4096-point IQ and 8192-point real (R = 4096), f32 input, audio_rate = period * audio_fft_size with period 2 .. 4, batches
of 1 to 12 frames.  Input: unit noise plus one tone inside the clients' windows, keyed by half-frames."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_noise_host as H
from helpers import assert_same_bits, read_client, row_names, set_client_kind

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = {"iq": (False, 1 << 12, 1000), "real": (True, 1 << 13, 1000)}  # is_real, N, the windows' first bin
LEVELS, MAXB = 3, 12
INVALID, STATE, NO_DATA = -1, -4, -7


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("noise_gpu"), "noise_plan_table")


@functools.lru_cache(maxsize=None)
def stream(shape, key, amp=6.0, seed=3):
    """f32 half-frames, flat: unit noise plus a tone on client bin L0 + 20, on in the half-frames whose key is 1"""
    is_real, N, L0 = SHAPES[shape]
    rng = np.random.default_rng(seed)
    ns = len(key) * (N // 2)
    t = np.arange(ns, dtype=np.float64)
    gate = np.repeat(np.asarray(key, np.float64), N // 2)
    if is_real:
        return (rng.standard_normal(ns) + gate * 2.0 * amp * np.cos(2 * np.pi * (L0 + 20) * t / N)).astype(F32)
    x = rng.standard_normal(ns) + 1j * rng.standard_normal(ns)
    x += gate * amp * np.exp(2j * np.pi * ((L0 + 20 + N // 2 + 1) % N) * t / N)  # client bin c is frequency index (c + N/2 + 1) mod N
    return x.astype(np.complex64).view(F32).copy()


class Rig:
    def __init__(self, shape, n, period, max_clients=8, key=None, post=False, nframes=24):
        from phantomsdr_amd import Context
        is_real, N, _ = SHAPES[shape]
        self.shape, self.n, self.period = shape, n, period
        self.ctx = Context(N, is_real, LEVELS, additional_size=n, audio_fft_size=n, audio_rate=period * n, input_format="f32", max_batch=MAXB,
                           max_clients=max_clients)
        raw = stream(shape, tuple(key) if key is not None else (0,) * (nframes + 1))
        self.d = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.d, raw)
        if post:
            self.ctx.set_post_chain(True)
        self.frame, self.spec, self.bufs = 0, [], [self.d]

    def add(self, kind, length=None, l=None, noise=True):
        from phantomsdr_amd import AudioClient
        g = AudioClient(self.ctx)
        set_client_kind(g, kind)
        l = SHAPES[self.shape][2] if l is None else l
        length = self.n if length is None else length
        g.set_audio_range(l, l + length / 2 + 0.25, l + length)
        if noise:
            g.set_noise_floor(True)
        return g

    def transform(self, F):
        """the next F frames through the FFT; their spectra are kept (the truth's input) in the coordinates of a client's l and r:
        psdr_read_spectrum delivers k order, and client bin c of an IQ spectrum is bin k = (c + N/2 + 1) mod N"""
        is_real, N, _ = SHAPES[self.shape]
        self.ctx.process_batch(self.d, F, offset_bytes=self.frame * self.ctx.half_frame_bytes())
        for f in range(F):
            k = self.ctx.read_spectrum(f)
            self.spec.append(k[:N // 2 + 1].copy() if is_real else np.roll(k[:N], -(N // 2 + 1)))

    def batch(self, F):
        self.transform(F)
        self.ctx.demod_batch(self.frame)
        self.frame += F

    def batch_from(self, spec, first_bin=0, nbins=None):
        """F frames of a spectrum the caller hands over, linear: spec complex64 [F][nbins]"""
        from phantomsdr_amd._lib import check
        spec = np.ascontiguousarray(spec, np.complex64)
        F, nb = spec.shape
        d = self.ctx.dev_alloc(spec.nbytes)
        self.bufs.append(d)
        self.ctx.h2d(d, spec)
        check(self.ctx.lib.psdr_demod_batch_from_band(self.ctx.h, d, nb, first_bin, nb, F, self.frame))
        self.ctx.last_nframes = self.ctx.last_demod_frames = F
        self.frame += F

    def close(self):
        self.ctx.synchronize()
        for d in self.bufs:
            self.ctx.dev_free(d)
        self.ctx.close()


def truth(exe, spec, l, r, period, lens):
    """the host program over the frames' window bins, from a zero state, as batches of `lens` -> (W f32[F], the state's fields)"""
    x = np.stack([s[l:r] for s in spec]) if r > l else np.zeros((len(spec), 0), np.complex64)
    line = H.frames_line(x, period, lens) if r > l else "frames 0 %d %d %d %s" % (period, len(spec), len(lens), " ".join(map(str, lens)))
    g = H.fields(H.run(exe, line + "\n").splitlines()[0])
    return H.from_bits(g["bits"]), g


def same_bits(a, b):
    return np.asarray(a, F32).tobytes() == np.asarray(b, F32).tobytes()


CASES = [("iq", 360, 4), ("real", 360, 3), ("iq", 128, 2)]


@pytest.mark.parametrize("shape,n,period", CASES)
def test_w_is_the_host_programs_on_the_gpus_own_spectrum(exe, shape, n, period):
    """window lengths 1, 5, 64, 65 and audio_fft_size, one client kind each; 12 frames as 5 + 7, a retune of two clients, 12 more as
    12 x 1: at least three evaluations on either side"""
    L0 = SHAPES[shape][2]
    A = Rig(shape, n, period)
    try:
        plan = [("USB", 1), ("AM", 5), ("FM", 64), ("SAM" if n == 360 else "LSB", 65), ("IQ", n), ("TUSB", 64)]
        cl = [A.add(kind, length) for kind, length in plan]
        wins = [(L0, L0 + length) for _, length in plan]
        starts = [0] * len(cl)
        got = [[] for _ in cl]
        sizes = [5, 7] + [1] * 12
        for bi, F in enumerate(sizes):
            if bi == 2:  # the retune: l alone, and r alone - both start over; a change of audio_mid alone and of the mode do not
                for i, (dl, dr) in ((1, (3, 3)), (2, (0, -1))):
                    wins[i] = (wins[i][0] + dl, wins[i][1] + dr)
                    cl[i].set_audio_range(wins[i][0], wins[i][0] + 1.5, wins[i][1])
                    starts[i] = 12
                cl[3].set_audio_range(wins[3][0], wins[3][0] + 11.75, wins[3][1])
                set_client_kind(cl[5], "USB")
            A.batch(F)
            for i, g in enumerate(cl):
                got[i].append(g.read_noise(F).copy())
        for i, (g, (l, r)) in enumerate(zip(cl, wins)):
            w = np.concatenate(got[i])
            if starts[i]:
                first, _ = truth(exe, A.spec[:12], L0, L0 + plan[i][1], period, [5, 7])
                rest, _ = truth(exe, A.spec[12:], l, r, period, [1] * 12)
                want = np.concatenate([first, rest])
            else:
                want, _ = truth(exe, A.spec, l, r, period, sizes)
            assert w.dtype == F32 and same_bits(w, want), (plan[i], np.nonzero(w.view(np.uint32) != want.view(np.uint32))[0].tolist())
            assert not w[:period - 1].any() and (w[period - 1:12] > 0).all() and np.isfinite(w).all(), plan[i]
            assert 12 // period >= 3  # at least three evaluations on either side of the retune
            if starts[i]:
                assert not w[12:12 + period - 1].any() and w[12 + period - 1] > 0  # started over at the retune
    finally:
        A.close()


def run_split(exe, shape, n, period, sizes, key):
    A = Rig(shape, n, period, key=key)
    try:
        cl = [A.add("USB", 64), A.add("AM", n), A.add("IQ", 65)]
        for g in cl:
            g.set_squelch(True, 9.0, 6.0, 2, 1)
            g.set_squelch_reference("noise")
        W, flags, pwr = [[] for _ in cl], [[] for _ in cl], [[] for _ in cl]
        for F in sizes:
            A.batch(F)
            for i, g in enumerate(cl):
                W[i].append(g.read_noise(F).copy())
                flags[i].append(g.read_squelch(F).copy())
                pwr[i].append((g.read_iq(F) if i == 2 else g.read_audio(F))[1].copy())
        return [np.concatenate(v) for v in W], [np.concatenate(v) for v in flags], [np.concatenate(v) for v in pwr], A.spec
    finally:
        A.close()


def rel_flags(exe, pwr, W, open_db, close_db, attack, hang):
    import squelch_model as M
    line = "relwalk %d %d %d %d %d %s %s\n" % (int(H.bits(M.threshold(open_db))), int(H.bits(M.threshold(close_db))), attack, hang, len(pwr), H.bit_list(pwr),
                                               H.bit_list(W))
    return np.array([int(ch) for ch in H.fields(H.run(exe, line).splitlines()[0])["flags"]], np.int32)


@pytest.mark.parametrize("shape,n,period", [("iq", 360, 4), ("real", 128, 3)])
def test_split_invariance(exe, shape, n, period):
    """the same 12 frames as 1 x 12, 12 x 1 and 5 + 7: the same W bits and the same squelch flags"""
    key = (0,) * 7 + (1,) * 3 + (0,) * 3
    runs = {name: run_split(exe, shape, n, period, sizes, key) for name, sizes in (("1x12", [12]), ("12x1", [1] * 12), ("5+7", [5, 7]))}
    W0, f0, p0, spec = runs["1x12"]
    L0 = SHAPES[shape][2]
    for name, (W, fl, pw, _) in runs.items():
        for i in range(3):
            assert same_bits(W[i], W0[i]) and np.array_equal(fl[i], f0[i]) and same_bits(pw[i], p0[i]), (name, i)
    for i, length in enumerate((64, n, 65)):
        want, _ = truth(exe, spec, L0, L0 + length, period, [12])
        assert same_bits(W0[i], want), i
        assert np.array_equal(f0[i], rel_flags(exe, p0[i], W0[i], 9.0, 6.0, 2, 1)), i
    assert f0[0].any() and not f0[0].all()  # the tone opens the gate, the noise alone does not hold it


def test_band_layout(exe):
    """psdr_demod_batch_from_band: a context that never transforms, fed one linear band with first_bin != 0, the client inside it"""
    from phantomsdr_amd._lib import check
    A, B = Rig("iq", 360, 4), Rig("iq", 360, 4)
    try:
        first, bins = 900, 700
        g = B.add("AM", 65, l=1010)
        h = B.add("IQ", 360, l=first)  # from the band's first bin
        for F in (5, 7):
            A.transform(F)
            d = A.ctx.dev_alloc(F * bins * 8)
            A.bufs.append(d)
            check(A.ctx.lib.psdr_pack_band(A.ctx.h, F, first, bins, d, bins))
            A.ctx.synchronize()
            band = np.empty((F, bins), np.complex64)
            A.ctx.d2h(band, d)
            assert np.array_equal(band[0].view(np.uint32), A.spec[-F][first:first + bins].view(np.uint32))
            B.batch_from(band, first, bins)
            A.frame += F
            want = truth(exe, A.spec, 1010, 1075, 4, [5, 7][:len(A.spec) // 6 + 1])[0][-F:]
            assert same_bits(g.read_noise(F), want)
            assert same_bits(h.read_noise(F), truth(exe, A.spec, first, first + 360, 4, [len(A.spec)])[0][-F:])
        assert g.read_noise(7)[-1] > 0
    finally:
        A.close()
        B.close()


def test_non_finite_bins(exe):
    """a NaN and an Inf bin inside the window, above the selected rank: W follows the model and stays finite.  Then every bin Inf for
    8 evaluations: an Inf entry is never the minimum, so W holds the last finite estimates while they are in the ring and is 0 once
    all 8 entries are non-finite - and comes back with the next finite evaluation"""
    n, period = 128, 2
    A, B = Rig("iq", n, period, nframes=24), Rig("iq", n, period, nframes=24)
    try:
        L0 = SHAPES["iq"][2]
        g = B.add("USB", 64)
        k = B.add("IQ", 5, l=L0 + 70)
        for F in (12, 12):
            A.transform(F)
            A.frame += F
        spec = np.stack(A.spec)
        spec[1, L0 + 60], spec[2, L0 + 61] = np.nan, np.inf
        spec[4:20, L0:L0 + 64] = np.inf  # evaluations 2 .. 9
        spec[5, L0 + 72] = np.nan
        got, gk = [], []
        for a, b in ((0, 11), (11, 12), (12, 24)):
            B.batch_from(spec[a:b])
            got.append(g.read_noise(b - a).copy())
            gk.append(k.read_noise(b - a).copy())
        w, wk = np.concatenate(got), np.concatenate(gk)
        want, st = truth(exe, list(spec), L0, L0 + 64, period, [11, 1, 12])
        assert same_bits(w, want), (w, want)
        assert same_bits(wk, truth(exe, list(spec), L0 + 70, L0 + 75, period, [11, 1, 12])[0])
        assert np.isfinite(w).all() and w[3] > 0 and w[15] == w[3]  # the two finite evaluations stand while both are in the ring ...
        assert w[17] > 0 and w[18] > 0 and w[19] == 0 and w[20] == 0 and w[21] > 0  # ... 0 only once all 8 entries are non-finite (frame 19)
        assert st["fill"] == "8" and np.isinf(H.from_bits(st["ring"])).sum() == 6
    finally:
        A.close()
        B.close()


def test_relative_squelch_and_the_post_chain(exe):
    """a level step across the threshold with an attack and a hang: the flags are the host program's walk with the per-frame
    thresholds t * W_f, the PCM behind the post chain is zero exactly on the closed frames"""
    n, period, nf = 360, 4, 36
    key = (0,) * 13 + (1,) * 8 + (0,) * 6 + (1,) * 2 + (0,) * 8
    A = Rig("iq", n, period, key=key, post=True, nframes=nf)
    try:
        g = A.add("AM", 64)
        g.set_squelch(True, 9.0, 6.0, 2, 2)
        g.set_squelch_reference("noise")
        e = A.add("USB", 64)
        e.set_squelch(True, 9.0, 9.0, 1, 0)
        e.set_squelch_reference("noise")
        out = {c: dict(W=[], fl=[], pw=[], pcm=[]) for c in (g, e)}
        for F in (12, 5, 7, 12):
            A.batch(F)
            for c in (g, e):
                o = out[c]
                o["W"].append(c.read_noise(F).copy()), o["fl"].append(c.read_squelch(F).copy())
                o["pw"].append(c.read_audio(F)[1].copy()), o["pcm"].append(c.read_pcm(F).copy())
        for c, params in ((g, (9.0, 6.0, 2, 2)), (e, (9.0, 9.0, 1, 0))):
            o = {k: np.concatenate(v) for k, v in out[c].items()}
            want = rel_flags(exe, o["pw"], o["W"], *params)
            with np.errstate(all="ignore"):
                print("snr dB", np.round(10 * np.log10(o["pw"] / o["W"]), 1).tolist(), "flags", o["fl"].tolist())
            assert np.array_equal(o["fl"], want), np.nonzero(o["fl"] != want)[0].tolist()
            closed = o["fl"] == 0
            assert closed.any() and (~closed).any()
            assert not o["pcm"][closed].any()
            assert all(o["pcm"][f].any() for f in np.nonzero(~closed)[0][4:])  # (the chain's look-ahead is silent for its first 320 samples)
        fl = np.concatenate(out[e]["fl"])
        assert fl[:period - 1].all()  # before the first evaluation W = 0: the gate is open for any power that is not NaN
        fl = np.concatenate(out[g]["fl"])
        assert fl[0] == 0 and not fl[8:12].any() and fl[14:20].all()  # the attack; closed on the noise alone; open on the tone
    finally:
        A.close()


MIXED = ("USB", "AM", "FM", "SAM", "IQ", "TUSB")


def test_nothing_else_moves():
    """A: one client of each kind with the noise floor on - AM and SAM with a noise-referenced squelch, FM with an absolute one -
    plus an absolute-squelch client and a plain client; B: the same clients in the same slots without the noise floor.  Rows, pwr,
    NaN flags, carrier records and (over three batches) the carried demodulation state are the same bytes"""
    key = (0, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 1, 0)
    A, B = Rig("iq", 360, 4, max_clients=9, key=key), Rig("iq", 360, 4, max_clients=9, key=key)
    try:
        kinds = list(MIXED) + ["AM", "USB"]
        ga = [A.add(k, 100, noise=i < len(MIXED)) for i, k in enumerate(kinds)]
        gb = [B.add(k, 100, noise=False) for k in kinds]
        for i in (1, 2, 3, 6):
            ga[i].set_squelch(True, 3.0, 0.0, 1, 1), gb[i].set_squelch(True, 3.0, 0.0, 1, 1)
        ga[1].set_squelch_reference("noise"), ga[3].set_squelch_reference("noise")
        for F in (5, 7, 12):
            A.batch(F), B.batch(F)
            for i, kind in enumerate(kinds):
                assert_same_bits(read_client(ga[i], kind, F), read_client(gb[i], kind, F), f"{kind} in slot {i}", row_names(kind))
                assert same_bits(gb[i].read_noise(F), np.zeros(F, F32))
            for i in (2, 6):  # the absolute squelch is the squelch as it was
                assert np.array_equal(ga[i].read_squelch(F), gb[i].read_squelch(F))
            assert ga[7].read_squelch(F).all() and not ga[7].read_noise(F).any() and ga[0].read_noise(F)[-1] > 0
    finally:
        A.close()
        B.close()


def test_fetch_carries_the_rows():
    from phantomsdr_amd import PsdrError
    A = Rig("iq", 360, 4, max_clients=8)
    try:
        cl = [A.add(k, 64, noise=i in (1, 5)) for i, k in enumerate(("USB", "AM", "IQ", "FM", "USB", "IQ", "SAM", "USB"))]
        assert [g.id for g in cl] == list(range(8))
        for bi, F in enumerate((5, 7, 12)):
            A.batch(F)
            if bi == 1:
                A.ctx.fetch_begin(A.ctx.FETCH_AUDIO)
                A.ctx.fetch_end()
            else:
                A.ctx.fetch_batch()
            for i, g in enumerate(cl):
                got = np.array([A.ctx.fetched_noise(g.id, f) for f in range(F)], F32)
                assert same_bits(got, g.read_noise(F)), (bi, i)
                assert (i in (1, 5)) == bool(got.any()) or bi == 0
            assert A.ctx.fetched_noise(5, F - 1) > 0 or bi == 0
            for bad in ((8, 0), (-1, 0), (1, F), (1, -1)):  # the id first, then the frame: as psdr_fetched_squelch
                w = C.c_float(7.0)
                assert A.ctx.lib.psdr_fetched_noise(A.ctx.h, bad[0], bad[1], C.byref(w)) == A.ctx.lib.psdr_fetched_squelch(A.ctx.h, bad[0], bad[1], C.byref(C.c_int32(0))) == INVALID
                assert w.value == 7.0
            assert A.ctx.lib.psdr_fetched_noise(A.ctx.h, 1, 0, None) == INVALID
        A.ctx.fetch_begin(A.ctx.FETCH_WATERFALL)  # a fetch without audio bits carries none
        A.ctx.fetch_end()
        with pytest.raises(PsdrError) as e:
            A.ctx.fetched_noise(1, 0)
        assert e.value.code == STATE
        with pytest.raises(PsdrError) as e2:
            A.ctx.fetched_squelch(1, 0)
        assert e2.value.code == STATE
    finally:
        A.close()


def test_errors_change_nothing(exe):
    from phantomsdr_amd import AudioClient, Context, PsdrError
    A = Rig("iq", 360, 4, max_clients=4)
    try:
        lib, h = A.ctx.lib, A.ctx.h
        g, p = A.add("USB", 64), A.add("AM", 64, noise=False)
        g.set_squelch(True, 9.0, 6.0, 1, 0)
        assert lib.psdr_client_set_noise_floor(h, 3, 1) == INVALID and lib.psdr_client_set_noise_floor(h, -1, 0) == INVALID
        assert lib.psdr_client_set_squelch_reference(h, 3, 1) == INVALID and lib.psdr_client_set_squelch_reference(h, g.id, 2) == INVALID
        assert lib.psdr_client_set_squelch_reference(h, p.id, 1) == STATE  # its noise floor is off
        g.set_squelch_reference("noise")
        assert lib.psdr_client_set_noise_floor(h, g.id, 0) == STATE  # the squelch would lose its reference
        with pytest.raises(PsdrError) as e:
            g.read_noise(5)
        assert e.value.code == STATE  # no batch yet
        A.batch(5), A.batch(7)
        W = g.read_noise(7)
        want, _ = truth(exe, A.spec, g.l, g.r, 4, [5, 7])
        assert same_bits(W, want[5:]) and W[-1] > 0  # nothing of the refused calls took: still on, still from the first batch's state
        assert same_bits(p.read_noise(7), np.zeros(7, F32))  # the feature off: zeros
        with pytest.raises(PsdrError) as e:
            g.read_noise(6)
        assert e.value.code == INVALID
        late = AudioClient(A.ctx)
        with pytest.raises(PsdrError) as e:
            late.read_noise(7)
        assert e.value.code == NO_DATA  # added after the batch
        A.ctx.fetch_batch()
        with pytest.raises(PsdrError) as e:
            A.ctx.fetched_noise(late.id, 0)
        assert e.value.code == NO_DATA
        g.set_squelch_reference("absolute"), g.set_noise_floor(False)
        A.batch(5)
        assert same_bits(g.read_noise(5), np.zeros(5, F32))
    finally:
        A.close()
    B = Context(1 << 12, False, LEVELS, audio_fft_size=360, audio_rate=0, max_clients=1)  # no audio rate: no period
    try:
        c = AudioClient(B)
        assert B.lib.psdr_client_set_noise_floor(B.h, c.id, 1) == STATE and B.lib.psdr_client_set_noise_floor(B.h, c.id + 1, 1) == INVALID
        assert B.lib.psdr_client_set_squelch_reference(B.h, c.id, 1) == STATE and B.lib.psdr_client_set_squelch_reference(B.h, c.id, 0) == 0
    finally:
        B.close()

"""Per-client notch filters on the GPU (include/psdr.h: psdr_client_set_notch, psdr_client_set_auto_notch, psdr_read_notches).

The defining rule is the reference for everything here: a client with notches is bit-identical to the same client without notches
on a spectrum whose notched bins are +0.0 + 0.0i.  Context A transforms the stream and demodulates notched clients; the test
copies A's spectrum (psdr_spectrum_device_ptr), zeroes the notched bins on the host and hands the copy to context B through
psdr_demod_batch_from, where the same clients have no notch.  No tolerance anywhere: bytes.

Shapes: a 2^14-point IQ context and a 2^15-point real one (natural spectrum layout), f32 input, max_batch 6, seeded noise plus
tones.  The detector's amplitudes are chosen so that every comparison against 16 x mean or 8 x mean has a factor of two of margin
whether or not the forward transform's window costs a tone a third of its power against the noise (see detector_stream)."""
import ctypes as C

import numpy as np
import pytest

from helpers import CLIENT_KINDS, assert_same_bits, read_client, row_names, set_client_kind

pytestmark = pytest.mark.gpu

SHAPES = {False: 1 << 14, True: 1 << 15}
LEVELS, RATE, MAXB = 4, 12000, 6
KINDS = tuple(CLIENT_KINDS)
L0, WIDTH, MIDOFF = 5000, 120, 60.3   # every client's window [L0, L0 + WIDTH), audio_mid = L0 + MIDOFF
# the two notch sets: (inside the window, straddling l) and (covering floor(audio_mid), wholly outside)
SETS = (((L0 + 80.0, 3.0), (float(L0), 4.0)), ((L0 + 60.0, 2.0), (L0 + 500.0, 3.0)))


def interval(centre, width):
    first, end = int(np.floor(centre - width / 2 + 0.5)), int(np.floor(centre + width / 2 + 0.5))
    return first, max(end, first + 1)


def stream(is_real, nhalves, seed, tones=()):
    """f32 half-frames [nhalves][...]: unit noise plus tones (bin of the spectrum's k order, amplitude); IQ: complex samples"""
    N = SHAPES[is_real]
    rng = np.random.default_rng(seed)
    ns = nhalves * (N // 2)
    t = np.arange(ns, dtype=np.float64)
    if is_real:
        x = rng.standard_normal(ns)
        for k, a in tones:
            x += a * np.cos(2 * np.pi * k * t / N)
        return x.astype(np.float32)
    x = rng.standard_normal(ns) + 1j * rng.standard_normal(ns)
    for k, a in tones:
        x += a * np.exp(2j * np.pi * k * t / N)
    return x.astype(np.complex64).view(np.float32)


class Ctx:
    def __init__(self, is_real, n, max_clients, raw=None, post=False):
        from phantomsdr_amd import Context
        self.is_real, self.n = is_real, n
        self.ctx = Context(SHAPES[is_real], is_real, LEVELS, additional_size=n, audio_fft_size=n, audio_rate=RATE,
                           input_format="f32", max_batch=MAXB, max_clients=max_clients)
        self.nbins = self.ctx.nbins
        self.d = None
        if raw is not None:
            self.d = self.ctx.dev_alloc(raw.nbytes)
            self.ctx.h2d(self.d, raw)
        self.dspec = self.ctx.dev_alloc(MAXB * self.nbins * 8)
        if post:
            self.ctx.set_post_chain(True)
        self.frame = 0

    def add(self, kind, win):
        from phantomsdr_amd import AudioClient
        g = AudioClient(self.ctx)
        set_client_kind(g, kind)
        g.set_audio_range(*win)
        return g

    def batch(self, F):
        """transform and demodulate the next F frames; -> the spectrum [F][nbins] complex64, copied from the device pointer"""
        self.ctx.process_batch(self.d, F, offset_bytes=self.frame * self.ctx.half_frame_bytes())
        self.ctx.demod_batch(self.frame)
        self.ctx.synchronize()
        spec = np.empty((F, self.nbins), np.complex64)
        for f in range(F):
            p, nb = C.c_void_p(), C.c_size_t()
            assert self.ctx.lib.psdr_spectrum_device_ptr(self.ctx.h, f, C.byref(p), C.byref(nb)) == 0 and nb.value == self.nbins
            self.ctx.d2h(spec[f], p)
        self.frame += F
        return spec

    def batch_from(self, spec):
        F = spec.shape[0]
        self.ctx.h2d(self.dspec, np.ascontiguousarray(spec))
        rc = self.ctx.lib.psdr_demod_batch_from(self.ctx.h, self.dspec, self.nbins, F, self.frame)
        assert rc == 0, rc
        self.ctx.last_nframes = self.ctx.last_demod_frames = F
        self.frame += F

    def close(self):
        if self.d is not None:
            self.ctx.dev_free(self.d)
        self.ctx.dev_free(self.dspec)
        self.ctx.close()


def window(kind):
    mid = L0 + MIDOFF
    return (L0, mid, L0 + WIDTH)


def zeroed(spec, notches):
    out = spec.copy()
    for c, w in notches:
        a, b = interval(c, w)
        a, b = max(a, 0), min(b, out.shape[1])
        if b > a:
            out[:, a:b] = 0
    return out


def tones_for(is_real):
    # a carrier on floor(audio_mid), a tone inside the first set's inner notch, one beside it
    bins = ((L0 + 60, 0.5), (L0 + 80, 0.4), (L0 + 95, 0.2))
    if is_real:
        return bins
    N = SHAPES[False]  # client bin c of an IQ spectrum is frequency index (c + N/2 + 1) mod N
    return tuple(((c + N // 2 + 1) % N, a) for c, a in bins)


RULE_CASES = [(r, n, c, False) for r in (False, True) for n, c in ((360, "1"), (360, "0"), (248, "1"), (720, "1"))] + [(False, 360, "1", True), (True, 360, "1", True)]


@pytest.mark.parametrize("is_real,n,chain,post", RULE_CASES,
                         ids=[f"{'real' if r else 'iq'}-{n}-chain{c}{'-post' if p else ''}" for r, n, c, p in RULE_CASES])
def test_defining_rule_bit_for_bit(is_real, n, chain, post, monkeypatch):
    """every client kind, two notch sets, three consecutive batches (6 + 6 + 5 frames: the tails carry): A's notched clients
    against B's plain clients on the zeroed spectrum - rows, pwr, NaN flags, carrier records, PCM, as bytes"""
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    sizes = (6, 6, 5)
    raw = stream(is_real, sum(sizes) + 1, 11, tones_for(is_real))
    A = Ctx(is_real, n, 2 * len(KINDS) + 1, raw, post=post)
    Bs = [Ctx(is_real, n, len(KINDS) + 1, post=post) for _ in SETS]
    try:
        ga, gb = [], []
        for si, notches in enumerate(SETS):
            for kind in KINDS:
                g = A.add(kind, window(kind))
                for idx, (c, w) in enumerate(notches):
                    g.set_notch(idx, c, w)
                ga.append((si, kind, g))
                gb.append(Bs[si].add(kind, window(kind)))
        for bi, F in enumerate(sizes):
            spec = A.batch(F)
            for si, notches in enumerate(SETS):
                Bs[si].batch_from(zeroed(spec, notches))
            for (si, kind, g), h in zip(ga, gb):
                a, b = read_client(g, kind, F, pcm=post), read_client(h, kind, F, pcm=post)
                assert_same_bits(a, b, f"{kind}, notch set {si}, batch {bi}", row_names(kind, pcm=post))
                want = [interval(c, w) for c, w in SETS[si]] + [(0, 0), (0, 0)]
                assert g.notches() == want and h.notches() == [(0, 0)] * 4
    finally:
        A.close()
        for b in Bs:
            b.close()


@pytest.mark.parametrize("n", [360, 248])
def test_batch_split(n):
    """6 frames as one batch, as six batches of one and as 4 + 2: the same bytes for notched clients of every kind"""
    is_real = True
    raw = stream(is_real, 7, 12, tones_for(is_real))
    got = []
    for sizes in ((6,), (1,) * 6, (4, 2)):
        A = Ctx(is_real, n, len(KINDS) + 1, raw)
        try:
            cl = []
            for kind in KINDS:
                g = A.add(kind, window(kind))
                g.set_notch(0, L0 + 80.0, 3.0)
                g.set_notch(1, L0 + 60.0, 2.0)
                cl.append(g)
            rows = {k: [] for k in KINDS}
            for F in sizes:
                A.batch(F)
                for kind, g in zip(KINDS, cl):
                    rows[kind].append(read_client(g, kind, F))
            got.append({k: tuple(np.concatenate([r[i] for r in v]) for i in range(len(v[0]))) for k, v in rows.items()})
        finally:
            A.close()
    for other in got[1:]:
        for kind in KINDS:
            assert_same_bits(got[0][kind], other[kind], f"{kind}: split", row_names(kind))


def test_no_collateral_and_arguments():
    """clients without notches give the same bytes whether or not their neighbours have notches or auto-notch on; every
    rejected psdr_client_set_notch leaves the previous notch in force, by bits"""
    is_real, n = False, 360
    raw = stream(is_real, 7, 13, tones_for(is_real))
    runs = []
    for neighbours in (False, True):
        A = Ctx(is_real, n, 2 * len(KINDS) + 1, raw)
        try:
            plain, noisy = [], []
            for kind in KINDS:
                plain.append(A.add(kind, window(kind)))
                g = A.add(kind, window(kind))
                noisy.append(g)
                if neighbours:
                    g.set_notch(0, L0 + 80.0, 3.0)
                    g.set_auto_notch(True)
            if neighbours:
                lib, hdl, g = A.ctx.lib, A.ctx.h, noisy[0]
                before = g.id
                for args in ((99, 0, 5050.0, 3.0), (-1, 0, 5050.0, 3.0), (before, 2, 5050.0, 3.0), (before, -1, 5050.0, 3.0),
                             (before, 0, float("nan"), 3.0), (before, 0, 5050.0, float("inf")), (before, 0, 5050.0, n + 0.5)):
                    assert lib.psdr_client_set_notch(hdl, *args) == -1, args
                assert lib.psdr_client_set_auto_notch(hdl, 99, 1) == -1
                assert lib.psdr_set_option(hdl, A.ctx.OPT_AUTO_NOTCH, 2) == -1
            spec = A.batch(6)
            ptrs = (C.c_void_p * 5)()
            assert A.ctx.lib.psdr_debug_notch_ptrs(A.ctx.h, ptrs) == 0
            if neighbours:
                assert all(ptrs[k] for k in range(5)), list(ptrs)
            else:
                # a context that never calls the new functions: no table, no sums, no counters, and null pointers to the kernels
                assert not any(ptrs[k] for k in range(5)), list(ptrs)
            runs.append(([read_client(g, k, 6) for g, k in zip(plain, KINDS)], [read_client(g, k, 6) for g, k in zip(noisy, KINDS)]))
            if neighbours:
                assert noisy[0].notches()[0] == interval(L0 + 80.0, 3.0)
                # the rejected calls left that notch in force, by bits: noisy[0] is a plain USB client on the zeroed spectrum
                B = Ctx(is_real, n, 2)
                try:
                    twin = B.add(KINDS[0], window(KINDS[0]))
                    B.batch_from(zeroed(spec, [(L0 + 80.0, 3.0)]))
                    assert_same_bits(runs[-1][1][0], read_client(twin, KINDS[0], 6), "after the rejected calls", row_names(KINDS[0]))
                finally:
                    B.close()
        finally:
            A.close()
    for kind, a, b in zip(KINDS, runs[0][0], runs[1][0]):
        assert_same_bits(a, b, f"{kind}: a plain client beside notched neighbours", row_names(kind))
    assert runs[1][1][0][1].tobytes() != runs[0][1][0][1].tobytes(), "the notch took no power out of the USB window"


@pytest.mark.parametrize("chain", ["1", "0"])
def test_non_finite_values_in_notched_bins_do_not_flag_the_frame(chain, monkeypatch):
    """NaN and Inf planted in notched bins of the spectrum A is handed (psdr_demod_batch_from: the frame-ordered NaN replay of
    USB / LSB runs too): no NaN flag, and every output equal to B's on the zeroed spectrum, over two batches"""
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    is_real, n = True, 360
    assert KINDS[0] == "USB"
    notches = SETS[0]  # [L0 + 79, L0 + 82) and [L0 - 2, L0 + 2)
    raw = stream(is_real, 13, 15, tones_for(is_real))
    T = Ctx(is_real, n, 1, raw)
    A, B = Ctx(is_real, n, len(KINDS) + 1), Ctx(is_real, n, len(KINDS) + 1)
    try:
        ga, gb = [], []
        for kind in KINDS:
            g = A.add(kind, window(kind))
            for idx, (c, w) in enumerate(notches):
                g.set_notch(idx, c, w)
            ga.append(g)
            gb.append(B.add(kind, window(kind)))
        for bi in range(2):
            spec = T.batch(6)
            bad = spec.copy()
            bad[1, L0 + 80] = np.nan
            bad[2, L0 + 1] = complex(np.inf, 1.0)
            bad[3, L0 + 79] = complex(0.0, -np.inf)
            bad[5, L0 - 1] = complex(np.nan, np.inf)  # below the window: notched, never read
            A.batch_from(bad)
            B.batch_from(zeroed(spec, notches))
            for kind, g, h in zip(KINDS, ga, gb):
                a, b = read_client(g, kind, 6), read_client(h, kind, 6)
                assert not a[2].any(), f"{kind}, batch {bi}: a frame was flagged"
                assert np.isfinite(a[1]).all(), f"{kind}, batch {bi}: pwr"
                assert_same_bits(a, b, f"{kind}, batch {bi}", row_names(kind))
    finally:
        for x in (T, A, B):
            x.close()


# ---- the detector -------------------------------------------------------------------------------------------------------
PERIOD = RATE // 360  # 33 frames
K0, K1 = 3000, 8000
KT = K0 + 30


def amp(x):
    """amplitude of a real tone whose bin holds x times the noise's power per bin, for unit noise and no window; a forward
    window takes at most a third of that ratio away (Hann: 0.25 / 0.375) - the margins below hold with and without"""
    return 2.0 * np.sqrt(x / SHAPES[True])


def detector_stream(nhalves):
    N = SHAPES[True]
    rng = np.random.default_rng(14)
    ns = nhalves * (N // 2)
    t = np.arange(ns, dtype=np.float64)
    x = rng.standard_normal(ns)
    # the heterodyne: 35 dB over the noise bin for two periods, then 4 x the noise bin (6 dB over the window's mean)
    strong = t < 2 * PERIOD * (N // 2)
    x += np.where(strong, amp(3000.0), amp(4.0)) * np.cos(2 * np.pi * KT * t / N)
    # three tones for the third client: 6000, 3000, 12000 times the noise bin
    for k, p in ((K1 + 50, 6000.0), (K1 + 120, 3000.0), (K1 + 200, 12000.0)):
        x += amp(p) * np.cos(2 * np.pi * k * t / N)
    return x.astype(np.float32)


def test_detector():
    """Margins (P = the noise's power per bin, window of 90 bins, tone T): mean = (89 P + T) / 90.  T = 3000 P (2000 P behind a
    window): 16 mean = 549 P (372 P), a factor 5 below T.  T = 4 P (2.7 P): 8 mean = 8.3 P (8.2 P), a factor 2 above T.  AM window
    of 80 bins: the tone would pass (16 mean = 616 P) were it not within 3 bins of floor(audio_mid).  Three tones in 300 bins:
    mean = 71 P (48 P), 16 mean = 1136 P (768 P), the weakest tone 3000 P (2000 P) a factor 2.6 above, the tones a factor 2 apart."""
    n = 360
    total = 3 * PERIOD + 1
    raw = detector_stream(total + 1)
    A = Ctx(True, n, 8, raw)
    try:
        from phantomsdr_amd import AudioClient
        usb = A.add("USB", (K0, float(K0), K0 + 90))
        late = A.add("USB", (K0, float(K0), K0 + 90))      # sits out one batch of 6: its evaluations come 6 frames later
        am = A.add("AM", (KT - 42, KT - 2 + 0.25, KT + 38))  # the tone at floor(audio_mid) + 2
        tri = A.add("USB", (K1, float(K1), K1 + 300))
        plain = A.add("USB", (K0, float(K0), K0 + 90))
        again = A.add("USB", (K0, float(K0), K0 + 90))     # switched off and on again while it sits out: starts from zero
        for g in (usb, late, again, am, tri):
            g.set_auto_notch(True)
        want = (KT - 1, KT + 2)
        done = 0
        pwr_before = pwr_after = None

        def run(F):
            nonlocal done
            A.batch(F)
            done += F

        run(6)
        late.set_paused(True)
        again.set_paused(True)
        again.set_auto_notch(False)
        again.set_auto_notch(True)
        run(6)
        late.set_paused(False)
        again.set_paused(False)
        while done < PERIOD - 1 - 5:
            run(6)
        run(PERIOD - 1 - done)
        assert done == PERIOD - 1
        for g in (usb, late, am, tri):
            assert g.notches() == [(0, 0)] * 4, "an entry one frame early"
        pwr_before = usb.read_audio(A.ctx.last_demod_frames)[1][-1]
        run(1)  # frame `period`
        assert usb.notches()[2:] == [want, (0, 0)]
        assert late.notches()[2:] == [(0, 0), (0, 0)], "the paused client's counter moved"
        assert am.notches()[2:] == [(0, 0), (0, 0)], "the wanted carrier's neighbourhood was notched"
        assert tri.notches()[2:] == [(K1 + 199, K1 + 202), (K1 + 49, K1 + 52)]
        run(6)  # the first batch with the notch in force; `late` evaluates at its own 33rd frame, the batch's last
        assert late.notches()[2:] == [want, (0, 0)]
        assert again.notches()[2:] == [(0, 0), (0, 0)]
        a_usb, p_usb, _ = usb.read_audio(6)
        a_pl, p_pl, _ = plain.read_audio(6)
        pwr_after = p_usb[-1]
        assert pwr_after * 5 < pwr_before and p_usb[-1] * 5 < p_pl[-1], (pwr_before, pwr_after, p_pl[-1])
        # the tone's audio line (bin KT - K0 of the window = audio bin 30 of 180) is down at the noise level
        line = lambda a: np.abs(np.fft.rfft(a[-1].astype(np.float64) * np.hanning(a.shape[1])))
        sp_u, sp_p = line(a_usb), line(a_pl)
        kk = int(np.argmax(sp_p))
        assert sp_p[kk] > 8 * np.median(sp_p) and sp_u[kk] < 4 * np.median(sp_u), (sp_p[kk], sp_u[kk], np.median(sp_u))
        # a retune resets the state of `tri`: its entries go with the next batch
        tri.set_audio_range(K1 + 1, float(K1 + 1), K1 + 300)
        run(6)  # `again` started from zero at frame 12: its 33rd frame is this batch's last
        assert done == 12 + PERIOD and again.notches()[2:] == [want, (0, 0)]
        while done < 2 * PERIOD - 6:
            run(6)
        assert tri.notches()[2:] == [(0, 0), (0, 0)]
        run(2 * PERIOD - done)
        assert usb.notches()[2:] == [want, (0, 0)], "the entry did not survive while the tone lasts"
        while done < 3 * PERIOD - 6:
            run(6)
        run(3 * PERIOD - 1 - done)
        assert usb.notches()[2:] == [want, (0, 0)]
        run(1)
        assert usb.notches()[2:] == [(0, 0), (0, 0)], "the entry outlived the tone"
    finally:
        A.close()

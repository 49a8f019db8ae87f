"""PSDR_SAM on the GPU (include/psdr.h: psdr_read_carrier): synchronous AM, the AM baseband detected against the recovered
carrier, against a float64 evaluation of the definition in psdr.h on the ORACLE's spectra.

Shapes: the smallest transforms (2^12-point IQ, 2^13-point real: R = 4096 either way), s16 input, 25 frames as batches of
19 + 1 + 5 (few clients: the chain kernel's K falls to 4, so chains with a warm-up frame, a one-frame batch and a ragged
last chain all occur), audio_rate 12000.  n = 360 / 720: k_demod_chain_sam (PSDR_DEMOD_CHAIN=0: k_demod_idft_fixed +
k_demod_ola_sam), 256: k_demod_idft_wave + k_demod_ola_sam, 1024: k_demod_idft + k_demod_ola_sam.

Signal (its own: helpers.synth_stream modulates its AM carrier at 41 Hz, inside the +-500 Hz carrier low-pass): noise of
sigma 2^-9 and one AM carrier of amplitude 8 / sqrt(N), a 1 kHz tone at modulation index 1.5, 0.37 bin above bin KC.

Bound of the audio, derived: AM's bound (test_gpu_parity.py, test_gpu_iq_mode.py) holds for B - max |dB| <= 2e-4 max |B| -
and the detector adds |B| |dC| / |C| to first order, with the same relative error in C: per frame
    max |d| <= 2e-4 * max |B| * (1 + max |B| / min |C|),
the factor taken from the truth.  The signal keeps it small: every frame after the first has min |C| >= 0.5 max |C| and
max |B| / min |C| <= 4 in the truth (asserted before anything is compared)."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import check_fm, pwr_tolerance, quantize_raw, rel_l2
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NF = 25
BATCHES = (19, 1, 5)
MAXB = 19
LEVELS = 3  # R = 4096, waterfall_size 1024
SHAPES = {0: 1 << 12, 1: 1 << 13}  # is_real -> N
RATE = 12000
KC = 1200  # the carrier sits 0.37 bin above this (even) bin, in client coordinates
OFFSET_BINS = 0.37
INVALID, NO_DATA, UNSUPPORTED = -1, -7, -6


def cutoff(n):
    return 500 * n // RATE


def windows(n):
    """on the carrier with floor(audio_mid) even and odd, +-(h - 2) bins; and one that starts above
    floor(mid) + cutoff + 1: no kept bin, C = 0 exactly"""
    w = n // 2 - 2
    free_l = KC + cutoff(n) + 2
    return [(KC - w, float(KC), KC + w), (KC + 1 - w, KC + 1.5, KC + 1 + w), (free_l, float(KC), min(free_l + n // 4, KC + n // 2 - 1))]


@functools.lru_cache(maxsize=None)
def stream(is_real, n):
    N = SHAPES[is_real]
    ns = (NF + 1) * (N // 2)
    rng = np.random.default_rng(170 + is_real)
    t = np.arange(ns, dtype=np.float64)
    amp = 8.0 / np.sqrt(N)
    env = 1.0 + 1.5 * np.cos(2 * np.pi * (n / 12.0) / N * t)  # 1 kHz at the audio rate: n / 12 bins
    if is_real:
        x = rng.standard_normal(ns) * 2.0 ** -9 + amp * env * np.cos(2 * np.pi * (KC + OFFSET_BINS) / N * t)
    else:
        fc = ((KC + OFFSET_BINS + N // 2 + 1) % N) / N  # client bin c is frequency index (c + N/2 + 1) mod N
        x = (rng.standard_normal(ns) + 1j * rng.standard_normal(ns)) * 2.0 ** -9 + amp * env * np.exp(2j * np.pi * fc * t)
    raw = quantize_raw(x, "s16", bool(is_real))
    conv = O.convert(raw, "s16")
    halves = (conv if is_real else conv.view(np.complex64)).reshape(NF + 1, N // 2)
    return raw, halves


@functools.lru_cache(maxsize=None)
def oracle_spectra(is_real, n):
    """the reference's spectra of the 25 frames (wrap copy of n bins), computed once per shape and left alone"""
    N = SHAPES[is_real]
    _, halves = stream(is_real, n)
    fo = O.FFT(N, bool(is_real), LEVELS, 0, n)
    out = []
    for f in range(NF):
        fo.load(halves[f], halves[f + 1])
        fo.execute()
        s = fo.output().copy()
        s.setflags(write=False)
        out.append(s)
    return fo, out


def flip_sign(frame, m_floor, is_real):
    return -1.0 if frame % 2 == 1 and ((m_floor % 2 == 0 and not is_real) or (m_floor % 2 == 1 and is_real)) else 1.0


def truth(is_real, n, win, sam_starts=(0,)):
    """float64, as psdr.h defines the mode, on the oracle's spectra of the 25 frames of one window (truth_of)"""
    fo, specs = oracle_spectra(is_real, n)
    return truth_of(specs, lambda s, l, ln: s[fo.slice_ptr_index(l):fo.slice_ptr_index(l) + ln], is_real, n, win, sam_starts)


def spectrum_rms(s):
    return float(np.sqrt(np.mean(np.abs(s[:4096].astype(np.complex128)) ** 2)))


def truth_of(specs, slice_of, is_real, n, win, sam_starts=(0,), rms_of=spectrum_rms):
    """float64, as psdr.h defines the mode: placement, np.fft.ifft * n, mask, flip, overlap-add, detector, carrier record -
    over the frames of one window.  specs: one spectrum per frame; slice_of(spectrum, l, ln): its bins [l, l + ln) in client
    order; rms_of(spectrum): the rms of its R bins.  sam_starts: the frames at which the carrier tail starts from zero.
    -> dict of B, C [frames][h] complex128, audio [frames][h], level, offset_hz, pwr, fwd_scale [frames]"""
    NF = len(specs)
    l, mid, r = win
    h, m_floor = n // 2, int(np.floor(mid))
    m, ln, cut = m_floor - l, r - l, cutoff(n)
    B, Cc = np.zeros((NF, h), np.complex128), np.zeros((NF, h), np.complex128)
    pw, fs = np.zeros(NF), np.zeros(NF)
    bt, ct = np.zeros(h, np.complex128), np.zeros(h, np.complex128)
    for f in range(NF):
        S = slice_of(specs[f], l, ln).astype(np.complex128)
        X = np.zeros(n, np.complex128)
        for t in range(ln):
            d = t - m
            if 0 <= d < h:
                X[d] = S[t]
            elif -(h - 1) <= d < 0:
                X[n + d] = S[t]
        Xc = X.copy()
        if 2 * cut < n:
            Xc[cut:n - cut] = 0
        y, c = np.fft.ifft(X) * n, np.fft.ifft(Xc) * n
        s = flip_sign(f, m_floor, is_real)
        if f in sam_starts:
            ct = np.zeros(h, np.complex128)
        B[f], bt = s * y[:h] + bt, s * y[h:]
        Cc[f], ct = s * c[:h] + ct, s * c[h:]
        pw[f] = float((np.abs(S) ** 2).sum())
        fs[f] = rms_of(specs[f]) * np.sqrt(max(ln, 1))
    mag = np.abs(Cc)
    with np.errstate(divide="ignore", invalid="ignore"):
        audio = np.where(mag == 0, B.real, (B.real * Cc.real + B.imag * Cc.imag) / mag)
    lag = (Cc[:, 1:] * np.conj(Cc[:, :-1])).sum(axis=1)
    return dict(B=B, C=Cc, audio=audio, level=mag.mean(axis=1), offset_hz=RATE / (2 * np.pi) * np.angle(lag), pwr=pw, fwd_scale=fs)


def assert_signal_condition(T, tag):
    """the condition the derived bound stands on: a statement about the signal, checked on the truth"""
    for f in range(1, len(T["C"])):
        cmin, cmax, bmax = np.abs(T["C"][f]).min(), np.abs(T["C"][f]).max(), np.abs(T["B"][f]).max()
        assert cmin >= 0.5 * cmax and bmax / cmin <= 4.0, (tag, f, cmin / cmax, bmax / cmin)


@functools.lru_cache(maxsize=None)
def truths(is_real, n):
    res = [truth(is_real, n, w) for w in windows(n)[:2]]
    for T in res:
        assert_signal_condition(T, (is_real, n))
    return res


def audio_bound(T, f):
    bmax, cmin = np.abs(T["B"][f]).max(), np.abs(T["C"][f]).min()
    return 2e-4 * bmax * (1.0 + (bmax / cmin if cmin > 0 else np.inf))


class Rig:
    """one context on the shared stream; batch(F) transforms and demodulates the next F frames"""

    def __init__(self, is_real, n, max_clients=4, post=False, pcm16=False):
        from phantomsdr_amd import Context
        self.N, self.is_real, self.n, self.h = SHAPES[is_real], is_real, n, n // 2
        raw, _ = stream(is_real, n)
        self.ctx = Context(self.N, is_real, LEVELS, additional_size=n, audio_fft_size=n, audio_rate=RATE, input_format="s16",
                           max_batch=MAXB, max_clients=max_clients)
        self.d = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.d, raw)
        if post:
            if pcm16:
                self.ctx.set_option(self.ctx.OPT_POST_CHAIN_PCM16, 1)
            self.ctx.set_post_chain(True)
        self.frame = 0

    def add(self, mode, win):
        from phantomsdr_amd import AudioClient
        g = AudioClient(self.ctx)
        g.set_audio_demodulation(mode)
        g.set_audio_range(*win)
        return g

    def batch(self, F, via="demod"):
        ctx = self.ctx
        ctx.process_batch(self.d, F, offset_bytes=self.frame * ctx.half_frame_bytes())
        if via == "from":  # psdr_demod_batch_from on the context's own spectrum
            from phantomsdr_amd._lib import check
            p, nb = C.c_void_p(), C.c_size_t()
            check(ctx.lib.psdr_spectrum_device_ptr(ctx.h, 0, C.byref(p), C.byref(nb)))
            stride = self.N // 2 + 2 if self.is_real else self.N
            check(ctx.lib.psdr_demod_batch_from(ctx.h, p, stride, F, self.frame))
            ctx.last_demod_frames = F
        else:
            ctx.demod_batch(self.frame)
        self.frame += F

    def close(self):
        self.ctx.dev_free(self.d)
        self.ctx.close()


def run_sam(is_real, n, batches=BATCHES, via="demod", read="read", wins=None, mode="SAM"):
    """the windows as SAM clients over the 25 frames: per client (audio[25][h], pwr[25], nan[25], level[25], offset_hz[25])"""
    wins = windows(n) if wins is None else wins
    rig = Rig(is_real, n)
    try:
        cl = [rig.add(mode, w) for w in wins]
        got = [[] for _ in cl]
        for F in batches:
            rig.batch(F, via)
            if read == "fetch_batch":
                rig.ctx.fetch_batch()
            elif read == "fetch":
                rig.ctx.fetch_begin(rig.ctx.FETCH_AUDIO)
                rig.ctx.fetch_end()
            for k, g in enumerate(cl):
                if read == "read":
                    a, p, nan = (x[:F] for x in g.read_audio(MAXB))
                    lv, off = g.read_carrier(MAXB) if mode == "SAM" else (np.zeros(F, np.float32),) * 2
                else:
                    rows = [rig.ctx.fetched_audio(g.id, f) for f in range(F)]
                    a, p, nan = np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.float32), np.array([r[2] for r in rows], np.int32)
                    car = [rig.ctx.fetched_carrier(g.id, f) for f in range(F)]
                    lv, off = np.array([c[0] for c in car], np.float32), np.array([c[1] for c in car], np.float32)
                got[k].append((a, p, nan, lv[:F], off[:F]))
        return [tuple(np.concatenate([b[i] for b in per]) for i in range(5)) for per in got]
    finally:
        rig.close()


def same_bits(a, b, tag):
    for x, y, what in zip(a, b, ("audio", "pwr", "nan flags", "carrier level", "carrier offset")):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{tag}: {what} differ"


# ---- 1. parity with the truth ----------------------------------------------------------------------------------------

PATHS = [(360, "1"), (360, "0"), (720, "1"), (720, "0"), (256, "1"), (1024, "1")]  # (n, PSDR_DEMOD_CHAIN)


@pytest.mark.parametrize("via", ["demod", "from"])
@pytest.mark.parametrize("is_real", [0, 1])
@pytest.mark.parametrize("n,chain", PATHS, ids=[f"{n}-chain{c}" for n, c in PATHS])
def test_audio_equals_the_truth(n, chain, is_real, via, monkeypatch):
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    tr = truths(is_real, n)
    got = run_sam(is_real, n, via=via, wins=windows(n)[:2])
    for k, ((audio, pwr, nan, _, _), T) in enumerate(zip(got, tr)):
        assert audio.shape == (NF, n // 2) and audio.dtype == np.float32
        assert not nan.any()
        for f in range(NF):
            tag = f"n {n} chain {chain} real {is_real} window {k} frame {f}"
            d, bound = float(np.abs(audio[f] - T["audio"][f]).max()), audio_bound(T, f)
            print(f"{tag}: max |d| {d:.3e}, bound {bound:.3e}, rel L2 {rel_l2(audio[f], T['audio'][f]):.2e}")
            assert d <= bound, tag
            assert abs(pwr[f] - T["pwr"][f]) <= pwr_tolerance(T["pwr"][f], T["fwd_scale"][f]), tag


# ---- 2. it is synchronous (from the GPU's audio alone) ---------------------------------------------------------------

def harmonic_ratio(stream_):
    """|second harmonic| / |fundamental| of the 1 kHz tone in frames 1..24, Hann-windowed"""
    L = stream_.size
    sp = np.abs(np.fft.rfft(stream_.astype(np.float64) * np.hanning(L)))
    k = L // 12  # 1 kHz at 12 kHz
    return sp[2 * k - 2:2 * k + 3].max() / sp[k - 2:k + 3].max()


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_second_harmonic_is_gone_and_the_audio_goes_negative(n, is_real):
    w = windows(n)[:1]
    sam = run_sam(is_real, n, wins=w)[0][0]
    am = run_sam(is_real, n, wins=w, mode="AM")[0][0]
    r_sam, r_am = harmonic_ratio(sam[1:].reshape(-1)), harmonic_ratio(am[1:].reshape(-1))
    print(f"n {n} real {is_real}: second harmonic / fundamental SAM {r_sam:.3e}, AM {r_am:.3e}")
    assert r_sam <= r_am / 100.0
    assert sam[1:].min() < 0 <= am.min()


# ---- 3. bit identities -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,chain,is_real", [(360, "1", 0), (720, "1", 1), (360, "0", 1), (256, "1", 0), (1024, "1", 1)])
def test_window_without_a_carrier_bin_gives_the_iq_rows_real_parts(n, chain, is_real, monkeypatch):
    """no kept bin: C = 0 exactly, the phase reference is 1, audio = B.re - and B is the PSDR_IQ row, bit for bit"""
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    w = windows(n)[2]
    assert w[0] > int(w[1]) + cutoff(n) + 1 and w[2] > w[0]
    rig = Rig(is_real, n)
    try:
        s, q = rig.add("SAM", w), rig.add("IQ", w)
        for F in BATCHES:
            rig.batch(F)
            a, _, nan = s.read_audio(MAXB)
            iq, _, _ = q.read_iq(MAXB)
            lv, off = s.read_carrier(MAXB)
            assert not nan.any() and np.abs(a).max() > 0
            assert a.tobytes() == np.ascontiguousarray(iq.real).tobytes()
            assert not lv.any() and not off.any()
    finally:
        rig.close()


def test_audio_size_with_cutoff_zero_gives_the_iq_rows_real_parts():
    n = 20
    assert cutoff(n) == 0
    w = (KC - 8, float(KC), KC + 8)
    rig = Rig(0, n)
    try:
        s, q = rig.add("SAM", w), rig.add("IQ", w)
        for F in BATCHES:
            rig.batch(F)
            a, iq = s.read_audio(MAXB)[0], q.read_iq(MAXB)[0]
            assert np.abs(a).max() > 0 and a.tobytes() == np.ascontiguousarray(iq.real).tobytes()
    finally:
        rig.close()


@pytest.mark.parametrize("n,chain,is_real", [(360, "1", 0), (720, "1", 1), (360, "0", 1), (256, "1", 1), (1024, "1", 0)])
def test_batch_splits_give_the_same_bits(n, chain, is_real, monkeypatch):
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    a = run_sam(is_real, n)
    for split in ((5, 19, 1), (1,) * NF):
        b = run_sam(is_real, n, batches=split)
        for k in range(3):
            same_bits(a[k], b[k], f"client {k}: 19 + 1 + 5 against {split[:3]}...")


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_every_way_to_read_gives_the_same_rows(n, is_real):
    a = run_sam(is_real, n)
    b = run_sam(is_real, n, read="fetch_batch")
    c = run_sam(is_real, n, read="fetch")
    for k in range(3):
        same_bits(a[k], b[k], f"client {k}: psdr_read_audio / _carrier against psdr_fetch_batch")
        same_bits(a[k], c[k], f"client {k}: psdr_read_audio / _carrier against psdr_fetch_begin / _end")


# ---- 4. state --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1), (720, 1)])
def test_mode_switches_continue_through_sam(n, is_real):
    """AM 5 frames -> SAM 6 -> FM 4 -> SAM 5 -> USB 5: AM, FM and USB match the oracle as if the client had been in that mode
    all along (the oracle runs AM in place of SAM: the same state), each SAM batch the truth started from a zero carrier tail"""
    seq = [("AM", 5), ("SAM", 6), ("FM", 4), ("SAM", 5), ("USB", 5)]
    h = n // 2
    fo, specs = oracle_spectra(is_real, n)
    wins = windows(n)[:2]
    tr = [truth(is_real, n, w, sam_starts=(5, 15)) for w in wins]
    rig = Rig(is_real, n)
    try:
        gs = [rig.add("AM", w) for w in wins]
        os_ = []
        for w in wins:
            o = O.AudioClient(bool(is_real), n, RATE, 4096)
            o.set_audio_range(*w)
            os_.append(o)
        frame = 0
        for mode, F in seq:
            for g, o in zip(gs, os_):
                g.set_audio_demodulation(mode)
                o.set_audio_demodulation("AM" if mode == "SAM" else mode)
            rig.batch(F)
            for k, (g, o) in enumerate(zip(gs, os_)):
                out, pwr, nan = g.read_audio(MAXB)
                assert len(out) == F and not nan.any()
                for f in range(F):
                    tag = f"n {n} real {is_real} client {k} {mode} frame {frame + f}"
                    a_o, p_o, _, dropped = o.send_audio(specs[frame + f], frame + f, fft=fo)
                    assert not dropped
                    assert abs(pwr[f] - p_o) <= pwr_tolerance(p_o, o.fwd_scale), tag
                    if mode == "SAM":
                        T = tr[k]
                        assert np.abs(out[f] - T["audio"][frame + f]).max() <= audio_bound(T, frame + f), tag
                    elif mode == "FM":
                        check_fm(out[f], a_o, o.baseband()[:h], o.bb_prev, tag, fwd_scale=max(o.fwd_scale, o.fwd_scale_prev))
                    else:
                        scale = max(np.abs(a_o).max(), 1e-30)
                        assert rel_l2(out[f], a_o) < 1e-4, f"{tag}: rel L2 {rel_l2(out[f], a_o):.2e}"
                        assert np.abs(out[f] - a_o).max() <= 2e-4 * scale, tag
                if mode == "SAM":
                    lv = g.read_carrier(MAXB)[0]
                    T = tr[k]
                    assert np.abs(lv - T["level"][frame:frame + F]).max() <= 2e-4 * T["level"][frame:frame + F].max()
                else:
                    from phantomsdr_amd import PsdrError
                    with pytest.raises(PsdrError) as e:
                        g.read_carrier(MAXB)
                    assert e.value.code == NO_DATA
            frame += F
    finally:
        rig.close()


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_paused_sam_client_keeps_its_state(n, is_real):
    """paused over the one-frame batch (frame 19): frames 20..24 continue from frame 18's tails, bit for bit as in a run of
    one-frame batches paused over the same frame"""
    from phantomsdr_amd import PsdrError

    def run(batches):
        rig = Rig(is_real, n)
        try:
            g, other = rig.add("SAM", windows(n)[0]), rig.add("SAM", windows(n)[1])
            out = []
            for F in batches:
                paused = rig.frame == 19
                g.set_paused(paused)
                rig.batch(F)
                if paused:
                    for call in (g.read_audio, g.read_carrier):
                        with pytest.raises(PsdrError) as e:
                            call(MAXB)
                        assert e.value.code == NO_DATA
                    other.read_carrier(MAXB)
                else:
                    out.append(g.read_audio(MAXB) + g.read_carrier(MAXB))
            return tuple(np.concatenate([o[i] for o in out]) for i in range(5))
        finally:
            rig.close()

    a, b = run(BATCHES), run((1,) * NF)
    assert a[0].shape == (NF - 1, n // 2)
    same_bits(a, b, "paused over frame 19")
    never = run_sam(is_real, n, wins=windows(n)[:1])[0]
    assert a[0][:19].tobytes() == never[0][:19].tobytes() and a[0][19].tobytes() != never[0][20].tobytes()


def run_old_modes(is_real, n, with_sam):
    """19 + 1 + 5 frames with the post chain on: three old-mode clients, per client and batch (audio, pwr, nan, pcm); with_sam:
    a SAM client in the slot between them"""
    rig = Rig(is_real, n, max_clients=6, post=True)
    try:
        w = windows(n)
        old = [rig.add("USB", w[0]), rig.add("AM", w[1])]
        if with_sam:
            sam = rig.add("SAM", w[0])
            assert sam.id == 2
        old.append(rig.add("FM", w[0]))
        res = [[] for _ in old]
        for F in BATCHES:
            rig.batch(F)
            for k, g in enumerate(old):
                res[k].append(g.read_audio(MAXB) + (g.read_pcm(MAXB),))
            if with_sam:
                assert np.abs(sam.read_audio(MAXB)[0]).max() > 0
        return res
    finally:
        rig.close()


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_other_clients_do_not_notice_a_sam_client(n, is_real):
    a, b = run_old_modes(is_real, n, False), run_old_modes(is_real, n, True)
    for k, (ra, rb) in enumerate(zip(a, b)):
        for bi, (x, y) in enumerate(zip(ra, rb)):
            for u, v, what in zip(x, y, ("audio", "pwr", "nan flags", "pcm")):
                assert u.shape == v.shape and u.tobytes() == v.tobytes(), f"client {k} batch {bi}: {what} differ with a SAM client beside it"


# ---- 5. post chain ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,is_real,pcm16", [(360, 0, False), (360, 0, True), (256, 1, False)])
def test_post_chain_of_a_sam_client_is_bit_exact(n, is_real, pcm16):
    """the oracle's DC blocker + AGC + int16 conversion fed the GPU's own SAM float rows: the PCM must be identical"""
    rig = Rig(is_real, n, post=True, pcm16=pcm16)
    try:
        gs = [rig.add("SAM", w) for w in windows(n)[:2]]
        chains = [O.PostChain(RATE) for _ in gs]
        total = 0
        for F in BATCHES:
            rig.batch(F)
            if pcm16:
                rig.ctx.fetch_begin(rig.ctx.FETCH_PCM)
                rig.ctx.fetch_end()
            for g, ch in zip(gs, chains):
                audio, _, nan = g.read_audio(MAXB)
                pcm = g.read_pcm(MAXB)
                assert not nan.any()
                for f in range(F):
                    want = ch.process(audio[f])
                    assert np.array_equal(pcm[f], want), f"frame {f}: {np.count_nonzero(pcm[f] != want)} samples differ"
                    if pcm16:
                        row = rig.ctx.fetched_pcm16(g.id, f)
                        assert row.dtype == np.int16 and np.array_equal(row.astype(np.int32), want)
                    total += int(np.count_nonzero(want))
        assert total > 1000, "the AGC never opened: the test did not exercise the chain"
    finally:
        rig.close()


# ---- 6. carrier record -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("is_real", [0, 1])
@pytest.mark.parametrize("n,chain", PATHS, ids=[f"{n}-chain{c}" for n, c in PATHS])
def test_carrier_record(n, chain, is_real, monkeypatch):
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    tr = truths(is_real, n)
    got = run_sam(is_real, n, wins=windows(n)[:2])
    binw = RATE / n
    for k, ((_, _, _, lv, off), T, w) in enumerate(zip(got, tr, windows(n)[:2])):
        want_bins = KC + OFFSET_BINS - int(np.floor(w[1]))  # above the centre of bin floor(audio_mid)
        for f in range(1, NF):
            tag = f"n {n} chain {chain} real {is_real} window {k} frame {f}"
            cm = np.abs(T["C"][f])
            print(f"{tag}: offset {off[f]:.3f} Hz (truth {T['offset_hz'][f]:.3f}, synthesised {want_bins * binw:.3f}), level {lv[f]:.6e} (truth {T['level'][f]:.6e})")
            assert abs(off[f] - want_bins * binw) <= 0.1 * binw, tag
            assert abs(off[f] - T["offset_hz"][f]) <= RATE / (2 * np.pi) * 4 * 2e-4 * (cm.max() / cm.min()) ** 2, tag
            assert abs(lv[f] - T["level"][f]) <= 2e-4 * T["level"][f], tag


# ---- 7. errors -------------------------------------------------------------------------------------------------------

def test_errors():
    from phantomsdr_amd import Group, PsdrError
    n = 360
    rig = Rig(0, n)
    try:
        am, sam = rig.add("AM", windows(n)[0]), rig.add("SAM", windows(n)[1])
        assert rig.ctx.lib.psdr_client_set_audio_demodulation(rig.ctx.h, am.id, 6) == INVALID
        assert rig.ctx.lib.psdr_client_set_audio_demodulation(rig.ctx.h, am.id, -1) == INVALID
        rig.batch(5)
        rig.ctx.fetch_batch()
        for call in (lambda: am.read_carrier(MAXB), lambda: rig.ctx.fetched_carrier(am.id, 0)):
            with pytest.raises(PsdrError) as e:
                call()
            assert e.value.code == NO_DATA
        lv, off = sam.read_carrier(MAXB)
        assert len(lv) == 5 and rig.ctx.fetched_carrier(sam.id, 4) == (float(lv[4]), float(off[4]))
        with pytest.raises(PsdrError) as e:
            rig.ctx.fetched_carrier(sam.id, 5)
        assert e.value.code == INVALID
    finally:
        rig.close()
    g = Group([0], "clients", 1 << 12, False, LEVELS, audio_fft_size=360, additional_size=360, max_clients=4)
    try:
        with pytest.raises(PsdrError) as e:
            g.client_add(100, 130.0, 160, "SAM")
        assert e.value.code == UNSUPPORTED
        gid = g.client_add(100, 130.0, 160, "AM")
        assert g.lib.psdr_group_client_set_audio_demodulation(g.h, gid, 5) == UNSUPPORTED
        assert g.lib.psdr_group_client_set_audio_demodulation(g.h, gid, 3) == 0
    finally:
        g.close()

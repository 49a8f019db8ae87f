"""Selectable-sideband synchronous AM on the GPU (include/psdr.h: psdr_client_set_sam_sideband): a PSDR_SAM client that detects
only the upper or only the lower sideband against the carrier recovered from the whole window - bit relations to PSDR_SAM
and PSDR_IQ clients, and a float64 evaluation of the definition in psdr.h on the ORACLE's spectra.

Rig, shapes and batches are test_gpu_sam_mode.py's: 2^12-point IQ and 2^13-point real (R = 4096 either way), s16 input, 25
frames as batches of 19 + 1 + 5, audio_rate 12000.  n = 360 / 720: k_demod_chain_sbsam (PSDR_DEMOD_CHAIN=0: k_demod_idft_fixed +
k_demod_ola_sbsam), 256: k_demod_idft_wave + k_demod_ola_sbsam, 1024: k_demod_idft + k_demod_ola_sbsam.

Signal: that test's (noise of sigma 2^-9, an AM carrier of amplitude 8 / sqrt(N) 0.37 bin above bin KC, a 1 kHz tone at
modulation index 1.5) plus an UNMODULATED interferer of a quarter of the carrier's amplitude 700 Hz (0.7 n / 12 bins) BELOW
the carrier: in the lower sideband, outside the +-500 Hz carrier low-pass.

Bound of the audio, derived: PSDR_SAM's (test_gpu_sam_mode.py) times the definition's exact factor 2 - per frame
    max |d| <= 2 * 2e-4 * max |B'| * (1 + max |B'| / min |C|),
the ratio taken from the truth; its precondition (every frame after the first has min |C| >= 0.5 max |C| and
max |B'| / min |C| <= 4) is asserted on the truth before anything is compared.

A second audio_rate, 500 n + 1, makes the carrier cutoff 500 n / audio_rate = 0: every carrier bin is zeroed, C = 0 exactly,
and the audio is 2 B'.re - B' itself becomes visible, bit for bit, on every path and through every change of state."""
import functools

import numpy as np
import pytest

from helpers import pwr_tolerance, quantize_raw
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
INVALID, NO_DATA = -1, -7
BOTH, UPPER, LOWER = "both", "upper", "lower"
PATHS = [(360, "1"), (360, "0"), (720, "1"), (720, "0"), (256, "1"), (1024, "1")]  # (n, PSDR_DEMOD_CHAIN)
PATH_IDS = [f"{n}-chain{c}" for n, c in PATHS]


def cutoff(n, rate=RATE):
    return 500 * n // rate


def zero_cutoff_rate(n):
    return 500 * n + 1


def windows(n):
    """test_gpu_sam_mode.py's: on the carrier with floor(audio_mid) even and odd, +-(h - 2) bins; and one that starts above
    floor(mid) + cutoff + 1: no kept bin, C = 0 exactly"""
    w = n // 2 - 2
    free_l = KC + cutoff(n) + 2
    return [(KC - w, float(KC), KC + w), (KC + 1 - w, KC + 1.5, KC + 1 + w), (free_l, float(KC), min(free_l + n // 4, KC + n // 2 - 1))]


def clipped(win, side):
    """the window clipped to the sideband, psdr.h's rule (tuned USB / LSB's)"""
    l, mid, r = win
    m = int(np.floor(mid))
    if side == UPPER:
        return (min(max(l, m), r), mid, r)
    if side == LOWER:
        return (l, mid, max(m + 1, l) if m < r else r)
    return win


@functools.lru_cache(maxsize=None)
def stream(is_real, n, nf=NF):
    """(raw s16 samples, converted half-frames [nf + 1][N / 2]) of nf frames"""
    N = SHAPES[is_real]
    ns = (nf + 1) * (N // 2)
    rng = np.random.default_rng(170 + is_real)
    t = np.arange(ns, dtype=np.float64)
    amp = 8.0 / np.sqrt(N)
    env = 1.0 + 1.5 * np.cos(2 * np.pi * (n / 12.0) / N * t)  # 1 kHz at the audio rate: n / 12 bins
    car, itf = KC + OFFSET_BINS, KC + OFFSET_BINS - 0.7 * n / 12.0  # the interferer: 700 Hz below the carrier
    if is_real:
        x = rng.standard_normal(ns) * 2.0 ** -9 + amp * env * np.cos(2 * np.pi * car / N * t) + 0.25 * amp * np.cos(2 * np.pi * itf / N * t)
    else:
        fc, fi = ((car + N // 2 + 1) % N) / N, ((itf + N // 2 + 1) % N) / N  # client bin c is frequency index (c + N/2 + 1) mod N
        x = ((rng.standard_normal(ns) + 1j * rng.standard_normal(ns)) * 2.0 ** -9 + amp * env * np.exp(2j * np.pi * fc * t)
             + 0.25 * amp * np.exp(2j * np.pi * fi * t))
    raw = quantize_raw(x, "s16", bool(is_real))
    conv = O.convert(raw, "s16")
    halves = (conv if is_real else conv.view(np.complex64)).reshape(nf + 1, N // 2)
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


@functools.lru_cache(maxsize=None)
def truth(is_real, n, win, side):
    """truth_of on the oracle's spectra of the 25 frames"""
    fo, specs = oracle_spectra(is_real, n)
    return truth_of(specs, lambda s, l, ln: s[fo.slice_ptr_index(l):fo.slice_ptr_index(l) + ln], is_real, n, win, side)


def spectrum_rms(s):
    return float(np.sqrt(np.mean(np.abs(s[:4096].astype(np.complex128)) ** 2)))


def truth_of(specs, slice_of, is_real, n, win, side, rms_of=spectrum_rms):
    """float64, as psdr.h defines it: the carrier from the whole window, B' from the window clipped to `side` (BOTH: PSDR_SAM
    itself, without the doubling), np.fft.ifft * n, flip, overlap-add from zero tails, detector.  specs: one spectrum per
    frame; slice_of(spectrum, l, ln): its bins [l, l + ln) in client order; rms_of(spectrum): the rms of its R bins.
    -> dict of B, C [frames][h] complex128, audio [frames][h], pwr, fwd_scale [frames]"""
    NF = len(specs)
    l, mid, r = win
    h, m_floor = n // 2, int(np.floor(mid))
    m, ln, cut = m_floor - l, r - l, cutoff(n)
    cl, _, cr = clipped(win, side)
    B, Cc = np.zeros((NF, h), np.complex128), np.zeros((NF, h), np.complex128)
    pw, fs = np.zeros(NF), np.zeros(NF)
    bt, ct = np.zeros(h, np.complex128), np.zeros(h, np.complex128)
    for f in range(NF):
        S = slice_of(specs[f], l, ln).astype(np.complex128)
        X, Xb = np.zeros(n, np.complex128), np.zeros(n, np.complex128)
        for t in range(ln):
            d = t - m
            if -(h - 1) <= d < h:
                X[d % n] = S[t]
                if cl <= l + t < cr:
                    Xb[d % n] = S[t]
        Xc = X.copy()
        if 2 * cut < n:
            Xc[cut:n - cut] = 0
        y, c = np.fft.ifft(Xb) * n, np.fft.ifft(Xc) * n
        s = flip_sign(f, m_floor, is_real)
        B[f], bt = s * y[:h] + bt, s * y[h:]
        Cc[f], ct = s * c[:h] + ct, s * c[h:]
        pw[f] = float((np.abs(S) ** 2).sum())
        fs[f] = rms_of(specs[f]) * np.sqrt(max(ln, 1))
    mag = np.abs(Cc)
    gain = 1.0 if side == BOTH else 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        audio = gain * np.where(mag == 0, B.real, (B.real * Cc.real + B.imag * Cc.imag) / mag)
    for f in range(1, NF):  # the condition the derived bound stands on: a statement about the signal, checked on the truth
        cmin, cmax, bmax = mag[f].min(), mag[f].max(), np.abs(B[f]).max()
        assert cmin >= 0.5 * cmax and bmax / cmin <= 4.0, (is_real, n, win, side, f, cmin / cmax, bmax / cmin)
    return dict(B=B, C=Cc, audio=audio, pwr=pw, fwd_scale=fs, gain=gain)


def audio_bound(T, f):
    bmax, cmin = np.abs(T["B"][f]).max(), np.abs(T["C"][f]).min()
    return T["gain"] * 2e-4 * bmax * (1.0 + bmax / cmin)


def line_weights(h):
    """Hann weights over the samples of frames 2..24.  The 23 frames are no whole number of periods of the 1 kHz tone or of
    the interferer: an unweighted projection leaks the tone - six times the line measured here - into 700 Hz at 1 / (pi 300 T),
    -47 dB of the tone at n = 256, which is as large as what UPPER has left of the line; under the Hann weights the leakage
    falls with the third power of the distance and is gone"""
    return np.hanning((NF - 2) * h + 2)[1:-1]


def line(audio, hz):
    """amplitude of the line at `hz` in frames 2..24: the (Hann-weighted) projection of their samples on exp(2 pi i hz t)"""
    x = np.asarray(audio[2:], np.float64).reshape(-1)
    w = line_weights(x.size // (NF - 2))
    t = np.arange(x.size) / RATE
    return 2.0 * abs(np.sum(w * x * np.exp(-2j * np.pi * hz * t))) / w.sum()


def line_tolerance(T):
    """how far errors of at most audio_bound(T, f) per sample of frame f move a line: the projection weighs sample t with
    2 w_t / sum w"""
    w = line_weights(T["B"].shape[1]).reshape(NF - 2, -1).sum(axis=1)
    return 2.0 * float(np.dot(w, [audio_bound(T, f) for f in range(2, NF)]) / w.sum())


@functools.lru_cache(maxsize=None)
def truth_lines(is_real, n, k):
    """the 700 Hz and the 1 kHz line of window k in the truth, per sideband - and what the feature is for, as statements
    about the truth: UPPER loses the lower sideband's interferer (at least 30 dB below BOTH's line), LOWER holds all of it
    (within 1 dB of twice BOTH's line: BOTH's real part shows one of the two halves the doubling restores)"""
    w = windows(n)[k]
    res = {s: (line(truth(is_real, n, w, s)["audio"], 700.0), line(truth(is_real, n, w, s)["audio"], 1000.0)) for s in (BOTH, UPPER, LOWER)}
    assert res[UPPER][0] <= res[BOTH][0] * 10 ** (-30 / 20), (is_real, n, k, res)
    assert abs(20 * np.log10(res[LOWER][0] / (2 * res[BOTH][0]))) <= 1.0, (is_real, n, k, res)
    return res


class Rig:
    """one context on the shared stream; batch(F) transforms and demodulates the next F frames"""

    def __init__(self, is_real, n, max_clients=8, post=False, pcm16=False, rate=RATE):
        from phantomsdr_amd import Context
        self.N, self.is_real, self.n, self.h = SHAPES[is_real], is_real, n, n // 2
        raw, _ = stream(is_real, n)
        self.ctx = Context(self.N, is_real, LEVELS, additional_size=n, audio_fft_size=n, audio_rate=rate, input_format="s16",
                           max_batch=MAXB, max_clients=max_clients)
        self.d = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.d, raw)
        if post:
            if pcm16:
                self.ctx.set_option(self.ctx.OPT_POST_CHAIN_PCM16, 1)
            self.ctx.set_post_chain(True)
        self.frame = 0

    def add(self, mode, win, side=None):
        from phantomsdr_amd import AudioClient
        g = AudioClient(self.ctx)
        g.set_audio_demodulation(mode)
        if side is not None:
            g.set_sam_sideband(side)
        g.set_audio_range(*win)
        return g

    def batch(self, F):
        self.ctx.process_batch(self.d, F, offset_bytes=self.frame * self.ctx.half_frame_bytes())
        self.ctx.demod_batch(self.frame)
        self.frame += F

    def close(self):
        self.ctx.dev_free(self.d)
        self.ctx.close()


def read_sam(g):
    """(audio, pwr, nan, level, offset_hz) of the last batch"""
    return g.read_audio(MAXB) + g.read_carrier(MAXB)


def cat(per_batch):
    return tuple(np.concatenate([b[i] for b in per_batch]) for i in range(len(per_batch[0])))


def run(is_real, n, specs, batches=BATCHES, read="read", rate=RATE):
    """specs: (mode, window, sideband) per client -> per client the 25 frames' (audio, pwr, nan, level, offset_hz) for a SAM
    client, (iq, pwr, nan) for an IQ client, (audio, pwr, nan) for any other"""
    rig = Rig(is_real, n, max_clients=max(4, len(specs)), rate=rate)
    try:
        cl = [rig.add(*s) for s in specs]
        got = [[] for _ in cl]
        for F in batches:
            rig.batch(F)
            if read == "fetch_batch":
                rig.ctx.fetch_batch()
            elif read == "fetch":
                rig.ctx.fetch_begin(rig.ctx.FETCH_AUDIO)
                rig.ctx.fetch_end()
            for k, (g, s) in enumerate(zip(cl, specs)):
                if read != "read":
                    rows = [rig.ctx.fetched_audio(g.id, f) for f in range(F)]
                    car = [rig.ctx.fetched_carrier(g.id, f) for f in range(F)]
                    got[k].append((np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.float32), np.array([r[2] for r in rows], np.int32),
                                   np.array([c[0] for c in car], np.float32), np.array([c[1] for c in car], np.float32)))
                elif s[0] == "SAM":
                    got[k].append(tuple(x[:F] for x in read_sam(g)))
                elif s[0] == "IQ":
                    got[k].append(tuple(x[:F] for x in g.read_iq(MAXB)))
                else:
                    got[k].append(tuple(x[:F] for x in g.read_audio(MAXB)))
        return [cat(per) for per in got]
    finally:
        rig.close()


NAMES = ("audio", "pwr", "nan flags", "carrier level", "carrier offset")


def same_bits(a, b, tag, what=NAMES):
    for x, y, w in zip(a, b, what):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{tag}: {w} differ"


def twice_re(iq):
    return np.ascontiguousarray(np.float32(2.0) * iq.real.astype(np.float32))


# ---- 1. bit relations --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("is_real", [0, 1])
@pytest.mark.parametrize("n,chain", PATHS, ids=PATH_IDS)
def test_carrier_and_pwr_are_the_both_sideband_twins(n, chain, is_real, monkeypatch):
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    wins = windows(n)[:2]
    got = run(is_real, n, [("SAM", w, s) for w in wins for s in (BOTH, UPPER, LOWER)])
    on_chain = n in (360, 720) and chain == "1"
    for k, w in enumerate(wins):
        both, T = got[3 * k], truth(is_real, n, w, BOTH)
        assert np.abs(both[3]).min() > 0
        for i, s in ((1, UPPER), (2, LOWER)):
            g, tag = got[3 * k + i], f"n {n} chain {chain} real {is_real} window {k} {s}"
            assert not g[2].any(), tag
            same_bits(g[3:], both[3:], tag, NAMES[3:])
            if on_chain:
                assert g[1].tobytes() == both[1].tobytes(), f"{tag}: pwr differs"
            for f in range(NF):
                assert abs(g[1][f] - both[1][f]) <= pwr_tolerance(T["pwr"][f], T["fwd_scale"][f]), (tag, f)
            assert g[0].tobytes() != both[0].tobytes() and np.abs(g[0]).max() > 0, f"{tag}: the sideband changed nothing"


@pytest.mark.parametrize("n,chain,is_real", [(360, "1", 0), (720, "1", 1), (360, "0", 1), (256, "1", 0), (1024, "1", 1)])
def test_window_without_a_carrier_bin_gives_twice_the_iq_rows_real_parts(n, chain, is_real, monkeypatch):
    """no kept bin: C = 0 exactly, audio = 2 B'.re.  The window lies above floor(audio_mid): UPPER clips nothing (B' is the
    PSDR_IQ row of the same window), LOWER everything (silence)"""
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    w = windows(n)[2]
    assert w[0] > int(w[1]) + cutoff(n) + 1 and w[2] > w[0] and clipped(w, UPPER) == w and clipped(w, LOWER)[2] == w[0]
    up, lo, iq = run(is_real, n, [("SAM", w, UPPER), ("SAM", w, LOWER), ("IQ", w, None)])
    assert not up[2].any() and np.abs(up[0]).max() > 0
    assert up[0].tobytes() == twice_re(iq[0]).tobytes()
    assert not lo[0].any() and not lo[2].any()
    assert up[1].tobytes() == lo[1].tobytes() and up[1].min() > 0  # pwr: the whole window's, whatever is placed
    for g in (up, lo):
        assert not g[3].any() and not g[4].any()


@pytest.mark.parametrize("n,is_real", [(360, 0), (720, 1), (256, 1), (1024, 0)])
def test_with_cutoff_zero_the_audio_is_twice_the_clipped_iq_rows_real_parts_on_every_path(n, is_real, monkeypatch):
    """audio_rate 500 n + 1: C = 0 everywhere, audio = 2 B'.re with B' the PSDR_IQ row of a client on the CLIPPED window (all
    fresh clients: every tail starts from zero, so from the first frame on) - and at n = 360 / 720 the same bits from
    k_demod_chain_sbsam and from k_demod_idft_fixed + k_demod_ola_sbsam"""
    rate = zero_cutoff_rate(n)
    assert cutoff(n, rate) == 0
    wins = windows(n)[:2]
    specs = [("SAM", w, s) for w in wins for s in (UPPER, LOWER)] + [("IQ", clipped(w, s), None) for w in wins for s in (UPPER, LOWER)]
    per_path = []
    for chain in (("1", "0") if n in (360, 720) else ("1",)):
        monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
        got = run(is_real, n, specs, rate=rate)
        for k in range(4):
            sb, iq = got[k], got[4 + k]
            assert np.abs(sb[0]).max() > 0 and not sb[2].any()
            assert sb[0].tobytes() == twice_re(iq[0]).tobytes(), f"n {n} chain {chain} real {is_real} client {k}"
        per_path.append(got[:4])
    if len(per_path) == 2:
        for k in range(4):
            same_bits(per_path[0][k], per_path[1][k], f"n {n} real {is_real} client {k}: PSDR_DEMOD_CHAIN 1 against 0")


# ---- 2. float64 truth --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("is_real", [0, 1])
@pytest.mark.parametrize("n,chain", PATHS, ids=PATH_IDS)
def test_audio_equals_the_truth(n, chain, is_real, monkeypatch):
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    wins = windows(n)[:2]
    specs = [("SAM", w, s) for w in wins for s in (UPPER, LOWER)]
    tr = [truth(is_real, n, w, s) for _, w, s in specs]
    got = run(is_real, n, specs)
    for (_, w, s), (audio, pwr, nan, _, _), T in zip(specs, got, tr):
        assert audio.shape == (NF, n // 2) and audio.dtype == np.float32
        assert not nan.any()
        for f in range(1, NF):
            tag = f"n {n} chain {chain} real {is_real} window {w} {s} frame {f}"
            d, bound = float(np.abs(audio[f] - T["audio"][f]).max()), audio_bound(T, f)
            print(f"{tag}: max |d| {d:.3e}, bound {bound:.3e}")
            assert d <= bound, tag
            assert abs(pwr[f] - T["pwr"][f]) <= pwr_tolerance(T["pwr"][f], T["fwd_scale"][f]), tag


# ---- 3. what the feature is for ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,chain,is_real", [(360, "1", 0), (720, "1", 1), (360, "0", 1), (256, "1", 0), (1024, "1", 1)])
def test_the_interferer_leaves_the_upper_sideband_and_stays_in_the_lower(n, chain, is_real, monkeypatch):
    """the 700 Hz line of the three detectors matches the truth's - which has it 30 dB down in UPPER and doubled in LOWER
    (truth_lines) - within the audio's bound as the projection passes it on (line_tolerance).  The 1 kHz tone comes out of
    all three at one amplitude, within 1 %."""
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    for k, w in enumerate(windows(n)[:2]):
        want = truth_lines(is_real, n, k)
        got = run(is_real, n, [("SAM", w, s) for s in (BOTH, UPPER, LOWER)])
        tone = {}
        for s, g in zip((BOTH, UPPER, LOWER), got):
            T = truth(is_real, n, w, s)
            tol = line_tolerance(T)
            l700, tone[s] = line(g[0], 700.0), line(g[0], 1000.0)
            print(f"n {n} chain {chain} real {is_real} window {k} {s}: 700 Hz {l700:.4e} (truth {want[s][0]:.4e}, tolerance {tol:.1e}), 1 kHz {tone[s]:.4e}")
            assert abs(l700 - want[s][0]) <= tol, (k, s)
        for s in (UPPER, LOWER):
            assert abs(tone[s] - tone[BOTH]) <= 0.01 * tone[BOTH], (k, s, tone)


# ---- 4. invariance -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,chain,is_real", [(360, "1", 0), (720, "1", 1), (360, "0", 1), (256, "1", 1), (1024, "1", 0)])
def test_batch_splits_give_the_same_bits(n, chain, is_real, monkeypatch):
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    specs = [("SAM", w, s) for w in windows(n) for s in (UPPER, LOWER)]
    a = run(is_real, n, specs)
    b = run(is_real, n, specs, batches=(5, 19, 1))
    for k in range(len(specs)):
        same_bits(a[k], b[k], f"client {k}: 19 + 1 + 5 against 5 + 19 + 1")


@pytest.mark.parametrize("n,is_real", [(360, 1), (720, 0)])
def test_the_two_paths_differ_only_as_sams_own_two_do(n, is_real, monkeypatch):
    """PSDR_DEMOD_CHAIN=0 against =1 with a carrier: the sideband client's carrier records are its PSDR_SAM_BOTH twin's on
    either path (test 1), pwr has the same bits, and the audio - B' identical (the cutoff-zero test), C in its last bits -
    stays inside twice the truth's bound"""
    wins = windows(n)[:2]
    specs = [("SAM", w, s) for w in wins for s in (UPPER, LOWER)]
    res = []
    for chain in ("1", "0"):
        monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
        res.append(run(is_real, n, specs))
    for (_, w, s), a, b in zip(specs, *res):
        T = truth(is_real, n, w, s)
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
        for f in range(1, NF):
            assert np.abs(a[0][f] - b[0][f]).max() <= 2 * audio_bound(T, f), (w, s, f)
            assert abs(a[3][f] - b[3][f]) <= 2e-4 * a[3][f], (w, s, f)


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_every_way_to_read_gives_the_same_rows(n, is_real):
    specs = [("SAM", w, s) for w, s in zip(windows(n), (UPPER, LOWER, UPPER))]
    a = run(is_real, n, specs)
    b = run(is_real, n, specs, read="fetch_batch")
    c = run(is_real, n, specs, read="fetch")
    for k in range(len(specs)):
        same_bits(a[k], b[k], f"client {k}: psdr_read_audio / _carrier against psdr_fetch_batch")
        same_bits(a[k], c[k], f"client {k}: psdr_read_audio / _carrier against psdr_fetch_begin / _end")


# ---- 5. state ----------------------------------------------------------------------------------------------------------

STRETCHES = ((BOTH, 7), (UPPER, 6), (LOWER, 5), (BOTH, 7))  # frames 0..6, 7..12, 13..17, 18..24


def run_stretches(is_real, n, rate):
    """window 0 over the 25 frames: x walks through STRETCHES, y stays BOTH, wu / wl are UPPER / LOWER all along, fu / fl are
    FRESH clients added right before the UPPER / the LOWER stretch -> dict of per-client rows (fu, fl: from their first frame)"""
    w = windows(n)[0]
    rig = Rig(is_real, n, max_clients=6, rate=rate)
    try:
        cl = dict(x=rig.add("SAM", w), y=rig.add("SAM", w), wu=rig.add("SAM", w, UPPER), wl=rig.add("SAM", w, LOWER))
        got = {k: [] for k in ("x", "y", "wu", "wl", "fu", "fl")}
        for i, (side, F) in enumerate(STRETCHES):
            cl["x"].set_sam_sideband(side)
            if i == 1:
                cl["fu"] = rig.add("SAM", w, UPPER)
            if i == 2:
                cl["fl"] = rig.add("SAM", w, LOWER)
            rig.batch(F)
            for k, g in cl.items():
                got[k].append(tuple(v[:F] for v in read_sam(g)))
        return {k: cat(v) for k, v in got.items()}
    finally:
        rig.close()


@pytest.mark.parametrize("n,chain,is_real", [(360, "1", 0), (720, "1", 1), (360, "0", 1), (256, "1", 0)])
def test_changes_of_sideband_keep_the_carrier_and_restart_the_sideband_tail(n, chain, is_real, monkeypatch):
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    g = run_stretches(is_real, n, RATE)
    x, y, wu, wl = g["x"], g["y"], g["wu"], g["wl"]
    # the carrier never notices: its records are those of the client that stayed BOTH, all 25 frames; so is pwr on the chain path
    same_bits(x[3:], y[3:], "carrier records through BOTH -> UPPER -> LOWER -> BOTH", NAMES[3:])
    assert x[0][:7].tobytes() == y[0][:7].tobytes()
    # a stretch starts from a ZERO sideband tail: its first frame is not the one of a client that had the sideband all along,
    # every later one is (the same carrier, the tail of the stretch's own first frame)
    assert x[0][7].tobytes() != wu[0][7].tobytes() and x[0][8:13].tobytes() == wu[0][8:13].tobytes()
    assert x[0][13].tobytes() != wl[0][13].tobytes() and x[0][14:18].tobytes() == wl[0][14:18].tobytes()
    # back in BOTH the AM / FM tail is the one from before the stretches (copied through, frame 6's): one frame later it is y's
    assert x[0][18].tobytes() != y[0][18].tobytes() and x[0][19:].tobytes() == y[0][19:].tobytes()
    assert not x[2].any()
    # with C = 0 a fresh client has "the same carrier tail": the stretch's first frame IS a fresh client's first frame
    z = run_stretches(is_real, n, zero_cutoff_rate(n))
    assert np.abs(z["x"][0][7]).max() > 0 and z["x"][0][7:13].tobytes() == z["fu"][0][:6].tobytes()
    assert z["x"][0][13:18].tobytes() == z["fl"][0][:5].tobytes()
    assert z["x"][0][7].tobytes() != z["wu"][0][7].tobytes() and z["x"][0][13].tobytes() != z["wl"][0][13].tobytes()


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_am_and_fm_continue_behind_a_sideband_stretch_as_behind_a_pause(n, is_real):
    """AM / FM 7 frames -> SAM UPPER 6 -> AM / FM 12: the sideband stretch copies AM's tail and FM's last sample through, so
    the third batch equals, bit for bit, that of a twin that was PAUSED over the stretch"""
    w = windows(n)[1]
    rig = Rig(is_real, n)
    try:
        cl = [rig.add("AM", w), rig.add("FM", w), rig.add("AM", w), rig.add("FM", w)]
        rig.batch(7)
        for g in cl[:2]:
            g.set_sam_sideband(LOWER)
            g.set_audio_demodulation("SAM")
        for g in cl[2:]:
            g.set_paused(True)
        rig.batch(6)
        assert np.abs(cl[0].read_audio(MAXB)[0]).max() > 0
        for g, mode in zip(cl[:2], ("AM", "FM")):
            g.set_audio_demodulation(mode)
        for g in cl[2:]:
            g.set_paused(False)
        rig.batch(12)
        for a, b, mode in zip(cl[:2], cl[2:], ("AM", "FM")):
            same_bits(a.read_audio(MAXB), b.read_audio(MAXB), f"{mode} behind a sideband stretch against {mode} behind a pause")
    finally:
        rig.close()


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_paused_sideband_client_keeps_its_state(n, is_real):
    """paused over the one-frame batch (frame 19): frames 20..24 continue from frame 18's tails, bit for bit as in a run of
    one-frame batches paused over the same frame"""
    from phantomsdr_amd import PsdrError

    def go(batches):
        rig = Rig(is_real, n)
        try:
            g, other = rig.add("SAM", windows(n)[0], UPPER), rig.add("SAM", windows(n)[1], LOWER)
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
                    out.append(read_sam(g))
            return cat(out)
        finally:
            rig.close()

    a, b = go(BATCHES), go((1,) * NF)
    assert a[0].shape == (NF - 1, n // 2)
    same_bits(a, b, "paused over frame 19")
    never = run(is_real, n, [("SAM", windows(n)[0], UPPER)])[0]
    assert a[0][:19].tobytes() == never[0][:19].tobytes() and a[0][19].tobytes() != never[0][20].tobytes()


def run_neighbours(is_real, n, with_sb):
    """19 + 1 + 5 frames with the post chain on: an AM, a USB and an IQ client; with_sb: a sideband SAM client in the slot
    between them"""
    rig = Rig(is_real, n, max_clients=6, post=True)
    try:
        w = windows(n)
        old = [rig.add("AM", w[1]), rig.add("USB", w[0])]
        if with_sb:
            sb = rig.add("SAM", w[0], LOWER)
            assert sb.id == 2
        iq = rig.add("IQ", w[0])
        res = []
        for F in BATCHES:
            rig.batch(F)
            res.append([g.read_audio(MAXB) + (g.read_pcm(MAXB),) for g in old] + [iq.read_iq(MAXB)])
            if with_sb:
                assert np.abs(sb.read_audio(MAXB)[0]).max() > 0
        return res
    finally:
        rig.close()


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_other_clients_do_not_notice_a_sideband_client(n, is_real):
    a, b = run_neighbours(is_real, n, False), run_neighbours(is_real, n, True)
    for bi, (ra, rb) in enumerate(zip(a, b)):
        for k, (x, y) in enumerate(zip(ra, rb)):
            for u, v in zip(x, y):
                assert u.shape == v.shape and u.tobytes() == v.tobytes(), f"client {k} batch {bi} differs with a sideband SAM client beside it"


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_the_setter_the_option_and_the_errors(n, is_real):
    w = windows(n)[0]
    rig = Rig(is_real, n, max_clients=12)
    try:
        lib, hdl = rig.ctx.lib, rig.ctx.h
        # in every mode but SAM the value is stored and has no effect; on a SAM client the fine-tune flag has none
        plain = [rig.add(m, w) for m in ("AM", "USB", "FM")]
        sided = [rig.add(m, w, UPPER) for m in ("AM", "USB", "FM")]
        up, up_fine, both = rig.add("SAM", w, UPPER), rig.add("SAM", w, UPPER), rig.add("SAM", w)
        up_fine.set_fine_tune(True)
        # the option: what psdr_client_add hands out from now on; existing clients keep theirs
        rig.ctx.set_option(rig.ctx.OPT_SAM_SIDEBAND, 1)
        opt_up = rig.add("SAM", w)
        rig.ctx.set_option(rig.ctx.OPT_SAM_SIDEBAND, 0)
        opt_both = rig.add("SAM", w)
        assert lib.psdr_set_option(hdl, rig.ctx.OPT_SAM_SIDEBAND, 3) == INVALID
        assert lib.psdr_set_option(hdl, rig.ctx.OPT_SAM_SIDEBAND, -1) == INVALID
        assert lib.psdr_client_set_sam_sideband(hdl, up.id, 3) == INVALID
        assert lib.psdr_client_set_sam_sideband(hdl, up.id, -1) == INVALID
        assert lib.psdr_client_set_sam_sideband(hdl, 11, 1) == INVALID  # a slot without a client
        assert lib.psdr_client_set_sam_sideband(hdl, 12, 1) == INVALID and lib.psdr_client_set_sam_sideband(hdl, -1, 1) == INVALID
        for F in BATCHES:
            rig.batch(F)
            for a, b in zip(plain, sided):
                same_bits(a.read_audio(MAXB), b.read_audio(MAXB), "a sideband on a client that is not SAM")
            r_up, r_both = read_sam(up), read_sam(both)
            same_bits(read_sam(up_fine), r_up, "the fine-tune flag on a sideband SAM client")
            same_bits(read_sam(opt_up), r_up, "a client added under PSDR_OPT_SAM_SIDEBAND = 1")
            same_bits(read_sam(opt_both), r_both, "a client added after the option went back to 0")
            assert r_up[0].tobytes() != r_both[0].tobytes()
    finally:
        rig.close()


# ---- 6. post chain and fetch -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,is_real,pcm16", [(360, 0, False), (360, 0, True), (256, 1, False)])
def test_post_chain_of_a_sideband_client_is_bit_exact(n, is_real, pcm16):
    """the oracle's DC blocker + AGC + int16 conversion fed the GPU's own float rows: the PCM must be identical"""
    rig = Rig(is_real, n, post=True, pcm16=pcm16)
    try:
        gs = [rig.add("SAM", w, s) for w, s in zip(windows(n)[:2], (UPPER, LOWER))]
        chains = [O.PostChain(RATE) for _ in gs]
        total = 0
        for F in BATCHES:
            rig.batch(F)
            rig.ctx.fetch_begin(rig.ctx.FETCH_AUDIO | rig.ctx.FETCH_PCM)
            rig.ctx.fetch_end()
            for g, ch in zip(gs, chains):
                audio, pwr, nan = g.read_audio(MAXB)
                lv, off = g.read_carrier(MAXB)
                pcm = g.read_pcm(MAXB)
                assert not nan.any()
                for f in range(F):
                    want = ch.process(audio[f])
                    assert np.array_equal(pcm[f], want), f"frame {f}: {np.count_nonzero(pcm[f] != want)} samples differ"
                    fa = rig.ctx.fetched_audio(g.id, f)
                    assert fa[0].tobytes() == audio[f].tobytes() and fa[1] == pwr[f] and fa[2] == nan[f]
                    assert rig.ctx.fetched_carrier(g.id, f) == (float(lv[f]), float(off[f]))
                    if pcm16:
                        row = rig.ctx.fetched_pcm16(g.id, f)
                        assert row.dtype == np.int16 and np.array_equal(row.astype(np.int32), want)
                    total += int(np.count_nonzero(want))
        assert total > 1000, "the AGC never opened: the test did not exercise the chain"
    finally:
        rig.close()

"""Fine tuning below one FFT bin on the GPU (include/psdr.h: psdr_client_set_fine_tune): USB / LSB / IQ clients with the flag
on, against their untuned twins, against a float64 evaluation of the definition on the ORACLE's spectra, and bit for bit
against themselves across batch splits, paths, mode switches and pauses.

Shapes, stream construction and Rig follow test_gpu_sam_mode.py: 2^12-point IQ and 2^13-point real (R = 4096 either way), s16
input, 25 frames as batches of 19 + 1 + 5, audio_rate 12000.  n = 360 / 720: k_demod_chain_ft (PSDR_DEMOD_CHAIN=0:
k_demod_idft_fixed + k_demod_ola_ft), 256: k_demod_idft_wave + k_demod_ola_ft, 1024: k_demod_idft + k_demod_ola_ft.

Signal: noise of sigma 2^-9 and one unmodulated carrier of amplitude 8 / sqrt(N), 0.37 bin above bin KC.

Bounds, derived.  The rotator against float64 (test 1): the phase as f32 turns 2^-25 turn = 1.9e-7 rad, two ulp of a sine or
cosine 2.4e-7, up to three complex f32 products 1.7e-7 each: about 1e-6 in all, the bound is twice that, relative to the
frame's largest sample.  USB / LSB (test 2) double the product: 4e-6.  Against float64 spectra (test 3) the transform's own
bound, the project's 2e-4 of AM, comes on top, and the audio is twice a real part."""
import ctypes as C
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
PATHS = [(360, "1"), (360, "0"), (720, "1"), (720, "0"), (256, "1"), (1024, "1")]  # (n, PSDR_DEMOD_CHAIN)
PATH_IDS = [f"{n}-chain{c}" for n, c in PATHS]
MASK = (1 << 32) - 1


@functools.lru_cache(maxsize=None)
def stream(is_real):
    N = SHAPES[is_real]
    ns = (NF + 1) * (N // 2)
    rng = np.random.default_rng(190 + is_real)
    t = np.arange(ns, dtype=np.float64)
    amp = 8.0 / np.sqrt(N)
    if is_real:
        x = rng.standard_normal(ns) * 2.0 ** -9 + amp * np.cos(2 * np.pi * (KC + OFFSET_BINS) / N * t)
    else:
        fc = ((KC + OFFSET_BINS + N // 2 + 1) % N) / N  # client bin c is frequency index (c + N/2 + 1) mod N
        x = (rng.standard_normal(ns) + 1j * rng.standard_normal(ns)) * 2.0 ** -9 + amp * np.exp(2j * np.pi * fc * t)
    raw = quantize_raw(x, "s16", bool(is_real))
    conv = O.convert(raw, "s16")
    halves = (conv if is_real else conv.view(np.complex64)).reshape(NF + 1, N // 2)
    return raw, halves


@functools.lru_cache(maxsize=None)
def oracle_spectra(is_real, n):
    """the reference's spectra of the 25 frames (wrap copy of n bins), computed once per shape and left alone"""
    N = SHAPES[is_real]
    _, halves = stream(is_real)
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


def clipped(mode, win):
    """the window clipped to the sideband: what a tuned USB / LSB client places"""
    l, mid, r = win
    m = int(np.floor(mid))
    if mode == "USB":
        return min(max(l, m), r), mid, r
    if mode == "LSB":
        return l, mid, max(min(r, m + 1), l)
    return win


def baseband64(is_real, n, win, fa, fb):
    """baseband64_of on the oracle's spectra"""
    fo, specs = oracle_spectra(is_real, n)
    return baseband64_of(specs, lambda s, l, ln: s[fo.slice_ptr_index(l):fo.slice_ptr_index(l) + ln], is_real, n, win, fa, fb)


def baseband64_of(specs, slice_of, is_real, n, win, fa, fb):
    """float64: the AM / FM placement of the window's bins, np.fft.ifft * n, flip, overlap-add from a ZERO tail at frame fa:
    B[fa..fb) complex128 [fb - fa][h].  specs: one spectrum per frame; slice_of(spectrum, l, ln): its bins [l, l + ln) in
    client order"""
    l, mid, r = win
    h, m_floor = n // 2, int(np.floor(mid))
    B, bt = np.zeros((fb - fa, h), np.complex128), np.zeros(h, np.complex128)
    for f in range(fa, fb):
        S = slice_of(specs[f], l, r - l).astype(np.complex128)
        X = np.zeros(n, np.complex128)
        for t in range(r - l):
            d = l + t - m_floor
            if 0 <= d < h:
                X[d] = S[t]
            elif -(h - 1) <= d < 0:
                X[n + d] = S[t]
        y = np.fft.ifft(X) * n
        s = flip_sign(f, m_floor, is_real)
        B[f - fa], bt = s * y[:h] + bt, s * y[h:]
    return B


class Phase:
    """the integer recurrence of psdr.h: phi of every sample of a batch, and the accumulator behind it"""

    def __init__(self, n):
        self.n, self.h, self.phi = n, n // 2, 0

    def batch(self, mid, F):
        delta = mid - np.floor(mid)
        step = int(np.floor(delta * 2.0 ** 32 / self.n + 0.5))
        assert 0 <= step < 1 << 30
        k = np.arange(F * self.h, dtype=np.uint64).reshape(F, self.h)
        ph = (np.uint64(self.phi) + k * np.uint64(step)) & np.uint64(MASK)
        self.phi = (self.phi + F * self.h * step) & MASK
        return ph


def w64(ph):
    return np.exp(-2j * np.pi * ph.astype(np.float64) / 2.0 ** 32)


class Rig:
    """one context on the shared stream; batch(F) transforms and demodulates the next F frames"""

    def __init__(self, is_real, n, max_clients=8, post=False, pcm16=False):
        from phantomsdr_amd import Context
        self.N, self.is_real, self.n, self.h = SHAPES[is_real], is_real, n, n // 2
        raw, _ = stream(is_real)
        self.ctx = Context(self.N, is_real, LEVELS, additional_size=n, audio_fft_size=n, audio_rate=RATE, input_format="s16",
                           max_batch=MAXB, max_clients=max_clients)
        self.d = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.d, raw)
        if post:
            if pcm16:
                self.ctx.set_option(self.ctx.OPT_POST_CHAIN_PCM16, 1)
            self.ctx.set_post_chain(True)
        self.frame = 0

    def add(self, mode, win, fine=False):
        from phantomsdr_amd import AudioClient
        g = AudioClient(self.ctx)
        g.set_audio_demodulation(mode)
        g.set_audio_range(*win)
        if fine:
            g.set_fine_tune(True)
        return g

    def batch(self, F):
        ctx = self.ctx
        ctx.process_batch(self.d, F, offset_bytes=self.frame * ctx.half_frame_bytes())
        ctx.demod_batch(self.frame)
        self.frame += F

    def skip(self, F):
        """the next F frames are not demodulated at all"""
        self.frame += F

    def close(self):
        self.ctx.dev_free(self.d)
        self.ctx.close()


def read(g, mode):
    """(rows, pwr, nan) of the last batch: complex rows of an IQ client, float rows of any other"""
    return g.read_iq(MAXB) if mode == "IQ" else g.read_audio(MAXB)


def wide(n, m):
    """a window around bin m that reaches h - 2 bins below and above it"""
    w = n // 2 - 2
    return m - w, m + w


# ---- 1. the rotator, sharply -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("pause", [False, True], ids=["run", "pause"])
@pytest.mark.parametrize("n,chain", PATHS, ids=PATH_IDS)
def test_tuned_iq_is_its_untuned_twin_times_the_rotator(n, chain, pause, monkeypatch):
    """the fraction changes at both batch boundaries (0.37 -> 0.81 -> 0.0); pause: both clients sit out the one-frame batch,
    and the phase stands still with them"""
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    is_real = (n // 8) % 2
    l, r = wide(n, KC)
    fracs = (0.37, 0.81, 0.0)
    rig, ph = Rig(is_real, n), Phase(n)
    try:
        twin, tuned = rig.add("IQ", (l, float(KC), r)), rig.add("IQ", (l, KC + fracs[0], r), fine=True)
        worst = 0.0
        for b, F in enumerate(BATCHES):
            tuned.set_audio_range(l, KC + fracs[b], r)
            paused = pause and b == 1
            twin.set_paused(paused)
            tuned.set_paused(paused)
            rig.batch(F)
            if paused:
                continue
            (a, pa, na), (t, pt, nt) = twin.read_iq(MAXB), tuned.read_iq(MAXB)
            phi = ph.batch(KC + fracs[b], F)
            assert not na.any() and not nt.any()
            assert all(abs(float(x) - float(y)) <= pwr_tolerance(float(x)) for x, y in zip(pa, pt))
            for f in range(F):
                d = float(np.abs(t[f].astype(np.complex128) - a[f].astype(np.complex128) * w64(phi[f])).max())
                scale = float(np.abs(a[f]).max())
                worst = max(worst, d / scale)
                assert d <= 2e-6 * scale, f"n {n} chain {chain} batch {b} frame {f}: {d / scale:.3e} of the frame's maximum"
        print(f"n {n} chain {chain} pause {pause}: worst |tuned - twin w64| / max |twin| = {worst:.3e}")
    finally:
        rig.close()


# ---- 2. tuned USB / LSB against their twins --------------------------------------------------------------------------

def ssb_windows(n, mode):
    """floor(mid) even and odd; the window reaches 20 bins into the other sideband, so the clip does something"""
    h = n // 2
    if mode == "USB":
        return [(KC - 20, KC + 0.37, KC + h - 2), (KC - 1 - 20, KC - 1 + 0.37, KC - 1 + h - 2)]
    return [(KC + 2 - (h - 2), KC + 2 + 0.37, KC + 2 + 20), (KC + 3 - (h - 2), KC + 3 + 0.37, KC + 3 + 20)]


@pytest.mark.parametrize("mode", ["USB", "LSB"])
@pytest.mark.parametrize("n,chain", PATHS, ids=PATH_IDS)
def test_tuned_ssb_is_twice_the_real_part_of_its_rotated_twin(n, chain, mode, monkeypatch):
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    is_real = (n // 8 + (mode == "LSB")) % 2
    wins = ssb_windows(n, mode)
    rig = Rig(is_real, n)
    try:
        tuned = [rig.add(mode, w, fine=True) for w in wins]
        twins, plain = [], []
        for w in wins:
            cl, _, cr = clipped(mode, w)
            assert (cl, cr) != (w[0], w[2]) and cr > cl
            twins.append(rig.add("IQ", (cl, float(np.floor(w[1])), cr)))
            plain.append(rig.add(mode, w))
        phs = [Phase(n) for _ in wins]
        for F in BATCHES:
            rig.batch(F)
            for k, w in enumerate(wins):
                a, pw, nan = tuned[k].read_audio(MAXB)
                tw = twins[k].read_iq(MAXB)[0].astype(np.complex128)
                phi = phs[k].batch(w[1], F)
                assert not nan.any()
                _, pp, _ = plain[k].read_audio(MAXB)
                for f in range(F):
                    tag = f"n {n} chain {chain} {mode} window {k} frame {rig.frame - F + f}"
                    want = 2.0 * (tw[f] * w64(phi[f])).real
                    d, scale = float(np.abs(a[f] - want).max()), float(np.abs(tw[f]).max())
                    assert d <= 4e-6 * scale, f"{tag}: {d / scale:.3e} of the twin's maximum"
                    assert abs(float(pw[f]) - float(pp[f])) <= pwr_tolerance(float(pp[f])), tag
    finally:
        rig.close()


# ---- 3. float64 anchor -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,chain", PATHS, ids=PATH_IDS)
def test_tuned_usb_equals_the_definition_in_float64(n, chain, monkeypatch):
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    is_real = (n // 8 + 1) % 2
    wins = ssb_windows(n, "USB")
    rig = Rig(is_real, n)
    try:
        gs = [rig.add("USB", w, fine=True) for w in wins]
        Bs = [baseband64(is_real, n, clipped("USB", w), 0, NF) for w in wins]
        phs = [Phase(n) for _ in wins]
        for F in BATCHES:
            rig.batch(F)
            for k, w in enumerate(wins):
                a, _, nan = gs[k].read_audio(MAXB)
                phi = phs[k].batch(w[1], F)
                assert not nan.any()
                for f in range(F):
                    B = Bs[k][rig.frame - F + f]
                    d = float(np.abs(a[f] - 2.0 * (B * w64(phi[f])).real).max())
                    bound = 2.0 * (2e-4 + 2e-6) * float(np.abs(B).max())
                    assert d <= bound, f"n {n} chain {chain} window {k} frame {rig.frame - F + f}: {d:.3e} > {bound:.3e}"
    finally:
        rig.close()


# ---- 4. the point of it ----------------------------------------------------------------------------------------------

def tone_hz(audio):
    """the frequency of the strongest line of frames 1..24: argmax of a zero-padded float64 periodogram (Hann window)"""
    x = audio[1:].reshape(-1).astype(np.float64)
    L = 1 << 21
    sp = np.abs(np.fft.rfft(x * np.hanning(x.size), L))
    return float(np.argmax(sp)) * RATE / L


@pytest.mark.parametrize("is_real", [0, 1])
def test_carrier_thirty_bins_above_the_tuning_is_a_1000_hz_note(is_real):
    """mid = KC - 30 + 0.37: the carrier is 30.00 bins above the tuning - 1000.0 Hz at 12 kHz and n = 360 - and 30.37 bins
    above bin floor(mid), which is where an untuned client hears it: 1012.3 Hz"""
    n = 360
    win = (KC - 30, KC - 30 + OFFSET_BINS, KC + 60)
    rig = Rig(is_real, n)
    try:
        tuned, plain = rig.add("USB", win, fine=True), rig.add("USB", win)
        rows = ([], [])
        for F in BATCHES:
            rig.batch(F)
            rows[0].append(tuned.read_audio(MAXB)[0])
            rows[1].append(plain.read_audio(MAXB)[0])
        f_tuned, f_plain = tone_hz(np.concatenate(rows[0])), tone_hz(np.concatenate(rows[1]))
        print(f"real {is_real}: tuned {f_tuned:.3f} Hz, untuned {f_plain:.3f} Hz")
        assert abs(f_tuned - 1000.0) <= 0.5
        assert abs(f_plain - 1012.3) <= 0.5
    finally:
        rig.close()


# ---- 5. batch splits -------------------------------------------------------------------------------------------------

def tuned_trio(n):
    l, r = wide(n, KC)
    return [("USB", ssb_windows(n, "USB")[1]), ("LSB", ssb_windows(n, "LSB")[0]), ("IQ", (l, KC + 0.63, r))]


def run_tuned(is_real, n, batches):
    """a tuned USB, LSB and IQ client over the 25 frames: per client (rows, pwr, nan)"""
    rig = Rig(is_real, n)
    try:
        cl = [(m, rig.add(m, w, fine=True)) for m, w in tuned_trio(n)]
        got = [[] for _ in cl]
        for F in batches:
            rig.batch(F)
            for k, (m, g) in enumerate(cl):
                got[k].append(read(g, m))
        return [tuple(np.concatenate([b[i] for b in per]) for i in range(3)) for per in got]
    finally:
        rig.close()


def same_bits(a, b, tag):
    for x, y, what in zip(a, b, ("rows", "pwr", "nan flags")):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{tag}: {what} differ"


@pytest.mark.parametrize("n,is_real", [(360, 0), (720, 1), (256, 1), (1024, 0)])
def test_batch_splits_and_paths_give_the_same_bits(n, is_real, monkeypatch):
    runs = {}
    for chain in (("1", "0") if n in (360, 720) else ("1",)):
        monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
        for split in (BATCHES, (7, 7, 7, 4)):
            runs[(chain, split)] = run_tuned(is_real, n, split)
    first_key = ("1", BATCHES)
    for k in range(3):
        assert np.abs(runs[first_key][k][0]).max() > 0 and not runs[first_key][k][2].any()
        for key, res in runs.items():
            same_bits(runs[first_key][k], res[k], f"n {n} client {k}: chain 1, 19 + 1 + 5 against chain {key[0]}, {key[1]}")


# ---- 6. neighbours and no-ops ----------------------------------------------------------------------------------------

def run_neighbours(is_real, n, with_tuned, flags_on=False, option_dance=False):
    """19 + 1 + 5 frames with the post chain on: USB, AM, FM, SAM and IQ clients, per client and batch (rows, pwr, nan[, pcm]);
    with_tuned: tuned clients in the slots between them; flags_on: the AM / FM / SAM clients carry the flag;
    option_dance: PSDR_OPT_FINE_TUNE is set to 1 and back to 0 before the clients are added"""
    rig = Rig(is_real, n, max_clients=10, post=True)
    try:
        if option_dance:
            rig.ctx.set_option(rig.ctx.OPT_FINE_TUNE, 1)
            rig.ctx.set_option(rig.ctx.OPT_FINE_TUNE, 0)
        l, r = wide(n, KC)
        w = (l, KC + 0.37, r)
        old = [("USB", rig.add("USB", w)), ("AM", rig.add("AM", w, fine=flags_on))]
        if with_tuned:
            for m, tw in tuned_trio(n):
                rig.add(m, tw, fine=True)
        old += [("FM", rig.add("FM", w, fine=flags_on)), ("SAM", rig.add("SAM", w, fine=flags_on)), ("IQ", rig.add("IQ", w))]
        res = [[] for _ in old]
        for F in BATCHES:
            rig.batch(F)
            for k, (m, g) in enumerate(old):
                res[k].append(read(g, m) + (() if m == "IQ" else (g.read_pcm(MAXB),)))
        return res
    finally:
        rig.close()


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_other_clients_and_other_modes_do_not_notice(n, is_real):
    base = run_neighbours(is_real, n, False)
    for what, other in (("a tuned client beside it", run_neighbours(is_real, n, True)),
                        ("the flag on in AM / FM / SAM", run_neighbours(is_real, n, False, flags_on=True)),
                        ("PSDR_OPT_FINE_TUNE set and cleared", run_neighbours(is_real, n, False, option_dance=True))):
        for k, (ra, rb) in enumerate(zip(base, other)):
            for bi, (x, y) in enumerate(zip(ra, rb)):
                for u, v in zip(x, y):
                    assert u.shape == v.shape and u.tobytes() == v.tobytes(), f"client {k} batch {bi} differs with {what}"


def test_option_gives_new_clients_the_flag():
    n, is_real = 360, 0
    win = ssb_windows(n, "USB")[0]
    rig = Rig(is_real, n)
    try:
        before = rig.add("USB", win)
        rig.ctx.set_option(rig.ctx.OPT_FINE_TUNE, 1)
        by_option = rig.add("USB", win)
        rig.ctx.set_option(rig.ctx.OPT_FINE_TUNE, 0)
        after, by_call = rig.add("USB", win), rig.add("USB", win, fine=True)
        rig.batch(5)
        rows = [g.read_audio(MAXB)[0] for g in (before, by_option, after, by_call)]
        assert rows[0].tobytes() == rows[2].tobytes()          # existing clients keep theirs; 0 again: as before
        assert rows[1].tobytes() == rows[3].tobytes() != rows[0].tobytes()
    finally:
        rig.close()


# ---- 7. mode switches ------------------------------------------------------------------------------------------------

SWITCH = [("USB", False, 5), ("USB", True, 6), ("AM", False, 4), ("LSB", True, 5), ("USB", True, 5)]


@pytest.mark.parametrize("mid_mode", ["AM", "FM"])
@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1), (720, 1)])
def test_mode_switches_leave_every_stream_continuous(n, is_real, mid_mode):
    """USB -> tuned USB -> AM (or FM: bb_last) -> tuned LSB -> tuned USB at batch boundaries.  The untuned stretches are
    bit-identical to a run that stayed untuned throughout; each tuned stretch is the float64 definition from a zero tail"""
    l, r = wide(n, KC + 1)
    win = (l, KC + 1 + 0.37, r)
    seq = [(mid_mode if m == "AM" else m, fine, F) for m, fine, F in SWITCH]
    rig, ref, ph = Rig(is_real, n), Rig(is_real, n), Phase(n)
    try:
        g, q = rig.add("USB", win), ref.add("USB", win)
        for mode, fine, F in seq:
            g.set_audio_demodulation(mode)
            q.set_audio_demodulation(mode)
            g.set_fine_tune(fine)
            f0 = rig.frame
            rig.batch(F)
            ref.batch(F)
            a, pw, nan = g.read_audio(MAXB)
            assert not nan.any()
            if not fine:
                for x, y in zip((a, pw, nan), q.read_audio(MAXB)):
                    assert x.tobytes() == y.tobytes(), f"n {n} {mode} from frame {f0}: differs from the run that stayed untuned"
                continue
            B = baseband64(is_real, n, clipped(mode, win), f0, f0 + F)
            phi = ph.batch(win[1], F)
            for f in range(F):
                d = float(np.abs(a[f] - 2.0 * (B[f] * w64(phi[f])).real).max())
                bound = 2.0 * (2e-4 + 2e-6) * float(np.abs(B[f]).max())
                assert d <= bound, f"n {n} tuned {mode} frame {f0 + f}: {d:.3e} > {bound:.3e}"
    finally:
        rig.close()
        ref.close()


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_paused_tuned_client_keeps_tail_and_phase(n, is_real):
    """paused over the one-frame batch, against a run in which that frame is not demodulated at all: the same bits"""
    def run(pause):
        rig = Rig(is_real, n)
        try:
            cl = [(m, rig.add(m, w, fine=True)) for m, w in tuned_trio(n)]
            out = [[] for _ in cl]
            for b, F in enumerate(BATCHES):
                if b == 1:
                    if not pause:
                        rig.skip(F)
                        continue
                    for _, g in cl[:2]:
                        g.set_paused(True)
                    other = cl[2][1]      # (a batch needs a client: the IQ one runs it and is left out of the comparison)
                    rig.batch(F)
                    from phantomsdr_amd import PsdrError
                    with pytest.raises(PsdrError) as e:
                        cl[0][1].read_audio(MAXB)
                    assert e.value.code == NO_DATA
                    other.read_iq(MAXB)
                    for _, g in cl[:2]:
                        g.set_paused(False)
                    continue
                rig.batch(F)
                for k, (m, g) in enumerate(cl):
                    out[k].append(read(g, m))
            return [tuple(np.concatenate([b[i] for b in per]) for i in range(3)) for per in out]
        finally:
            rig.close()

    a, b = run(True), run(False)
    for k in range(2):
        same_bits(a[k], b[k], f"n {n} client {k}: paused over frame 19 against frame 19 never demodulated")
    assert a[2][0][:19].tobytes() == b[2][0][:19].tobytes() and a[2][0][19:].tobytes() != b[2][0][19:].tobytes()


# ---- 8. post chain and read paths ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,is_real,pcm16", [(360, 0, False), (360, 0, True), (256, 1, False)])
def test_post_chain_of_a_tuned_usb_client_is_bit_exact(n, is_real, pcm16):
    """the oracle's DC blocker + AGC + int16 conversion fed the GPU's own tuned float rows: the PCM must be identical"""
    rig = Rig(is_real, n, post=True, pcm16=pcm16)
    try:
        gs = [rig.add("USB", w, fine=True) for w in ssb_windows(n, "USB")]
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


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_every_way_to_read_gives_the_same_rows(n, is_real):
    rig = Rig(is_real, n, post=True)
    try:
        (_, usb), (_, lsb), (_, iq) = [(m, rig.add(m, w, fine=True)) for m, w in tuned_trio(n)]
        ctx, h = rig.ctx, n // 2
        for F in BATCHES:
            rig.batch(F)
            for g in (usb, lsb):
                a, pw, nan = g.read_audio(MAXB)
                p, q = C.c_void_p(), C.c_void_p()
                assert ctx.lib.psdr_audio_device_ptr(ctx.h, g.id, C.byref(p), C.byref(q)) == 0 and p.value
                back = np.empty((F, h), np.float32)
                ctx.d2h(back, p)
                assert np.abs(a).max() > 0 and back.tobytes() == a.tobytes()
            rows, pw_iq, nan_iq = iq.read_iq(MAXB)
            p, q = C.c_void_p(), C.c_void_p()
            assert ctx.lib.psdr_iq_device_ptr(ctx.h, iq.id, C.byref(p), C.byref(q)) == 0 and p.value
            back = np.empty((F, h), np.complex64)
            ctx.d2h(back, p)
            assert back.tobytes() == rows.tobytes()
            pcm = [g.read_pcm(MAXB) for g in (usb, lsb)]
            want = [g.read_audio(MAXB) for g in (usb, lsb)]
            for how in ("fetch_batch", "fetch"):
                if how == "fetch_batch":
                    ctx.fetch_batch()
                else:
                    ctx.fetch_begin(ctx.FETCH_AUDIO | ctx.FETCH_PCM | ctx.FETCH_IQ)
                    ctx.fetch_end()
                for g, (a, pw, nan), pc in zip((usb, lsb), want, pcm):
                    for f in range(F):
                        fa, fp, fn, fpc = ctx.fetched_audio(g.id, f, pcm=True)
                        assert fa.tobytes() == a[f].tobytes() and fp == float(pw[f]) and fn == int(nan[f]), how
                        assert np.array_equal(fpc, pc[f]), how
                for f in range(F):
                    fi, fp, fn = ctx.fetched_iq(iq.id, f)
                    assert fi.tobytes() == rows[f].tobytes() and fp == float(pw_iq[f]) and fn == int(nan_iq[f]), how
    finally:
        rig.close()


# ---- 9. errors -------------------------------------------------------------------------------------------------------

def test_errors():
    from phantomsdr_amd import PsdrError
    n = 360
    rig = Rig(0, n, post=True)
    try:
        lib, hdl = rig.ctx.lib, rig.ctx.h
        l, r = wide(n, KC)
        iq, usb = rig.add("IQ", (l, KC + 0.37, r), fine=True), rig.add("USB", (l, KC + 0.37, r), fine=True)
        assert lib.psdr_client_set_fine_tune(hdl, 7, 1) == INVALID      # a free slot
        assert lib.psdr_client_set_fine_tune(hdl, -1, 1) == INVALID
        assert lib.psdr_client_set_fine_tune(hdl, 1000, 0) == INVALID
        assert lib.psdr_client_set_fine_tune(None, 0, 1) == INVALID
        assert lib.psdr_set_option(hdl, rig.ctx.OPT_FINE_TUNE, 2) == INVALID
        assert lib.psdr_set_option(hdl, rig.ctx.OPT_FINE_TUNE, -1) == INVALID
        rig.batch(5)
        rig.ctx.fetch_batch()
        for call in (lambda: iq.read_audio(MAXB), lambda: iq.read_pcm(MAXB), lambda: rig.ctx.fetched_audio(iq.id, 0),
                     lambda: usb.read_iq(MAXB), lambda: rig.ctx.fetched_iq(usb.id, 0)):
            with pytest.raises(PsdrError) as e:
                call()
            assert e.value.code == NO_DATA
        assert len(iq.read_iq(MAXB)[0]) == 5 and len(usb.read_audio(MAXB)[0]) == 5
    finally:
        rig.close()

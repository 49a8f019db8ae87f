"""PSDR_IQ on the GPU (include/psdr.h: psdr_read_iq): the overlap-added complex baseband of a client as its output, against
the oracle's audio_complex_baseband sample by sample, bit identities between the ways to produce and to read it, continuity
across mode switches, and that no other client notices.

Shapes: the smallest transforms (2^12-point IQ, 2^13-point real: R = 4096 either way), s16 input, 25 frames as batches of
19 + 1 + 5 - with three clients the chain kernel's default K falls to 4, so chains with a warm-up frame, a one-frame batch
and a ragged last chain all occur.  n = 360 / 720: k_demod_chain_iq (PSDR_DEMOD_CHAIN=0: k_demod_idft_fixed +
k_demod_ola_iq), 256: k_demod_idft_wave + k_demod_ola_iq, 1024: k_demod_idft + k_demod_ola_iq.

Bounds: those test_gpu_parity.py applies to AM audio, whose input this is - relative L2 < 1e-4 and max |d| <= 2e-4 * max |IQ|
per frame, pwr within helpers.pwr_tolerance, NaN flags 0."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import check_fm, pwr_tolerance, quantize_raw, rel_l2, synth_stream
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NF = 25
BATCHES = (19, 1, 5)
MAXB = 19
LEVELS = 3  # R = 4096, waterfall_size 1024
SHAPES = {0: 1 << 12, 1: 1 << 13}  # is_real -> N
NO_DATA, UNSUPPORTED = -7, -6


def tone_bin(N, is_real, fnorm):
    if is_real:
        return fnorm * N
    return (fnorm * N - (N // 2 + 1)) % N


def windows(is_real, n):
    """three windows on the AM carrier of helpers.synth_stream (0.11 cycles / sample), as test_gpu_parity.py places its
    clients: floor(audio_mid) even and odd (the flip rule, src/signal.cpp:223-234), and one with l = 0"""
    N = SHAPES[is_real]
    am = int(tone_bin(N, is_real, 0.11))
    am -= am & 1
    w = n // 2 - 2
    return [(am - w, float(am), am + w), (am + 1 - w, am + 1.5, am + 1 + w), (0, 30.0, 30 + n // 4)]


@functools.lru_cache(maxsize=None)
def stream(is_real):
    N = SHAPES[is_real]
    x = synth_stream((NF + 1) * (N // 2), bool(is_real), seed=90 + is_real, fft_size=N)
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


@functools.lru_cache(maxsize=None)
def oracle_baseband(is_real, n):
    """per window: (IQ[25][h], pwr[25], fwd_scale[25]) of an oracle client in AM mode - audio_complex_baseband[:h] after
    src/signal.cpp:235-237"""
    fo, specs = oracle_spectra(is_real, n)
    R, h = 4096, n // 2
    res = []
    for l, mid, r in windows(is_real, n):
        o = O.AudioClient(bool(is_real), n, 12000, R)
        o.set_audio_demodulation("AM")
        o.set_audio_range(l, mid, r)
        bb, pw, fs = np.zeros((NF, h), np.complex64), np.zeros(NF), np.zeros(NF)
        for f in range(NF):
            _, p, _, dropped = o.send_audio(specs[f], f, fft=fo)
            assert not dropped
            bb[f], pw[f], fs[f] = o.baseband()[:h], p, o.fwd_scale
        for a in (bb, pw, fs):
            a.setflags(write=False)
        res.append((bb, pw, fs))
    return res


class Rig:
    """one context on the shared stream; batch(F) transforms and demodulates the next F frames"""

    def __init__(self, is_real, n, max_clients=4, post=False):
        from phantomsdr_amd import Context
        self.N, self.is_real, self.n, self.h = SHAPES[is_real], is_real, n, n // 2
        raw, _ = stream(is_real)
        self.ctx = Context(self.N, is_real, LEVELS, additional_size=n, audio_fft_size=n, audio_rate=12000, input_format="s16",
                           max_batch=MAXB, max_clients=max_clients)
        self.d = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.d, raw)
        if post:
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

    def fetched_iq(self, g, F):
        rows = [self.ctx.fetched_iq(g.id, f) for f in range(F)]
        return (np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.float32), np.array([r[2] for r in rows], np.int32))

    def close(self):
        self.ctx.dev_free(self.d)
        self.ctx.close()


def run_iq(is_real, n, batches=BATCHES, via="demod", fetch=False):
    """the three windows as IQ clients over the 25 frames: per client (iq[25][h], pwr[25], nan[25])"""
    rig = Rig(is_real, n)
    try:
        cl = [rig.add("IQ", w) for w in windows(is_real, n)]
        got = [[] for _ in cl]
        for F in batches:
            rig.batch(F, via)
            if fetch:
                rig.ctx.fetch_begin(rig.ctx.FETCH_IQ)
                rig.ctx.fetch_end()
            for k, g in enumerate(cl):
                got[k].append(rig.fetched_iq(g, F) if fetch else g.read_iq(MAXB))
        return [tuple(np.concatenate([b[i] for b in per]) for i in range(3)) for per in got]
    finally:
        rig.close()


def same_bits(a, b, tag):
    for x, y, what in zip(a, b, ("iq", "pwr", "nan flags")):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{tag}: {what} differ"


def check_iq(iq_g, bb_o, tag):
    scale = max(float(np.abs(bb_o).max()), 1e-30)
    print(f"{tag}: rel L2 {rel_l2(iq_g, bb_o):.2e}, max |d| / max |IQ| {float(np.abs(iq_g - bb_o).max()) / scale:.2e}")
    assert rel_l2(iq_g, bb_o) < 1e-4, f"{tag}: rel L2 {rel_l2(iq_g, bb_o):.2e}"
    assert np.abs(iq_g - bb_o).max() <= 2e-4 * scale, tag


# ---- 1. oracle parity ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("is_real", [0, 1])
@pytest.mark.parametrize("n", [360, 720, 256, 1024])
def test_iq_rows_equal_the_oracles_baseband(n, is_real):
    got = run_iq(is_real, n)
    for k, ((iq, pwr, nan), (bb, pw_o, fs)) in enumerate(zip(got, oracle_baseband(is_real, n))):
        assert iq.shape == (NF, n // 2) and iq.dtype == np.complex64
        assert not nan.any()
        for f in range(NF):
            tag = f"n {n} real {is_real} window {windows(is_real, n)[k]} frame {f}"
            check_iq(iq[f], bb[f], tag)
            assert abs(pwr[f] - pw_o[f]) <= pwr_tolerance(pw_o[f], fs[f]), tag


# ---- 2. bit identities -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("is_real", [0, 1])
@pytest.mark.parametrize("n", [360, 720, 256, 1024])
def test_one_frame_batches_give_the_same_bits(n, is_real):
    a, b = run_iq(is_real, n), run_iq(is_real, n, batches=(1,) * NF)
    for k in range(3):
        same_bits(a[k], b[k], f"client {k}: 19 + 1 + 5 against 25 x 1")


@pytest.mark.parametrize("n,is_real", [(360, 0), (720, 1), (360, 1), (720, 0)])
def test_chain_kernel_and_two_kernel_path_give_the_same_bits(n, is_real, monkeypatch):
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", "1")
    a = run_iq(is_real, n)
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", "0")
    b = run_iq(is_real, n)
    for k in range(3):
        same_bits(a[k], b[k], f"client {k}: PSDR_DEMOD_CHAIN=1 against 0")


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_fetched_rows_and_demod_batch_from_give_the_same_bits(n, is_real):
    a = run_iq(is_real, n)
    b = run_iq(is_real, n, fetch=True)
    c = run_iq(is_real, n, via="from")
    for k in range(3):
        same_bits(a[k], b[k], f"client {k}: psdr_read_iq against psdr_fetched_iq")
        same_bits(a[k], c[k], f"client {k}: psdr_demod_batch against psdr_demod_batch_from")


# ---- 3. continuity across mode switches -----------------------------------------------------------------------------

@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1), (720, 1)])
def test_mode_switches_continue_through_iq(n, is_real):
    """USB 3 frames -> AM 3 -> IQ 4 -> FM 3 -> USB 3, the oracle with AM in place of IQ: the IQ kernel leaves the tail and the
    last sample FM's first frame pairs with, and copies the USB tail through"""
    seq = [("USB", 3), ("AM", 3), ("IQ", 4), ("FM", 3), ("USB", 3)]
    h = n // 2
    fo, specs = oracle_spectra(is_real, n)
    wins = windows(is_real, n)[:2]
    rig = Rig(is_real, n)
    try:
        gs = [rig.add("USB", w) for w in wins]
        os_ = []
        for w in wins:
            o = O.AudioClient(bool(is_real), n, 12000, 4096)
            o.set_audio_range(*w)
            os_.append(o)
        frame = 0
        for mode, F in seq:
            for g, o in zip(gs, os_):
                g.set_audio_demodulation(mode)
                o.set_audio_demodulation("AM" if mode == "IQ" else mode)
            rig.batch(F)
            for k, (g, o) in enumerate(zip(gs, os_)):
                out, pwr, nan = g.read_iq(MAXB) if mode == "IQ" else g.read_audio(MAXB)
                assert len(out) == F and not nan.any()
                for f in range(F):
                    tag = f"n {n} real {is_real} client {k} {mode} frame {frame + f}"
                    a_o, p_o, _, dropped = o.send_audio(specs[frame + f], frame + f, fft=fo)
                    assert not dropped
                    assert abs(pwr[f] - p_o) <= pwr_tolerance(p_o, o.fwd_scale), tag
                    if mode == "IQ":
                        check_iq(out[f], o.baseband()[:h], tag)
                    elif mode == "FM":
                        check_fm(out[f], a_o, o.baseband()[:h], o.bb_prev, tag, fwd_scale=max(o.fwd_scale, o.fwd_scale_prev))
                    else:
                        scale = max(np.abs(a_o).max(), 1e-30)
                        assert rel_l2(out[f], a_o) < 1e-4, f"{tag}: rel L2 {rel_l2(out[f], a_o):.2e}"
                        assert np.abs(out[f] - a_o).max() <= 2e-4 * scale, tag
            frame += F
    finally:
        rig.close()


# ---- 4. nobody else notices -----------------------------------------------------------------------------------------

def old_mode_clients(is_real, n):
    """eight clients of the four old modes on the two carrier windows"""
    w = windows(is_real, n)
    return [(m, w[i % 2]) for i, m in enumerate(("USB", "LSB", "AM", "FM", "FM", "AM", "LSB", "USB"))]


def run_old_modes(is_real, n, with_iq):
    """19 + 1 + 5 frames with the post chain on: per old-mode client and batch (audio, pwr, nan, pcm).  with_iq: two IQ clients
    interleaved in slot order (slots 2 and 5); the second is switched back to AM for the last batch."""
    from phantomsdr_amd import PsdrError
    rig = Rig(is_real, n, max_clients=10, post=True)
    try:
        old, iqs = [], []
        specs = old_mode_clients(is_real, n)
        for i, (m, w) in enumerate(specs):
            if with_iq and i in (2, 4):  # the next free slot: 2, then 5
                iqs.append(rig.add("IQ", windows(is_real, n)[len(iqs)]))
            old.append(rig.add(m, w))
        if with_iq:
            assert [g.id for g in iqs] == [2, 5]
        res = [[] for _ in old]
        for b, F in enumerate(BATCHES):
            if with_iq and b == 2:
                iqs[1].set_audio_demodulation("AM")
            rig.batch(F)
            for k, g in enumerate(old):
                res[k].append(g.read_audio(MAXB) + (g.read_pcm(MAXB),))
            for k, g in enumerate(iqs):
                if k == 1 and b == 2:  # switched back from IQ: audio and PCM again on the next batch, no error
                    a, p, nan = g.read_audio(MAXB)
                    assert a.shape == (F, n // 2) and not nan.any() and np.abs(a).max() > 0
                    assert g.read_pcm(MAXB).shape == (F, n // 2)
                    with pytest.raises(PsdrError) as e:
                        g.read_iq(MAXB)
                    assert e.value.code == NO_DATA
                    continue
                iq, _, nan = g.read_iq(MAXB)
                assert iq.shape == (F, n // 2) and not nan.any()
                for call in (g.read_audio, g.read_pcm):
                    with pytest.raises(PsdrError) as e:
                        call(MAXB)
                    assert e.value.code == NO_DATA
            if with_iq:
                with pytest.raises(PsdrError) as e:
                    old[2].read_iq(MAXB)  # an AM client
                assert e.value.code == NO_DATA
        return res
    finally:
        rig.close()


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_other_clients_do_not_notice_iq_clients(n, is_real):
    a, b = run_old_modes(is_real, n, False), run_old_modes(is_real, n, True)
    for k, (ra, rb) in enumerate(zip(a, b)):
        for bi, (x, y) in enumerate(zip(ra, rb)):
            for u, v, what in zip(x, y, ("audio", "pwr", "nan flags", "pcm")):
                assert u.shape == v.shape and u.tobytes() == v.tobytes(), f"client {k} batch {bi}: {what} differ with IQ clients beside it"


@pytest.mark.parametrize("n,is_real", [(360, 0), (256, 1)])
def test_paused_iq_client_keeps_its_state(n, is_real):
    """paused over the one-frame batch (frame 19): frames 20..24 continue from frame 18's tail, bit for bit as in a run of
    one-frame batches paused over the same frame"""
    from phantomsdr_amd import PsdrError

    def run(batches):
        rig = Rig(is_real, n)
        try:
            g, other = rig.add("IQ", windows(is_real, n)[0]), rig.add("IQ", windows(is_real, n)[1])
            out = []
            for F in batches:
                paused = rig.frame == 19
                g.set_paused(paused)
                rig.batch(F)
                if paused:
                    with pytest.raises(PsdrError) as e:
                        g.read_iq(MAXB)
                    assert e.value.code == NO_DATA
                    other.read_iq(MAXB)
                else:
                    out.append(g.read_iq(MAXB))
            return tuple(np.concatenate([o[i] for o in out]) for i in range(3))
        finally:
            rig.close()

    a, b = run(BATCHES), run((1,) * NF)
    assert a[0].shape == (NF - 1, n // 2)
    same_bits(a, b, "paused over frame 19")
    # (and the frames after the pause are not those of a client that was never paused)
    never = run_iq(is_real, n)[0][0]
    assert a[0][:19].tobytes() == never[:19].tobytes() and a[0][19].tobytes() != never[20].tobytes()


# ---- 5. edges --------------------------------------------------------------------------------------------------------

def test_read_before_the_first_batch_and_reused_slot():
    from phantomsdr_amd import PsdrError
    n = 360
    rig = Rig(0, n)
    try:
        g = rig.add("IQ", windows(0, n)[0])
        with pytest.raises(PsdrError):  # nothing demodulated yet: an error, no fault
            g.read_iq(MAXB)
        p, q = C.c_void_p(), C.c_void_p()
        assert rig.ctx.lib.psdr_iq_device_ptr(rig.ctx.h, g.id, C.byref(p), C.byref(q)) != 0
        rig.batch(5)
        rig.ctx.fetch_begin(rig.ctx.FETCH_IQ)
        rig.ctx.fetch_end()
        iq, _, _ = g.read_iq(MAXB)
        assert rig.fetched_iq(g, 5)[0].tobytes() == iq.tobytes()
        assert rig.ctx.lib.psdr_iq_device_ptr(rig.ctx.h, g.id, C.byref(p), C.byref(q)) == 0 and p.value
        back = np.empty((5, n // 2), np.complex64)
        rig.ctx.d2h(back, p)
        assert back.tobytes() == iq.tobytes()
        # the slot handed to a new client: the previous occupant's rows are not its own
        slot = g.id
        g.on_close()
        g2 = rig.add("IQ", windows(0, n)[1])
        assert g2.id == slot
        for call in (lambda: g2.read_iq(MAXB), lambda: rig.ctx.fetched_iq(g2.id, 0)):
            with pytest.raises(PsdrError) as e:
                call()
            assert e.value.code == NO_DATA
    finally:
        rig.close()


def test_fetch_copies_only_the_span_of_iq_slots():
    n, F = 256, 5
    rig = Rig(1, n, max_clients=64)
    try:
        w = windows(1, n)
        cl = [rig.add("IQ" if i in (3, 5) else "AM", w[i % 2]) for i in range(6)]
        rig.batch(F)
        rig.ctx.fetch_begin(rig.ctx.FETCH_IQ | rig.ctx.FETCH_AUDIO)
        rig.ctx.fetch_end()
        assert rig.ctx.fetched_iq_span() == (3, 3, 3 * F * (n // 2) * 8)
        for i in (3, 5):
            assert rig.fetched_iq(cl[i], F)[0].tobytes() == cl[i].read_iq(MAXB)[0].tobytes()
        au = np.stack([rig.ctx.fetched_audio(cl[4].id, f)[0] for f in range(F)])
        assert au.tobytes() == cl[4].read_audio(MAXB)[0].tobytes()
        # a batch without an IQ client: nothing to copy
        for i in (3, 5):
            cl[i].set_audio_demodulation("FM")
        rig.batch(F)
        rig.ctx.fetch_begin(rig.ctx.FETCH_IQ)
        rig.ctx.fetch_end()
        assert rig.ctx.fetched_iq_span() == (0, 0, 0)
    finally:
        rig.close()


def test_groups_refuse_iq_clients():
    from phantomsdr_amd import Group, PsdrError
    g = Group([0], "clients", 1 << 12, False, LEVELS, audio_fft_size=360, additional_size=360, max_clients=4)
    try:
        with pytest.raises(PsdrError) as e:
            g.client_add(100, 130.0, 160, "IQ")
        assert e.value.code == UNSUPPORTED
        gid = g.client_add(100, 130.0, 160, "AM")
        assert g.lib.psdr_group_client_set_audio_demodulation(g.h, gid, 4) == UNSUPPORTED
        assert g.lib.psdr_group_client_set_audio_demodulation(g.h, gid, 3) == 0
    finally:
        g.close()

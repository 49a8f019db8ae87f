"""The per-batch tables of the squelch, the audio filter and the AGC profiles travel in one image per slot of the client
parameter ring (ParamRing::K = 8): a batch in flight keeps the settings it was planned with while the host already writes the
next batches' images, and the ring wraps onto images the device has read.

One configuration, the smallest the library accepts: a 2^12-point IQ context, audio_fft_size 360, max_batch 2, three client
slots, post chain on - a squelch client in slot 0, a client with a one-section audio filter in slot 1 and a client on a manual-gain
AGC profile in slot 2.  2 K + 4 = 20 batches of 2 frames; before each one the squelch thresholds, the filter's section and the
manual gain change to values drawn from a fixed seed.  The batches run twice over the same input and settings: enqueued back to
back, the results collected by fetches that lag two batches behind (no drain anywhere), and with a drain behind every batch.
PCM, float audio, squelch flags and the carried AGC gain are the same bits in both, for every batch.  psdr_read_agc_gain
synchronises, so the undrained gain behind batch b comes from an undrained run of its own that ends with batch b.

The input's level alternates by 20 dB every three half-frames and the thresholds are drawn around the middle between the two
levels' pwr (measured once, on a context without any of the features), so the squelch opens on some frames and closes on others."""
import ctypes as C

import numpy as np
import pytest

import agc_profile_model as M

pytestmark = pytest.mark.gpu

RING_K = 8  # ParamRing::K (phantomsdr_amd/csrc/ctx.h)
BATCH, NBATCH, SLOTS = 2, 2 * RING_K + 4, 3
FRAMES = BATCH * NBATCH
LAG = 2  # fetches in flight behind the newest batch (PSDR_FETCH_SETS = 4 holds them)


def raw_stream(seed=11):
    """s16 IQ noise, loud and 20 dB quieter in turns of three half-frames (not a multiple of the batch)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((FRAMES + 1, M.N // 2, 2))
    for hf in range(FRAMES + 1):
        x[hf] *= 1500.0 if (hf // 3) % 2 == 0 else 150.0
    return np.clip(np.round(x), -32768, 32767).astype(np.int16).reshape(-1)


class Run:
    def __init__(self, raw):
        from phantomsdr_amd import AudioClient, Context
        self.ctx = Context(M.N, False, M.LEVELS, additional_size=M.AUDIO_N, audio_fft_size=M.AUDIO_N, audio_rate=M.RATE, input_format="s16",
                           max_batch=BATCH, max_clients=SLOTS)
        self.ctx.set_post_chain(True)
        self.d = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.d, raw)
        self.cl = [AudioClient(self.ctx) for _ in range(SLOTS)]
        assert [g.id for g in self.cl] == list(range(SLOTS))
        for k, g in enumerate(self.cl):
            g.set_audio_demodulation("USB")
            g.set_audio_range(*M.window(k))

    def apply(self, s):
        """one batch's settings: (open_db, close_db, section, manual_gain)"""
        self.cl[0].set_squelch(True, open_db=s[0], close_db=s[1])
        self.cl[1].set_audio_filter([s[2]])
        self.cl[2].set_agc_profile("reference", manual=True, manual_gain=s[3])

    def enqueue(self, b):
        self.ctx.process_batch(self.d, BATCH, offset_bytes=b * BATCH * self.ctx.half_frame_bytes())
        self.ctx.demod_batch(b * BATCH)

    def ptrs(self, name):
        out = (C.c_void_p * 2)()
        fn = getattr(self.ctx.lib, name)
        fn.argtypes = [C.c_void_p, C.c_void_p]
        assert fn(self.ctx.h, out) == 0
        return out[0] or 0, out[1] or 0

    def tables(self):
        """(the audio filter's table, its state, the AGC profiles' table) as integers, 0 = null"""
        return self.ptrs("psdr_debug_audio_filter_ptrs") + self.ptrs("psdr_debug_agc_profile_ptrs")[:1]

    def gains(self):
        return np.array([g.read_agc_gain() for g in self.cl], np.float32)

    def close(self):
        self.ctx.dev_free(self.d)
        self.ctx.close()


@pytest.fixture(scope="module")
def raw():
    return raw_stream()


@pytest.fixture(scope="module")
def settings(raw):
    """the 20 batches' settings, from a fixed seed; the thresholds around the middle of the input's two levels and the manual gain
    scaled to the rows' peak, both read from one plain run"""
    from phantomsdr_amd import design_audio_filter
    r = Run(raw)
    try:
        pwr, peak = [], 0.0
        for b in range(NBATCH):
            r.enqueue(b)
            pwr.append(r.cl[0].read_audio()[1].copy())
            peak = max(peak, float(np.abs(r.cl[2].read_audio()[0]).max()))
    finally:
        r.close()
    db = 10 * np.log10(np.concatenate(pwr))
    assert db.max() - db.min() > 15, "the input's two levels do not show in pwr"
    mid = (db.max() + db.min()) / 2
    rng = np.random.default_rng(3)
    out = []
    for _ in range(NBATCH):
        open_db = mid + rng.uniform(-3, 3)
        out.append((open_db, open_db - rng.uniform(0, 3), design_audio_filter(("lowpass", "highpass", "peak")[rng.integers(3)], M.RATE, rng.uniform(300, 3000)),
                    rng.uniform(0.05, 0.5) / peak))
    return out


def collect(r, out):
    """the batch the last fetch_end completed: per slot the audio and PCM rows, and slot 0's squelch flags"""
    rows = [[r.ctx.fetched_audio(s, f, pcm=True) for f in range(BATCH)] for s in range(SLOTS)]
    out["audio"].append(np.array([[fr[0] for fr in slot] for slot in rows]))
    out["nan"].append(np.array([[fr[2] for fr in slot] for slot in rows]))
    out["pcm"].append(np.array([[fr[3] for fr in slot] for slot in rows]))
    out["open"].append(np.array([r.ctx.fetched_squelch(0, f) for f in range(BATCH)]))


def undrained(raw, settings, nb, fetch):
    """batches 0 .. nb - 1 back to back; fetch: their results through fetches LAG batches behind -> (results, gains behind the last)"""
    r = Run(raw)
    out = dict(audio=[], nan=[], pcm=[], open=[])
    try:
        for b in range(nb):
            r.apply(settings[b])
            r.enqueue(b)
            if fetch:
                r.ctx.fetch_begin(r.ctx.FETCH_AUDIO | r.ctx.FETCH_PCM)
                if b >= LAG:
                    r.ctx.fetch_end()
                    collect(r, out)
        for _ in range(min(LAG, nb) if fetch else 0):
            r.ctx.fetch_end()
            collect(r, out)
        return out, r.gains()
    finally:
        r.close()


def test_batches_in_flight_keep_their_tables(raw, settings):
    got, last_gains = undrained(raw, settings, NBATCH, True)
    assert len(got["pcm"]) == NBATCH
    r = Run(raw)
    try:
        assert r.tables() == (0, 0, 0), "a table before the first setter"
        first = None
        for b in range(NBATCH):
            r.apply(settings[b])
            if first is None:
                first = r.tables()
                assert all(first), "no table behind the first setter"
            r.enqueue(b)
            r.ctx.synchronize()
            for s in range(SLOTS):
                audio, _, nan = r.cl[s].read_audio()
                pcm = r.cl[s].read_pcm()
                assert np.array_equal(audio.view(np.uint32), got["audio"][b][s].view(np.uint32)), f"batch {b} slot {s}: float audio"
                assert np.array_equal(nan, got["nan"][b][s]) and not nan.any(), f"batch {b} slot {s}: NaN flags"
                assert np.array_equal(pcm, got["pcm"][b][s]), f"batch {b} slot {s}: PCM"
            assert np.array_equal(r.cl[0].read_squelch(), got["open"][b]), f"batch {b}: squelch flags"
            gains = r.gains()
            want = last_gains if b == NBATCH - 1 else undrained(raw, settings, b + 1, False)[1]
            assert np.array_equal(gains.view(np.uint32), want.view(np.uint32)), f"batch {b}: psdr_read_agc_gain {gains} != {want}"
            assert r.tables() == first, f"batch {b}: a table moved"
        # a second client's first use of each feature finds the tables there
        r.cl[0].set_audio_filter([settings[0][2]])
        r.cl[1].set_agc_profile("fast")
        assert r.tables() == first, "a second client's first use allocated again"
    finally:
        r.close()
    flags = np.concatenate(got["open"])
    print("squelch flags", flags.tolist())
    assert 0 < flags.sum() < flags.size, "the squelch flags are constant: the thresholds do not act"
    pcm = np.concatenate(got["pcm"], axis=1)  # [slot][frame][h]
    print("PCM peak per slot", np.abs(pcm).max(axis=(1, 2)).tolist(), "saturated", (np.abs(pcm) >= 32767).mean(axis=(1, 2)).tolist())
    for s in range(SLOTS):  # (the AGC's look-ahead of 2400 samples is silent, and the squelch client's stream is its open frames only)
        assert np.count_nonzero(pcm[s]) > M.H, f"slot {s}: the PCM is almost all zeros"
    assert (np.abs(pcm[2]) >= 32767).mean() < 0.5, "the manual-gain client's PCM is saturated: the gain does not show"

"""Per-client AGC profiles in the post chain (include/psdr.h: psdr_client_set_agc_profile) on the GPU, bit for bit.

One configuration throughout (tests/agc_profile_model.py): a 2^12-point IQ context, 12 kHz audio in frames of 180 samples (L =
2400, D = 32), 80 slots with USB clients in slots 0, 1, 63, 64 and 79 - a boundary between two groups of 64 slots and a partly
filled group -, 48 frames of noise whose level rises by 20 dB in the middle.  The GPU's own float audio rows are the input of the
expectation, as in test_gpu_post_chain_forms.py: through the oracle library's DC blocker, then either its AGC built with the
profile's numbers (profiles the oracle can express) or the host program over agcplan.h that test_agc_profile_host.py pins to that
AGC (cap, manual gain, a change in mid-stream), then its int16 conversion.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import agc_profile_model as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

FORMS = {"one-kernel": 1, "five-kernel": 0}
FRAMES_SPEC = 48
FIVE = [M.profile(attack_ms=5.0, release_ms=100.0), M.REFERENCE, M.profile(release_ms=2000.0), M.profile(desired=0.05), M.profile(desired=0.5, attack_ms=5.0, release_ms=100.0)]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_agc_profile")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


@pytest.fixture(scope="module")
def raw():
    return M.raw_stream()


class Run:
    """one context with the five clients; batch() runs one batch and collects every client's audio and PCM rows"""

    def __init__(self, raw, form=1, pcm16=False, batch=16):
        from phantomsdr_amd import AudioClient, Context
        self.ctx = Context(M.N, False, M.LEVELS, additional_size=M.AUDIO_N, audio_fft_size=M.AUDIO_N, audio_rate=M.RATE, input_format="s16",
                           max_batch=batch, max_clients=M.MAX_CLIENTS)
        self.ctx.set_option(self.ctx.OPT_POST_CHAIN_AGC, form)
        if pcm16:
            self.ctx.set_option(self.ctx.OPT_POST_CHAIN_PCM16, 1)
        self.ctx.set_post_chain(True)
        self.d = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.d, raw)
        everyone = [AudioClient(self.ctx) for _ in range(M.MAX_CLIENTS)]
        for g in everyone:
            if g.id not in M.SLOTS:
                g.on_close()
        self.cl = {s: everyone[s] for s in M.SLOTS}
        for k, s in enumerate(M.SLOTS):
            self.cl[s].set_audio_demodulation("USB")
            self.cl[s].set_audio_range(*M.window(k))
        self.f0 = 0
        self.audio = {s: [] for s in M.SLOTS}
        self.pcm = {s: [] for s in M.SLOTS}

    def batch(self, nb, read=None, collect=True):
        self.ctx.process_batch(self.d, nb, offset_bytes=self.f0 * self.ctx.half_frame_bytes())
        self.ctx.demod_batch(self.f0)
        self.f0 += nb
        if not collect:
            return
        for s in (M.SLOTS if read is None else read):
            a, _, nan = self.cl[s].read_audio()
            assert not nan.any()
            self.audio[s].append(a.copy())
            self.pcm[s].append(self.cl[s].read_pcm().copy())

    def batch_from(self, spec, read):
        """one batch demodulated from the caller's spectra [nb][N] complex64 (psdr_demod_batch_from): the way to hand a client
        non-finite bins"""
        nb = spec.shape[0]
        d = self.ctx.dev_alloc(spec.nbytes)
        try:
            self.ctx.h2d(d, np.ascontiguousarray(spec))
            rc = self.ctx.lib.psdr_demod_batch_from(self.ctx.h, d, M.N, nb, self.f0)
            assert rc == 0, self.ctx.lib.psdr_last_error()
            self.ctx.last_demod_frames = nb
            self.f0 += nb
            flags = {}
            for s in read:
                a, _, nan = self.cl[s].read_audio()
                flags[s] = nan.copy()
                self.audio[s].append(a.copy())
                self.pcm[s].append(self.cl[s].read_pcm().copy())
            return flags
        finally:
            self.ctx.synchronize()
            self.ctx.dev_free(d)

    def table_ptrs(self):
        """(the context's profile table, PostArgs::agc_tab of the last chain batch) as integers, 0 = null"""
        out = (C.c_void_p * 2)()
        self.ctx.lib.psdr_debug_agc_profile_ptrs.argtypes = [C.c_void_p, C.c_void_p]
        assert self.ctx.lib.psdr_debug_agc_profile_ptrs(self.ctx.h, out) == 0
        return out[0] or 0, out[1] or 0

    def rows(self, s):
        return np.concatenate(self.audio[s]), np.concatenate(self.pcm[s])

    def close(self):
        self.ctx.dev_free(self.d)
        self.ctx.close()


def run_plain(raw, profiles, form=1, pcm16=False, splits=(16, 16, 16), changes=None, read_gains=True):
    """profiles: {slot: profile} set before the first batch; changes: {batch index: {slot: profile or None}} set in front of
    that batch -> ({slot: (audio, pcm)}, {slot: [carried gain behind each batch]} - empty lists with read_gains = False)"""
    r = Run(raw, form, pcm16, batch=max(splits))
    try:
        for s, p in profiles.items():
            r.cl[s].set_agc_profile(p)
        gains = {s: [] for s in M.SLOTS}
        for b, nb in enumerate(splits):
            for s, p in (changes or {}).get(b, {}).items():
                r.cl[s].set_agc_profile(p)
            r.batch(nb)
            if read_gains:
                for s in M.SLOTS:
                    gains[s].append(r.cl[s].read_agc_gain())
        return {s: r.rows(s) for s in M.SLOTS}, gains
    finally:
        r.close()


@pytest.fixture(scope="module")
def plain(raw):
    """the context without the feature call, once: every client on the context's AGC"""
    return run_plain(raw, {})[0]


def assert_pcm(got, want, tag):
    want = want.reshape(got.shape)
    assert np.count_nonzero(want) > 1000, f"{tag}: the expectation is almost all zeros"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{tag}: {len(bad)} samples differ, first at frame {bad[0][0]} sample {bad[0][1]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


@pytest.mark.parametrize("pcm16", [False, True], ids=["int32", "pcm16"])
@pytest.mark.parametrize("form", list(FORMS))
def test_profiles_against_the_oracle(raw, form, pcm16):
    """five different uncapped, non-manual profiles, one of them the reference's: PCM bit for bit the oracle's chain with
    orc_agc_create(profile)"""
    got, _ = run_plain(raw, dict(zip(M.SLOTS, FIVE)), FORMS[form], pcm16)
    seen = set()
    for s, p in zip(M.SLOTS, FIVE):
        audio, pcm = got[s]
        assert_pcm(pcm, M.oracle_chain(audio, p), f"slot {s} {form}")
        seen.add(pcm.tobytes())
    assert len(seen) == len(FIVE), "two different profiles gave the same PCM: the profiles do not act"


MANUAL_CAP = {0: M.profile(manual=1, manual_gain=2.5, attack_ms=5.0, release_ms=100.0), 1: M.profile(max_gain=1.5), 63: M.profile(manual=1, manual_gain=0.0),
              64: M.profile(max_gain=400.0, attack_ms=5.0, release_ms=100.0), 79: M.profile(manual=1, manual_gain=40.0, desired=0.7)}


@pytest.mark.parametrize("form", list(FORMS))
def test_manual_and_cap_against_the_table_program(raw, exe, tmp, form):
    got, gains = run_plain(raw, MANUAL_CAP, FORMS[form])
    jobs = [(M.dc_block(got[s][0]), [(got[s][0].size, 0, MANUAL_CAP[s])]) for s in M.SLOTS]
    for s, (y, g) in zip(M.SLOTS, M.model_runs(exe, tmp, jobs, tag="mc" + form)):
        if MANUAL_CAP[s]["manual_gain"] != 0.0 or not MANUAL_CAP[s]["manual"]:
            assert_pcm(got[s][1], M.to_int16(y), f"slot {s} {form}")
        else:
            assert np.array_equal(got[s][1].reshape(-1), M.to_int16(y)) and not got[s][1].any(), "manual gain 0: silence"
        for b in range(3):
            assert gains[s][b].view(np.uint32) == g[(b + 1) * 16 * M.H - 1].view(np.uint32), f"slot {s} batch {b}: psdr_read_agc_gain is not the model's carried gain"
    assert got[1][1].tobytes() != got[64][1].tobytes()


def test_no_effect_elsewhere(raw, plain):
    """profiles on slots 1 and 64 only: slots 0, 63 and 79 are a context's without the feature call; and the reference-valued
    profile is no profile"""
    got, _ = run_plain(raw, {1: M.profile(attack_ms=5.0, release_ms=100.0, max_gain=3.0), 64: M.profile(manual=1, manual_gain=7.0)})
    for s in (0, 63, 79):
        assert np.array_equal(got[s][0], plain[s][0]) and np.array_equal(got[s][1], plain[s][1]), f"slot {s} changed beside a client with a profile"
    for s in (1, 64):
        assert not np.array_equal(got[s][1], plain[s][1])
    ref, _ = run_plain(raw, {s: M.REFERENCE for s in M.SLOTS})
    for s in M.SLOTS:
        assert np.array_equal(ref[s][1], plain[s][1]), f"slot {s}: the reference-valued profile differs from no profile"
        assert np.count_nonzero(plain[s][1]) > 1000


@pytest.mark.parametrize("form", list(FORMS))
def test_batch_splits_and_the_timing_of_a_change(raw, exe, tmp, form):
    """a profile set between batches 0 and 1 (of 3 x 16) shows from batch 1 on and not earlier; the gain is continuous across the
    change (the model starts the new profile from the old gain); the same PCM however the 48 frames are split"""
    first = {0: FIVE[0], 64: M.profile(max_gain=2.0)}
    change = {1: {0: M.profile(manual=1, manual_gain=1.25, attack_ms=5.0, release_ms=100.0), 1: FIVE[2], 64: None}}
    got, gains = run_plain(raw, first, FORMS[form], changes=change)
    T1 = 16 * M.H
    segs = {0: [(T1, 0, first[0]), (2 * T1, 0, change[1][0])], 1: [(T1, 0, None), (2 * T1, 0, change[1][1])], 64: [(T1, 0, first[64]), (2 * T1, 0, None)],
            63: [(3 * T1, 0, None)], 79: [(3 * T1, 0, None)]}
    jobs = [(M.dc_block(got[s][0]), segs[s]) for s in M.SLOTS]
    model = dict(zip(M.SLOTS, M.model_runs(exe, tmp, jobs, tag="ch" + form)))
    for s in M.SLOTS:
        assert_pcm(got[s][1], M.to_int16(model[s][0]), f"slot {s} {form}")
        for b in range(3):
            assert gains[s][b].view(np.uint32) == model[s][1][(b + 1) * T1 - 1].view(np.uint32), (s, b)
    # not earlier: batch 0 is what the unchanged profiles give; and from batch 1 on: it differs from them
    same, _ = run_plain(raw, first, FORMS[form], splits=(16,))
    for s in M.SLOTS:
        assert np.array_equal(same[s][1], got[s][1][:16]), f"slot {s}: the change shows in the batch before it"
    # 48 x 1 with the same change in front of frame 16 ...
    other, _ = run_plain(raw, first, FORMS[form], splits=(1,) * 48, changes={16: change[1]}, read_gains=False)
    for s in M.SLOTS:
        assert np.array_equal(other[s][1], got[s][1]), f"slot {s}: 48 x 1 differs from 3 x 16"
    # ... 1 x 48 against 3 x 16 (one batch cannot hold a change: five fixed profiles) ...
    whole, _ = run_plain(raw, dict(zip(M.SLOTS, FIVE)), FORMS[form], splits=(48,))
    parts, _ = run_plain(raw, dict(zip(M.SLOTS, FIVE)), FORMS[form])
    for s in M.SLOTS:
        assert np.array_equal(whole[s][1], parts[s][1]), f"slot {s}: 1 x 48 differs from 3 x 16"
    # ... and 3 x 16 with the fetches lagging three batches
    r = Run(raw, FORMS[form])
    try:
        for s, p in first.items():
            r.cl[s].set_agc_profile(p)
        for b in range(3):
            for s, p in change.get(b, {}).items():
                r.cl[s].set_agc_profile(p)
            r.batch(16, collect=False)
            r.ctx.fetch_begin(r.ctx.FETCH_PCM)
        for b in range(3):
            r.ctx.fetch_end()
            for s in M.SLOTS:
                for f in range(16):
                    assert np.array_equal(r.ctx.fetched_audio(s, f, pcm=True)[3], got[s][1][16 * b + f]), f"slot {s} batch {b} frame {f}: the lagging fetch"
    finally:
        r.close()


def test_state_is_kept(raw, exe, tmp):
    """a mode change still resets the AGC (and a profile survives it); a paused client, and a profile change while paused, freeze
    the gain (a squelch-closed and an all-NaN batch: test_a_dropped_batch_freezes_the_gain)"""
    r = Run(raw, 1)
    try:
        p = M.profile(attack_ms=5.0, release_ms=100.0, max_gain=30.0)
        r.cl[1].set_agc_profile(p)
        r.batch(16)
        g1 = r.cl[1].read_agc_gain()
        r.cl[1].set_paused(True)
        r.cl[1].set_agc_profile(M.profile(manual=1, manual_gain=9.0))
        r.batch(16, read=(0, 63, 64, 79))
        assert r.cl[1].read_agc_gain().view(np.uint32) == g1.view(np.uint32), "a paused client's gain moved"
        r.cl[1].set_paused(False)
        r.cl[1].set_agc_profile(p)
        r.cl[63].set_agc_profile(FIVE[0])
        r.cl[63].set_audio_demodulation("LSB")  # AGC::reset, at the next batch; the profile stays
        r.f0 = 16
        r.batch(16)
        a1, pcm1 = r.rows(1)
        (y, g), = M.model_runs(exe, tmp, [(M.dc_block(a1), [(a1.size, 0, p)])], tag="pause")
        assert_pcm(pcm1, M.to_int16(y), "slot 1 across a pause")
        assert r.cl[1].read_agc_gain().view(np.uint32) == g[-1].view(np.uint32)
        # slot 63: the third batch starts from AGC::reset - zeros while the look-ahead fills again (13 frames and a part)
        pcm63 = r.pcm[63][-1]
        assert not pcm63[: (M.L - 1) // M.H].any() and pcm63[-1].any(), "the mode change did not reset the AGC"
    finally:
        r.close()


def noise_spectra(frames=FRAMES_SPEC, seed=9):
    """spectra for psdr_demod_batch_from: complex noise whose level rises by 20 dB in the middle"""
    rng = np.random.default_rng(seed)
    x = ((rng.standard_normal((frames, M.N)) + 1j * rng.standard_normal((frames, M.N))) * 1e-3).astype(np.complex64)
    x[frames // 2:] *= np.float32(10)
    return x


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind", ["squelch-closed", "all-NaN"])
def test_a_dropped_batch_freezes_the_gain(raw, exe, tmp, kind, form):
    """a batch in which every frame of a client with a profile is dropped - closed by its squelch, or flagged by the NaN guard -
    is an empty stream: a listed client with a table entry and T = 0.  The carried gain is bit for bit what it was, the batch's
    PCM is zero, and the PCM behind it follows the model over the client's surviving frames; the neighbour in the same
    work-group, on another profile, runs through all three batches"""
    p, q = M.profile(attack_ms=5.0, release_ms=100.0, max_gain=30.0), FIVE[2]
    spec = noise_spectra()
    r = Run(raw, FORMS[form])
    try:
        r.cl[1].set_agc_profile(p)
        r.cl[0].set_agc_profile(q)
        flags = r.batch_from(spec[:16], read=(0, 1))
        assert not flags[0].any() and not flags[1].any()
        g1 = r.cl[1].read_agc_gain()
        assert g1 > 0
        bad = spec[16:32].copy()
        if kind == "all-NaN":
            bad[:, M.window(1)[0] + 30] = np.nan  # a bin of client 1's window alone, in every frame
        else:
            r.cl[1].set_squelch(True, open_db=300.0)  # never opens
        flags = r.batch_from(bad, read=(0, 1))
        assert not flags[0].any(), "the neighbour lost frames"
        if kind == "all-NaN":
            assert flags[1].all(), "not every frame of the batch was flagged"
        else:
            assert not flags[1].any() and not r.cl[1].read_squelch().any(), "the squelch opened"
            r.cl[1].set_squelch(False)
        assert not r.pcm[1][-1].any(), "PCM behind dropped frames"
        assert r.cl[1].read_agc_gain().view(np.uint32) == g1.view(np.uint32), "the gain moved across an empty stream"
        assert r.table_ptrs()[1] != 0, "the batch ran without the table"
        flags = r.batch_from(spec[32:48], read=(0, 1))
        assert not flags[0].any() and not flags[1].any(), "a frame behind the dropped batch was dropped too"
        kept = np.concatenate([r.audio[1][0], r.audio[1][2]])
        a0 = np.concatenate(r.audio[0])
        (y1, gm1), (y0, gm0) = M.model_runs(exe, tmp, [(M.dc_block(kept), [(kept.size, 0, p)]), (M.dc_block(a0), [(a0.size, 0, q)])], tag="drop" + kind + form)
        assert_pcm(np.concatenate([r.pcm[1][0], r.pcm[1][2]]), M.to_int16(y1), f"slot 1 around a {kind} batch")
        assert_pcm(np.concatenate(r.pcm[0]), M.to_int16(y0), "slot 0, the neighbour")
        assert g1.view(np.uint32) == gm1[16 * M.H - 1].view(np.uint32)
        assert r.cl[1].read_agc_gain().view(np.uint32) == gm1[-1].view(np.uint32) and r.cl[0].read_agc_gain().view(np.uint32) == gm0[-1].view(np.uint32)
    finally:
        r.close()


def test_the_table_exists_and_travels_only_when_needed(raw):
    """a context without a profile allocates no table and hands the chain a null pointer; with one, the batch gets the table
    only while a client with a profile has a stream in it - not while that client is paused or an IQ client"""
    r = Run(raw, 1)
    try:
        r.batch(4, collect=False)
        assert r.table_ptrs() == (0, 0), "a context that never had a profile has a table"
        r.cl[64].set_agc_profile(None)
        r.batch(4, collect=False)
        assert r.table_ptrs() == (0, 0), "clearing a profile that was never set allocated the table"
        r.cl[64].set_agc_profile("fast")
        tab = r.table_ptrs()[0]
        assert tab != 0
        r.batch(4, collect=False)
        assert r.table_ptrs()[0] == tab and r.table_ptrs()[1] != 0
        r.cl[64].set_paused(True)
        r.batch(4, collect=False)
        assert r.table_ptrs() == (tab, 0), "a batch whose only client with a profile is paused got the table"
        r.cl[64].set_paused(False)
        r.cl[64].set_audio_demodulation("IQ")
        r.batch(4, collect=False)
        assert r.table_ptrs() == (tab, 0), "a batch whose only client with a profile is an IQ client got the table"
        r.cl[64].set_audio_demodulation("USB")
        r.batch(4, collect=False)
        assert r.table_ptrs()[1] != 0
        r.cl[64].set_agc_profile(None)
        r.batch(4, collect=False)
        assert r.table_ptrs() == (tab, 0), "the table travels though no client has a profile any more"
    finally:
        r.close()


def test_errors_and_iq(raw):
    from phantomsdr_amd import PsdrError, _lib
    r = Run(raw, 1)
    try:
        lib, h = r.ctx.lib, r.ctx.h
        good = _lib.psdr_agc_profile(0.2, 50.0, 300.0, 0.0, 0, 0.0)
        rc = lib.psdr_client_set_agc_profile(h, 5, C.byref(good))
        assert rc != 0, "an unknown id was accepted"
        INVALID = rc
        for bad in ((float("nan"), 50, 300, 0, 0, 0), (0, 50, 300, 0, 0, 0), (0.2, 0, 300, 0, 0, 0), (0.2, 50, 20000, 0, 0, 0), (0.2, 50, 300, -1, 0, 0),
                    (0.2, 50, 300, 0, 2, 0), (0.2, 50, 300, 0, 1, -1), (0.2, 300, 50, 0, 0, 0)):
            p = _lib.psdr_agc_profile(*[float(v) if k != 4 else int(v) for k, v in enumerate(bad)])
            assert lib.psdr_client_set_agc_profile(h, 0, C.byref(p)) == INVALID, bad
            with pytest.raises(PsdrError):
                r.cl[0].set_agc_profile(dict(desired=bad[0], attack_ms=bad[1], release_ms=bad[2], max_gain=bad[3], manual=bad[4], manual_gain=bad[5]))
        g = C.c_float(0)
        assert lib.psdr_read_agc_gain(h, 0, C.byref(g)) not in (0, INVALID), "a client no chain batch has listed has no gain to read"
        assert lib.psdr_read_agc_gain(h, 5, C.byref(g)) == INVALID
        # an IQ client keeps its profile and gets it back on return to USB (a fresh client: its chain starts with its first USB batch)
        p = FIVE[0]
        r.cl[0].set_agc_profile(p)
        r.cl[0].set_audio_demodulation("IQ")
        r.batch(16, read=(1,))
        r.cl[0].set_audio_demodulation("USB")
        r.batch(16, read=(0,))
        r.batch(16, read=(0,))
        a0, pcm0 = r.rows(0)
        assert a0.shape[0] == 32
        assert_pcm(pcm0, M.oracle_chain(a0, p), "slot 0 back from IQ")
        assert not np.array_equal(pcm0, M.oracle_chain(a0, M.REFERENCE).reshape(pcm0.shape))
        r.cl[0].set_agc_profile(None)
    finally:
        r.close()

"""Per-client squelch on the GPU (include/psdr.h: psdr_client_set_squelch, psdr_read_squelch, psdr_fetched_squelch).

Expected flags come from tests/squelch_model.py, fed the GPU's own pwr bits: there is no tolerance anywhere.  What the model
is fed is checked too: every expected sequence must hold an opening, a closing, a gap shorter than the hang (bridged), a burst
shorter than the attack (rejected) and a NaN frame - a condition on the input, not on the code.

Input: unit noise plus two tones inside every client's window, keyed by half-frames (a frame is two half-frames: both keyed =
"full", one = "half").  With the CPU oracle's pwr of these streams (all three shapes, both audio sizes, every mode the same -
pwr is the window's power): full -1.0 .. -1.3 dB, half -4.0 .. -4.4 dB, noise below -16 dB.  The thresholds sit between
them with more than 1 dB on either side: OPEN_DB between half and full, CLOSE_DB between noise and half."""
import functools

import numpy as np
import pytest

import squelch_model as M
from helpers import CLIENT_KINDS, assert_same_bits, read_client, row_names, set_client_kind

pytestmark = pytest.mark.gpu

LEVELS, RATE, MAXB = 4, 12000, 8
KINDS = tuple(CLIENT_KINDS)
OPEN_DB, CLOSE_DB, ATTACK, HANG = -2.7, -10.0, 2, 2
STD = (OPEN_DB, CLOSE_DB, ATTACK, HANG)
# half-frames 0..32 of the 32-frame script.  Frames: 3 full alone (a burst shorter than the attack), 9..13 full (opens at 10),
# 14 half / 15 noise / 16 half (a gap shorter than the hang), 17..20 full, 21 half, 22.. noise (closes at 24), 26..30 full
KEY = [0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0]
NAN_HALF = 19  # one NaN sample: frames 18 and 19 are NaN, inside an open stretch
NF = len(KEY) - 1
SPLITS = {"8": (8,), "1+7": (1, 7), "3+5": (3, 5), "1x8": (1,) * 8}
SHAPES = {"iq": (False, 1 << 14, 5000), "real": (True, 1 << 15, 5000), "iq12": (False, 1 << 12, 1000)}
EVENTS = {"opening", "closing", "bridged", "rejected", "nan"}


@functools.lru_cache(maxsize=None)
def stream(shape, key=tuple(KEY), nan_half=NAN_HALF, seed=5):
    """f32 half-frames, flat: unit noise plus the keyed tones on client bins L0 + 30 and L0 + 70"""
    is_real, N, L0 = SHAPES[shape]
    rng = np.random.default_rng(seed)
    ns = len(key) * (N // 2)
    t = np.arange(ns, dtype=np.float64)
    gate = np.repeat(np.asarray(key, np.float64), N // 2)
    if is_real:
        x = rng.standard_normal(ns)
        for k in (L0 + 30, L0 + 70):
            x += gate * 2.0 * np.cos(2 * np.pi * k * t / N)
        raw = x.astype(np.float32)
        if nan_half is not None:
            raw[nan_half * (N // 2) + 17] = np.nan
        return raw
    x = rng.standard_normal(ns) + 1j * rng.standard_normal(ns)
    for k in (L0 + 30, L0 + 70):  # client bin c of an IQ spectrum is frequency index (c + N/2 + 1) mod N
        x += gate * np.exp(2j * np.pi * ((k + N // 2 + 1) % N) * t / N)
    raw = x.astype(np.complex64).view(np.float32).copy()
    if nan_half is not None:
        raw[2 * (nan_half * (N // 2) + 17)] = np.nan
    return raw


def window(shape):
    L0 = SHAPES[shape][2]
    return (L0, L0 + 50.3, L0 + 100)


class Ctx:
    def __init__(self, shape, n, max_clients, maxb=MAXB, post=False, agc=1, pcm16=0, raw=None, rate=RATE):
        from phantomsdr_amd import Context
        is_real, N, _ = SHAPES[shape]
        self.shape, self.n = shape, n
        self.ctx = Context(N, is_real, LEVELS, additional_size=n, audio_fft_size=n, audio_rate=rate, input_format="f32", max_batch=maxb,
                           max_clients=max_clients)
        raw = stream(shape) if raw is None else raw
        self.d = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.d, raw)
        if post:
            self.ctx.set_option(self.ctx.OPT_POST_CHAIN_AGC, agc)
            self.ctx.set_option(self.ctx.OPT_POST_CHAIN_PCM16, pcm16)
            self.ctx.set_post_chain(True)
        self.frame = 0

    def add(self, kind, squelch=None):
        from phantomsdr_amd import AudioClient
        g = AudioClient(self.ctx)
        set_client_kind(g, kind)
        g.set_audio_range(*window(self.shape))
        if squelch is not None:
            g.set_squelch(True, *squelch)
        return g

    def batch(self, F):
        self.ctx.process_batch(self.d, F, offset_bytes=self.frame * self.ctx.half_frame_bytes())
        self.ctx.demod_batch(self.frame)
        self.frame += F

    def close(self):
        self.ctx.dev_free(self.d)
        self.ctx.close()


class Gate:
    """the model's side of one client: settings, carried state, on / paused"""

    def __init__(self, params=None):
        self.on, self.params, self.state, self.paused = params is not None, params, (0, 0), False

    def set(self, on, params=None):
        if on and not self.on:
            self.state = (0, 0)  # switched on: from (closed, 0)
        self.on = on
        if on:
            self.params = params

    def batch(self, pwr):
        if not self.on:
            return np.ones(len(pwr), np.int32)
        o, c, a, h = self.params
        flags, self.state = M.run(pwr, M.threshold(o), M.threshold(c), a, h, self.state)
        return flags


# the three extra clients of the flags test and what happens to them at a frame boundary (a multiple of 8: every split has it)
T_NEW = (OPEN_DB, OPEN_DB, 1, 5)
EXTRAS = (("P", "USB"), ("R", "AM"), ("T", "FM"))


def act(at, gp, gates, twins):
    """P sits out frames 16..23 with the gate open and a below-frame counted; R is off for them and on again at 24; T gets new
    thresholds and counts at 16"""
    g = dict(zip((k for k, _ in EXTRAS), gp))
    if at == 16:
        g["P"].set_paused(True), twins["P"].set_paused(True)
        gates["P"].paused = True
        g["R"].set_squelch(False)
        gates["R"].set(False)
        g["T"].set_squelch(True, *T_NEW)
        gates["T"].set(True, T_NEW)
    if at == 24:
        g["P"].set_paused(False), twins["P"].set_paused(False)
        gates["P"].paused = False
        g["R"].set_squelch(True, *STD)
        gates["R"].set(True, STD)


@functools.lru_cache(maxsize=None)
def flags_run(shape, n, split):
    """every kind and the three extras with squelch in context A, the same clients without in context B, the 32 frames in
    batches of `split` (repeated); -> per client name: (got flags, want flags, pwr, A's rows == B's rows message or None)"""
    from phantomsdr_amd import PsdrError
    names = list(KINDS) + [k for k, _ in EXTRAS]
    kinds = list(KINDS) + [k for _, k in EXTRAS]
    A, B = Ctx(shape, n, len(names) + 1), Ctx(shape, n, len(names) + 1)
    try:
        ga = [A.add(k, STD) for k in kinds]
        gb = [B.add(k) for k in kinds]
        gates = {nm: Gate(STD) for nm in names}
        twins = dict(zip(names, gb))
        out = {nm: dict(got=[], want=[], pwr=[], frames=[], diff=[]) for nm in names}
        sizes = SPLITS[split] * (NF // 8)
        at = 0
        for F in sizes:
            if at % 8 == 0:
                act(at, ga[len(KINDS):], gates, twins)
            A.batch(F), B.batch(F)
            for nm, kind, g, h in zip(names, kinds, ga, gb):
                o = out[nm]
                if gates[nm].paused:
                    for fn in (g.read_squelch, g.read_audio):
                        with pytest.raises(PsdrError) as e:
                            fn(F)
                        assert e.value.code == -7  # PSDR_ERR_NO_DATA
                    continue
                a, b = read_client(g, kind, F), read_client(h, kind, F)
                try:
                    assert_same_bits(a, b, f"{nm} at frame {at}", row_names(kind))
                except AssertionError as e:
                    o["diff"].append(str(e))
                o["got"].append(g.read_squelch(F).copy())
                o["want"].append(gates[nm].batch(a[1]))
                o["pwr"].append(a[1].copy())
                o["frames"] += list(range(at, at + F))
                assert np.array_equal(h.read_squelch(F), np.ones(F, np.int32))  # a client without squelch reads 1, without device access
            at += F
        return {nm: {k: (np.concatenate(v) if k in ("got", "want", "pwr") else v) for k, v in o.items()} for nm, o in out.items()}
    finally:
        A.close()
        B.close()


CASES = [(s, n) for s in ("iq", "real") for n in (360, 128)]


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("shape,n", CASES)
def test_flags_are_the_models_for_every_kind_and_split(shape, n, split):
    res = flags_run(shape, n, split)
    for kind in KINDS:
        r = res[kind]
        with np.errstate(all="ignore"):
            print(f"{shape} n {n} split {split} {kind}: pwr dB {np.round(10 * np.log10(r['pwr']), 1).tolist()} flags {r['got'].tolist()}")
        assert r["got"].dtype == np.int32 and np.array_equal(r["got"], r["want"]), (kind, np.nonzero(r["got"] != r["want"])[0].tolist())
        ev = M.events(r["pwr"], r["want"], M.threshold(OPEN_DB), M.threshold(CLOSE_DB), ATTACK, HANG)
        assert ev == EVENTS, (kind, "the input does not hold", EVENTS - ev)
    first = res[KINDS[0]]["want"]
    assert all(np.array_equal(res[k]["want"], first) for k in KINDS)  # (pwr is the window's power in every kind: one sequence)
    # the paused client's state stood still: it left open with one frame of the hang used up, and goes on from there
    p = res["P"]
    assert p["frames"] == list(range(16)) + list(range(24, 32)) and np.array_equal(p["got"], p["want"])
    # (indices 15..18 are frames 15, 24, 25, 26: frame 24 is the second one below, within the hang, and 25 is a half frame - the
    # gate stays open; a state that started over at 24 would be closed until the attack completes at 27)
    assert p["want"][15:19].all() and first[24] == 0 and first[25] == 0 and first[26] == 0
    # off and on again restarts the state: the kinds' own sequence is still open at 23, this client is closed at 24
    r = res["R"]
    assert np.array_equal(r["got"], r["want"]) and r["want"][16:24].all() and r["want"][15] == 1 and r["want"][24] == 0
    assert first[23] == 1
    # new thresholds and counts keep it: open at 16, where a fresh state would be closed
    t = res["T"]
    assert np.array_equal(t["got"], t["want"]) and t["want"][15] == 1 and t["want"][16] == 1


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("shape,n", CASES)
def test_the_demodulator_is_untouched(shape, n, split):
    """rows, pwr, NaN flags and carrier records of every squelch client are the bytes of its twin without squelch"""
    res = flags_run(shape, n, split)
    for nm, r in res.items():
        assert not r["diff"], (nm, r["diff"][:3])
        assert len(r["got"]) >= 24


def test_chunk_seam():
    """2^12-point IQ, one batch of 130 frames: the gate opens between frames 63 and 64 and closes between 127 and 128 - the
    seams of the kernel's chunks of 64 frames; a second batch of 130 continues from the first one's state"""
    key = [0] * 64 + [1] * 65 + [0] * 2 + [0] * 60 + [1] * 6 + [0] * 64
    raw = stream("iq12", tuple(key), None, 9)
    F = 130
    A = Ctx("iq12", 360, 3, maxb=F, raw=raw)
    try:
        one = (OPEN_DB, OPEN_DB, 1, 0)
        cl = [(A.add("USB", one), Gate(one)), (A.add("AM", (OPEN_DB, CLOSE_DB, 3, 40)), Gate((OPEN_DB, CLOSE_DB, 3, 40)))]
        got, want = [[], []], [[], []]
        for b in range(2):
            A.batch(F)
            for i, (g, gate) in enumerate(cl):
                pwr = g.read_audio(F)[1]
                got[i].append(g.read_squelch(F).copy())
                want[i].append(gate.batch(pwr))
        for i in range(2):
            g, w = np.concatenate(got[i]), np.concatenate(want[i])
            print("seam client", i, g.tolist())
            assert np.array_equal(g, w), np.nonzero(g != w)[0].tolist()
        w = np.concatenate(want[0])
        assert (w[63], w[64], w[127], w[128]) == (0, 1, 1, 0) and not w[:64].any() and w[64:128].all()
        w = np.concatenate(want[1])
        # the long hang carries the open gate and its counter over the batch seam: 40 frames below from 129 on, closed at 169
        assert w[66] == 1 and w[129] == 1 and w[130] == 1 and w[168] == 1 and w[169] == 0 and w[193] == 1
    finally:
        A.close()


# ---- the post chain ----------------------------------------------------------------------------------------------------------
CHAIN_KINDS = ("USB", "AM", "FM", "SAM", "TUSB", "SAMU")
ALWAYS, NEVER = (-300.0, -300.0, 1, 0), (300.0, 300.0, 1, 0)
# The chain's AGC looks 200 ms ahead and the DC blocker delays by 32 samples: the first 2432 samples of a client's stream leave
# it as zeros.  So the chain's script is the 32-frame one four times over, 128 frames: the squelch clients' open frames alone
# are 4000 samples at n = 128 (64 a frame)
CHAIN_KEY = tuple(KEY[:32] * 4 + [0])
NFC = len(CHAIN_KEY) - 1


@functools.lru_cache(maxsize=None)
def chain_run(n, agc, pcm16):
    """context A: the six kinds with squelch, two neighbours without, an always-open and a never-open client (squelch switched
    off behind frame 15); context B: the same clients in the same slots, nobody with squelch.  Sixteen batches of 8."""
    names = list(CHAIN_KINDS) + ["N1", "N2", "ALWAYS", "NEVER"]
    kinds = list(CHAIN_KINDS) + ["USB", "AM", "AM", "AM"]
    sq = [STD] * len(CHAIN_KINDS) + [None, None, ALWAYS, NEVER]
    raw = stream("iq", CHAIN_KEY)
    A, B = (Ctx("iq", n, len(names) + 1, post=True, agc=agc, pcm16=pcm16, raw=raw) for _ in range(2))
    try:
        ga = [A.add(k, s) for k, s in zip(kinds, sq)]
        gb = [B.add(k) for k in kinds]
        out = {nm: dict(a=[], b=[], open=[]) for nm in names}
        for bi in range(NFC // 8):
            if bi == 2:
                ga[names.index("NEVER")].set_squelch(False)
            A.batch(8), B.batch(8)
            for nm, kind, g, h in zip(names, kinds, ga, gb):
                out[nm]["a"].append(read_client(g, kind, 8, pcm=True))
                out[nm]["b"].append(read_client(h, kind, 8, pcm=True))
                out[nm]["open"].append(g.read_squelch(8).copy())
        cat = lambda rows: tuple(np.concatenate([r[i] for r in rows]) for i in range(len(rows[0])))  # noqa: E731
        return {nm: dict(a=cat(o["a"]), b=cat(o["b"]), open=np.concatenate(o["open"]), kind=k) for (nm, o), k in zip(out.items(), kinds)}
    finally:
        A.close()
        B.close()


def oracle_pcm(audio, keep, h):
    """oracle.PostChain over the concatenation of the kept frames' rows: PCM rows [F][h], zero where a frame is not kept"""
    from oracle import oracle as O
    ch = O.PostChain(RATE)
    want = np.zeros((len(audio), h), np.int32)
    for f in range(len(audio)):
        if keep[f]:
            want[f] = ch.process(audio[f])
    return want


CHAIN_CASES = [(n, agc, p16) for n in (360, 128) for agc in (1, 0) for p16 in (0, 1)]


@pytest.mark.parametrize("n,agc,pcm16", CHAIN_CASES)
def test_chain_hears_the_open_frames_alone(n, agc, pcm16):
    res = chain_run(n, agc, pcm16)
    total = 0
    for nm in CHAIN_KINDS:
        r = res[nm]
        audio, nan, pcm = r["a"][0], r["a"][2], r["a"][-1]
        keep = (r["open"] == 1) & (nan == 0)
        assert keep.any() and (r["open"] == 0).any() and (nan != 0).any() and ((r["open"] == 1) & (nan != 0)).any(), nm
        want = oracle_pcm(audio, keep, n // 2)  # (one chain over all sixteen batches: the stream continues across them)
        assert not pcm[~keep].any(), (nm, "a closed or NaN frame has PCM")
        bad = [f for f in range(NFC) if not np.array_equal(pcm[f], want[f])]
        assert not bad, (nm, bad)
        total += int(np.count_nonzero(want))
        assert_same_bits(r["a"][:-1], r["b"][:-1], f"{nm}: demodulator", row_names(r["kind"]))
    assert total > 1000, "the chain was not exercised"


@pytest.mark.parametrize("n,agc,pcm16", CHAIN_CASES)
def test_chain_neighbours_always_open_and_never_open(n, agc, pcm16):
    res = chain_run(n, agc, pcm16)
    for nm in ("N1", "N2"):  # not affected by a bit
        assert_same_bits(res[nm]["a"], res[nm]["b"], nm, row_names(res[nm]["kind"], pcm=True))
        assert res[nm]["open"].all() and res[nm]["a"][-1].any()
    r = res["ALWAYS"]  # open from frame 0 on (the NaN frames apart, which neither chain sees): the twin's PCM bytes
    assert np.array_equal(r["open"], (~np.isnan(r["a"][1])).astype(np.int32)) and r["open"][0] == 1
    assert_same_bits(r["a"], r["b"], "always open", row_names("AM", pcm=True))
    r = res["NEVER"]
    audio, nan, pcm = r["a"][0], r["a"][2], r["a"][-1]
    assert not r["open"][:16].any() and r["open"][16:].all() and not pcm[:16].any()
    # switched off: the chain goes on from the state in front of the closed stretch - a fresh client's
    keep = np.arange(NFC) >= 16
    want = oracle_pcm(audio, keep & (nan == 0), n // 2)
    assert np.array_equal(pcm, want) and np.count_nonzero(want) > 100
    assert_same_bits(r["a"][:-1], r["b"][:-1], "never open: demodulator", row_names("AM"))


# ---- fetch, profiling, arguments ---------------------------------------------------------------------------------------------
def test_fetch_carries_the_flags():
    from phantomsdr_amd import PsdrError
    A = Ctx("iq", 360, 6)
    try:
        cl = [A.add("USB"), A.add("AM", STD), A.add("IQ"), A.add("IQ", (OPEN_DB, OPEN_DB, 1, 0)), A.add("FM")]
        seen = set()
        for bi in range(NF // 8):
            A.batch(8)
            if bi % 2:  # the asynchronous form
                A.ctx.fetch_begin(A.ctx.FETCH_AUDIO | A.ctx.FETCH_IQ)
                A.ctx.fetch_end()
            else:
                A.ctx.fetch_batch()
            for i, g in enumerate(cl):
                want = g.read_squelch(8)
                got = np.array([A.ctx.fetched_squelch(g.id, f) for f in range(8)], np.int32)
                assert np.array_equal(got, want), (bi, i)
                assert i in (1, 3) or want.all()
                if i in (1, 3):
                    seen |= set(want.tolist())
            with pytest.raises(PsdrError):
                A.ctx.fetched_squelch(cl[0].id, 8)
            if bi == 1:
                cl[1].set_squelch(False), cl[3].set_squelch(False)  # batch 2: no squelch client, no extra copy
            if bi == 2:
                cl[3].set_squelch(True, OPEN_DB, OPEN_DB, 1, 0)
        assert seen == {0, 1}
    finally:
        A.close()
    B = Ctx("iq", 360, 3)  # a context that never had a squelch client
    try:
        g = B.add("USB")
        B.batch(8)
        B.ctx.fetch_begin(B.ctx.FETCH_AUDIO)
        B.ctx.fetch_end()
        assert [B.ctx.fetched_squelch(g.id, f) for f in range(8)] == [1] * 8 and g.read_squelch(8).all()
    finally:
        B.close()


def test_no_squelch_no_trace():
    A = Ctx("iq", 360, 4, post=True)
    try:
        A.ctx.set_profiling(1)
        g, h = A.add("USB"), A.add("AM")
        A.batch(8), A.batch(8)
        A.ctx.synchronize()
        st = A.ctx.kernel_stats()
        assert "squelch" not in st and st["post_chain"][1] > 0 and st["demod_idft"][1] > 0
        h.set_squelch(True, *STD)  # ... and the profiler does see the kernel once a client has it
        A.batch(8)
        A.ctx.synchronize()
        assert A.ctx.kernel_stats()["squelch"][1] == 1
        assert g.read_squelch(8).all()
    finally:
        A.close()


def test_arguments():
    from phantomsdr_amd import PsdrError
    A = Ctx("iq", 360, 3)
    try:
        g = A.add("USB", STD)
        lib, h = A.ctx.lib, A.ctx.h
        bad = [(2, 1, -20.0, -23.0, 2, 3), (-1, 1, -20.0, -23.0, 2, 3), (g.id, 1, float("nan"), -23.0, 2, 3), (g.id, 1, -20.0, float("inf"), 2, 3),
               (g.id, 1, 300.5, -23.0, 2, 3), (g.id, 1, -20.0, -300.5, 2, 3), (g.id, 1, -20.0, -19.0, 2, 3), (g.id, 1, -20.0, -23.0, 0, 3),
               (g.id, 1, -20.0, -23.0, (1 << 20) + 1, 3), (g.id, 1, -20.0, -23.0, 2, -1), (g.id, 1, -20.0, -23.0, 2, (1 << 20) + 1), (2, 0, 0.0, 0.0, 1, 0)]
        for args in bad:
            assert lib.psdr_client_set_squelch(h, *args) == -1, args  # PSDR_ERR_INVALID
        with pytest.raises(PsdrError) as e:
            g.read_squelch(8)
        assert e.value.code == -4  # no batch yet
        A.batch(8)
        flags = g.read_squelch(8)
        want, _ = M.run(g.read_audio(8)[1], M.threshold(OPEN_DB), M.threshold(CLOSE_DB), ATTACK, HANG)  # nothing of the refused calls took
        assert np.array_equal(flags, want)
        with pytest.raises(PsdrError) as e:
            g.read_squelch(7)
        assert e.value.code == -1
        assert lib.psdr_client_set_squelch(h, g.id, 1, 300.0, -300.0, 1 << 20, 1 << 20) == 0 and lib.psdr_client_set_squelch(h, g.id, 0, float("nan"), 1.0, -3, -3) == 0
    finally:
        A.close()

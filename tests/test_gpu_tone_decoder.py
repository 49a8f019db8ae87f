"""Per-client tone decoder on the GPU (include/psdr.h: psdr_client_set_tone_decoder, psdr_read_tone).

The detector's input is the client's own rows and NaN flags, read back; tests/tone_model.py's records() - a numpy restatement of
the rule in its own f32 arithmetic - on those rows gives tone, level and open, compared as bits: there is no tolerance anywhere.
Every tone client has a twin without the decoder in a second context with the same clients, batches and history.

Input (the smallest context tests/test_gpu_audio_blanker.py's rig makes: a 2^12-point IQ transform, audio_rate 12000): unit noise
and a carrier 100.0 Hz above the lower edge of the clients' window - tone 12 for a USB client -, keyed off for the stream's last
third so that the gate closes again, and one NaN sample."""
import functools
import json
import os

import numpy as np
import pytest

import tone_model as M
from conftest import ROOT
from helpers import assert_same_bits, read_client, row_names
from test_gpu_squelch import RATE, SHAPES, Ctx, oracle_pcm

pytestmark = pytest.mark.gpu

SHAPE = "iq12"
NF = 120
# the issue's "5 x 6" is read as batches of 5 and 6 frames in turn (ten of each, then the last 10 frames): at h = 180 every one of them
# ends inside a block, so each batch carries a partial block over
SPLITS = {"120": (120,), "1x120": (1,) * 120, "3x40": (3,) * 40, "5+6": (5, 6) * 10 + (10,), "40x3": (40,) * 3}
NAN_HALF = 40
KEY_OFF = 70  # the carrier's last frame + 1
TONE, HZ = 12, 100.0
L0 = SHAPES[SHAPE][2]
WINDOW = (L0, L0 + 0.3, L0 + 100)


@functools.lru_cache(maxsize=None)
def raw_of(n, hz=HZ, seed=11):
    """f32 half-frames, flat: unit noise plus a carrier `hz` above client bin L0 (the lower edge of the rig's window)"""
    N = SHAPES[SHAPE][1]
    rng = np.random.default_rng(seed)
    ns = (NF + 1) * (N // 2)
    t = np.arange(ns, dtype=np.float64)
    x = rng.standard_normal(ns) + 1j * rng.standard_normal(ns)
    c = L0 + hz * n / RATE  # client bin c of an IQ spectrum is frequency index (c + N/2 + 1) mod N
    x += (t < KEY_OFF * (N // 2)) * 4.0 * np.exp(2j * np.pi * ((c + N // 2 + 1) % N) * t / N)
    raw = x.astype(np.complex64).view(np.float32).copy()
    raw[2 * (NAN_HALF * (N // 2) + 17)] = np.nan
    return raw


class TCtx(Ctx):
    def __init__(self, n, max_clients, maxb=NF, **kw):
        super().__init__(SHAPE, n, max_clients, maxb=maxb, raw=raw_of(n), **kw)

    def add(self, kind="USB", tone=None, **kw):
        g = super().add(kind, **kw)
        g.set_audio_range(*WINDOW)  # a sideband window: its lower edge is the carrier position, audio frequency zero
        if tone is not None:
            g.set_tone_decoder(True, **tone)
        return g


def cat(parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(len(parts[0])))


def rec_of(t):
    r = np.zeros(len(t[0]), M.REC_DTYPE)
    r["tone"], r["level"], r["open"] = t
    return r


def model(rows, flags, h, **cfg):
    return M.records(rows, flags, h, RATE, **cfg)


def record(name, **figures):
    d = os.path.join(ROOT, "build", "records")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "tone_gpu.jsonl"), "a") as f:
        f.write(json.dumps(dict(test=name, **figures)) + "\n")


# ---- records ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def records_run(n, split):
    A = TCtx(n, 3)
    try:
        A.add("AM")
        g = A.add("USB", tone=dict(gate=0, hang_blocks=2))
        A.ctx.set_profiling(1)
        a, t = [], []
        for F in SPLITS[split]:
            A.batch(F)
            a.append(read_client(g, "USB", F)), t.append(g.read_tone(F))
        return cat(a), cat(t), A.ctx.kernel_stats()
    finally:
        A.close()


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("n", (360, 512))
def test_records_are_the_models_on_the_clients_own_rows(n, split):
    (rows, _, nan), t, stats = records_run(n, split)
    h = n // 2
    assert rows.shape == (NF, h) and nan[NAN_HALF] and t[0].dtype == np.int32 and t[1].dtype == np.float32 and t[2].dtype == np.int32
    got, want = rec_of(t), model(rows, nan, h, gate=0, hang=2)
    print(f"n {n} split {split}: tone {got['tone'].tolist()} open {got['open'].tolist()} level {got['level'][KEY_OFF - 1]:.4g}")
    bad = [f for f in range(NF) if got[f].tobytes() != want[f].tobytes()]
    assert not bad, (bad[:8], got[bad[:4]], want[bad[:4]])
    # the window fills with block NB - 1; from there to the carrier's end the tone is named
    filled = -(-M.nb_of(RATE) * M.B // h)
    assert (got["tone"][:filled - 1] == -1).all() and not got["open"][:filled - 1].any()
    assert (got["tone"][filled:KEY_OFF] == TONE).all() and got["open"][filled + 2 * M.B // h + 1:KEY_OFF].all()
    assert got["tone"][-1] == -1 and got["open"][-1] == 0  # ... and the gate has closed behind it
    if split == "40x3":
        ms, cnt = stats["audio_tone"]
        record("records", n=n, split=split, launches=int(cnt), us_per_launch=1e3 * ms / max(cnt, 1))
        assert cnt == 3


# ---- the twin -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twin_run(n):
    """context A: a plain tone client and one with audio blanker, noise reduction and audio filter behind the decoder, gate = 0, and
    a squelch client; context B: the same clients without the decoder.  Post chain on."""
    from phantomsdr_amd import design_audio_filter
    sec = [design_audio_filter("highpass", RATE, 300.0)]
    A, B = TCtx(n, 4, post=True), TCtx(n, 4, post=True)
    try:
        cl = []
        for X, tone in ((A, dict(gate=0)), (B, None)):
            p = X.add("USB", tone=tone)
            q = X.add("USB", tone=tone)
            q.set_audio_blanker("normal"), q.set_noise_reduction("normal"), q.set_audio_filter(sec)
            s = X.add("USB", tone=tone, squelch=(-100.0, -100.0, 1, 0))
            cl.append((p, q, s))
        got = [[[] for _ in range(3)] for _ in range(2)]
        tones = [[] for _ in range(3)]
        for F in SPLITS["40x3"]:
            A.batch(F), B.batch(F)
            for x in range(2):
                for i, g in enumerate(cl[x]):
                    got[x][i].append(read_client(g, "USB", F, pcm=True) + (g.read_squelch(F),))
            for i, g in enumerate(cl[0]):
                tones[i].append(g.read_tone(F))
        out = [[cat(v) for v in side] for side in got], [cat(v) for v in tones]
        return out
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("n", (360, 512))
def test_a_twin_without_the_decoder_is_the_same_to_the_bit(n):
    (a, b), tones = twin_run(n)
    names = row_names("USB", pcm=True) + ("squelch flags",)
    for i, what in enumerate(("plain", "blanker + noise reduction + filter", "squelch")):
        assert_same_bits(a[i], b[i], what, names)
        assert a[i][3].any()  # (the chain ran)
    # the detector saw the rows in front of the blanker, the noise reduction and the filter: the plain client's records
    assert not np.array_equal(a[0][0], a[1][0])
    for k in range(3):
        assert np.array_equal(tones[0][k], tones[1][k]) and np.array_equal(tones[0][k], tones[2][k])
    assert (tones[1][0] == TONE).any()
    want = model(a[0][0], a[0][2], n // 2, gate=0)
    assert rec_of(tones[0]).tobytes() == want.tobytes()


# ---- the gate in the chain ----------------------------------------------------------------------------------------------------
SQ = (-100.0, -100.0, 1, 0)  # a level squelch that the NaN frames close (pwr is NaN there) and nothing else


@functools.lru_cache(maxsize=None)
def chain_run(n):
    names = ("T12", "T13", "SQ", "PLAIN")
    A, B = TCtx(n, 5, post=True), TCtx(n, 5, post=True)
    try:
        ca = [A.add("USB", tone=dict(want=12, gate=1, hang_blocks=2)), A.add("USB", tone=dict(want=13, gate=1)),
              A.add("USB", tone=dict(want=12, gate=1, hang_blocks=0), squelch=SQ), A.add("USB")]
        cb = [B.add("USB"), B.add("USB"), B.add("USB", squelch=SQ), B.add("USB")]
        res = {nm: dict(a=[], b=[], t=[], sa=[], sb=[]) for nm in names}
        for F in SPLITS["5+6"]:
            A.batch(F), B.batch(F)
            for nm, g, h in zip(names, ca, cb):
                r = res[nm]
                r["a"].append(read_client(g, "USB", F, pcm=True)), r["b"].append(read_client(h, "USB", F, pcm=True))
                r["sa"].append((g.read_squelch(F),)), r["sb"].append((h.read_squelch(F),))
                if nm != "PLAIN":
                    r["t"].append(g.read_tone(F))
        return {nm: {k: cat(v) for k, v in r.items() if v} for nm, r in res.items()}
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("n", (360, 512))
def test_the_chain_hears_the_open_frames_alone(n):
    res = chain_run(n)
    h = n // 2
    for nm in res:  # rows, pwr, NaN flags and squelch flags: the twin's
        assert_same_bits(res[nm]["a"][:3], res[nm]["b"][:3], nm, row_names("USB"))
        assert np.array_equal(res[nm]["sa"][0], res[nm]["sb"][0]), nm
    for nm, cfg in (("T12", dict(want=12, hang=2)), ("T13", dict(want=13)), ("SQ", dict(want=12, hang=0))):
        r = res[nm]
        assert rec_of(r["t"]).tobytes() == model(r["a"][0], r["a"][2], h, **cfg).tobytes(), nm
    r = res["T12"]
    audio, nan, pcm, op = r["a"][0], r["a"][2], r["a"][3], r["t"][2]
    keep = (op == 1) & (nan == 0)
    assert keep.any() and (op == 0).any() and ((op == 1) & (nan != 0)).any() and op[KEY_OFF - 1] == 1 and op[-1] == 0
    want = oracle_pcm(audio, keep, h)  # (one chain over all batches: AGC and DC blocker stand still across the closed frames)
    assert not pcm[~keep].any()
    assert [f for f in range(NF) if not np.array_equal(pcm[f], want[f])] == [] and np.count_nonzero(want) > 1000
    r = res["T13"]  # the wrong tone: shut for the whole stream
    assert not r["t"][2].any() and (r["t"][0] == -1).all() and r["t"][1].max() > 0 and not r["a"][3].any() and r["b"][3].any()
    r = res["SQ"]  # level squelch and tone gate together: nan | !sq_open | !tone_open
    audio, nan, pcm, op, sq = r["a"][0], r["a"][2], r["a"][3], r["t"][2], r["sa"][0]
    keep = (nan == 0) & (sq == 1) & (op == 1)
    assert keep.any() and (sq == 0).any() and (op == 0).any()
    assert np.array_equal(pcm, oracle_pcm(audio, keep, h)) and not pcm[~keep].any()
    r = res["PLAIN"]  # a client without either, in the same batches: the twin's bytes, PCM included
    assert_same_bits(r["a"], r["b"], "plain", row_names("USB", pcm=True))
    assert r["a"][3].any()


# ---- lifecycle ----------------------------------------------------------------------------------------------------------------
def test_restart_pause_slots_and_errors():
    from phantomsdr_amd import AudioClient, Context, PsdrError
    n, h = 360, 180
    cfg = dict(gate=0, attack_blocks=1)
    mc = dict(gate=0, attack=1)
    A = TCtx(n, 12, maxb=40)
    try:
        fill = [A.add("AM") for _ in range(5)]  # the table index is not the slot (slots past 64, holes and a reused high slot: tests/test_gpu_tone_slots.py)
        names = ("KEEP", "RETUNE", "MODE", "AGAIN", "PAUSE", "REUSE", "IQ")
        cl = dict(zip(names, [A.add("USB", tone=cfg) for _ in names[:-1]] + [A.add("USB")]))
        assert cl["REUSE"].id == 10 and cl["IQ"].id == 11
        rows = {nm: [] for nm in names}
        recs = {nm: [] for nm in names}
        kinds = dict.fromkeys(names, "USB")
        for bi in range(3):
            if bi == 1:
                cl["RETUNE"].set_audio_range(L0 - 1, L0 - 0.7, L0 + 99)
                cl["MODE"].set_audio_demodulation("LSB"), kinds.update(MODE="LSB")
                cl["AGAIN"].set_tone_decoder(True, **cfg)
                cl["PAUSE"].set_paused(True)
                cl["REUSE"].on_close()
                g = AudioClient(A.ctx)  # the slot's next occupant starts from zero, and without the decoder
                assert g.id == 10
                g.set_audio_range(*WINDOW)
                cl["REUSE"] = g
                cl["IQ"].set_tone_decoder(True, **cfg)  # on as USB, then an IQ client: keeps the setting, is not listed
                cl["IQ"].set_audio_demodulation("IQ")
            if bi == 2:
                cl["PAUSE"].set_paused(False)
                cl["REUSE"].set_tone_decoder(True, **cfg)
                cl["IQ"].set_audio_demodulation("USB")
            A.batch(40)
            for nm in names:
                g = cl[nm]
                silent = (nm == "PAUSE" and bi == 1) or (nm == "REUSE" and bi == 1) or (nm == "IQ" and bi < 2)
                if silent:
                    with pytest.raises(PsdrError) as e:
                        g.read_tone(40)
                    assert e.value.code == -7, nm  # PSDR_ERR_NO_DATA
                    continue
                a = g.read_audio(40)
                rows[nm].append((a[0], a[2])), recs[nm].append(rec_of(g.read_tone(40)))
        with pytest.raises(PsdrError) as e:
            fill[0].read_tone(40)
        assert e.value.code == -7
        with pytest.raises(PsdrError) as e:
            cl["IQ"].set_audio_demodulation("IQ"), cl["IQ"].set_tone_decoder(True)
        assert e.value.code == -1 and "PSDR_IQ" in str(e.value)

        def want(nm, parts):
            r, f = cat([rows[nm][i] for i in parts])
            return model(r, f, h, **mc)

        def got(nm, parts):
            return np.concatenate([recs[nm][i] for i in parts])

        assert got("KEEP", (0, 1, 2)).tobytes() == want("KEEP", (0, 1, 2)).tobytes()
        assert (got("KEEP", (1,))["tone"] == TONE).all()
        for nm in ("RETUNE", "MODE", "AGAIN"):  # batch 0, then from zero at batch 1
            assert got(nm, (0,)).tobytes() == want(nm, (0,)).tobytes() and got(nm, (1, 2)).tobytes() == want(nm, (1, 2)).tobytes(), nm
            assert (got(nm, (1,))["tone"][:20] == -1).all(), nm
        # the paused client's state stood still: batch 2 goes on behind batch 0, its window still full of the tone (the carrier
        # ended while the client sat out; a state from zero would name nothing for 27 frames)
        assert got("PAUSE", (0, 1)).tobytes() == want("PAUSE", (0, 1)).tobytes() and (got("PAUSE", (1,))["tone"][:10] == TONE).all()
        for nm in ("REUSE", "IQ"):  # their one listed batch starts from zero
            assert got(nm, (-1,)).tobytes() == want(nm, (-1,)).tobytes() and (got(nm, (-1,))["tone"][:20] == -1).all(), nm
    finally:
        A.close()
    # an audio_rate outside [2000, 48000]: PSDR_ERR_STATE, and the defaults refuse it
    _, N, _ = SHAPES[SHAPE]
    ctx = Context(N, False, 4, additional_size=n, audio_fft_size=n, audio_rate=1000, input_format="f32", max_batch=8, max_clients=2)
    try:
        g = AudioClient(ctx)
        with pytest.raises(PsdrError) as e:
            g.set_tone_decoder(True)
        assert e.value.code == -4 and "audio_rate" in str(e.value)
        g.set_tone_decoder(False)
    finally:
        ctx.close()

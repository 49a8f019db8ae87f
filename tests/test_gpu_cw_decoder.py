"""Per-client CW decoder on the GPU (include/psdr.h: psdr_client_set_cw_decoder, psdr_read_cw, psdr_read_cw_text).

The decoder's input is the client's own rows and NaN flags, read back; tests/cw_model.py's records() - a numpy restatement of the
rule in its own f32 arithmetic - on those rows gives the records and the text, compared as bits: there is no tolerance anywhere.
The decoded client has a twin without the decoder in a second context with the same clients, batches and history.

Input (the smallest context tests/test_gpu_tone_decoder.py's rig makes: a 2^12-point IQ transform, audio_rate 12000): unit noise and
a carrier of amplitude 4, 700 Hz above the lower edge of a USB client's window, keyed in the raw samples with `CQ DE K` at 25 WPM
behind 0.75 s of noise alone (the floor's ring fills in 0.68 s), and one NaN sample in the gap behind `DE`."""
import functools
import json
import os

import numpy as np
import pytest

import cw_model as M
from conftest import ROOT
from helpers import assert_same_bits, read_client, row_names
from test_gpu_squelch import RATE, SHAPES, Ctx, oracle_pcm

pytestmark = pytest.mark.gpu

SHAPE = "iq12"
TEXT, WPM, PITCH, LEAD = "CQ DE K", 25.0, 700.0, 0.75
NF = {360: 258, 512: 183}  # the keying and 3.5 to 4.8 dots of noise behind it: the last character's space and no word space; 3 divides both
# (5, 6) in turn, then what is left: at h = 180 every one of these batches ends inside a hop
SPLITS = {"whole": lambda nf: (nf,), "1 per batch": lambda nf: (1,) * nf, "5+6": lambda nf: (5, 6) * (nf // 11) + ((nf % 11,) if nf % 11 else ()),
          "3 parts": lambda nf: (nf // 3,) * 3}
L0 = SHAPES[SHAPE][2]
WINDOW = (L0, L0 + 0.3, L0 + 100)
CFG = dict(wpm=WPM)


def timing(n):
    """(raw samples per second, the keying's runs as (on, first raw sample, end), the NaN sample's index)"""
    N = SHAPES[SHAPE][1]
    fs = RATE * (N // 2) / (n // 2)  # a frame is N / 2 raw samples and n / 2 audio samples
    dot, t, runs = 1.2 / WPM, LEAD, []
    for on, dots in M.keying(TEXT):
        runs.append((on, int(round(t * fs)), int(round((t + dots * dot) * fs))))
        t += dots * dot
    gaps = [r for r in runs if not r[0] and r[2] - r[1] > 6 * dot * fs]
    assert len(gaps) == 2
    return fs, runs, (gaps[1][1] + gaps[1][2]) // 2, t


@functools.lru_cache(maxsize=None)
def raw_of(n, seed=11):
    """f32 half-frames, flat: unit noise plus the keyed carrier PITCH above client bin L0 (the lower edge of the rig's window)"""
    N = SHAPES[SHAPE][1]
    fs, runs, nan_at, t_end = timing(n)
    ns = (NF[n] + 1) * (N // 2)
    assert (t_end + 3.5 * 1.2 / WPM) * fs < NF[n] * (N // 2) < (t_end + 4.8 * 1.2 / WPM) * fs  # the stream ends between 2 u and 5 u of space
    rng = np.random.default_rng(seed)
    t = np.arange(ns, dtype=np.float64)
    x = rng.standard_normal(ns) + 1j * rng.standard_normal(ns)
    key = np.zeros(ns)
    for on, a, b in runs:
        key[a:b] = on
    c = L0 + PITCH * n / RATE  # client bin c of an IQ spectrum is frequency index (c + N/2 + 1) mod N
    x += key * 4.0 * np.exp(2j * np.pi * ((c + N // 2 + 1) % N) * t / N)
    raw = x.astype(np.complex64).view(np.float32).copy()
    raw[2 * nan_at] = np.nan
    return raw


class CCtx(Ctx):
    def __init__(self, n, max_clients, maxb=None, **kw):
        super().__init__(SHAPE, n, max_clients, maxb=maxb or NF[n], raw=raw_of(n), **kw)

    def add(self, kind="USB", cw=None, tone=None, **kw):
        g = super().add(kind, **kw)
        g.set_audio_range(*WINDOW)  # a sideband window: its lower edge is audio frequency zero
        if cw is not None:
            g.set_cw_decoder(True, **cw)
        if tone is not None:
            g.set_tone_decoder(True, **tone)
        return g


def cat(parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(len(parts[0])))


def rec_of(t):
    r = np.zeros(len(t[0]), M.REC_DTYPE)
    r["nchars"], r["wpm"], r["pitch_hz"], r["level"], r["key"] = t
    return r


def model(rows, flags, h, **cfg):
    return M.records(rows, flags, h, RATE, **cfg)


def record(name, **figures):
    d = os.path.join(ROOT, "build", "records")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "cw_gpu.jsonl"), "a") as f:
        f.write(json.dumps(dict(test=name, **figures)) + "\n")


# ---- records and text ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def records_run(n, split):
    A = CCtx(n, 3)
    try:
        A.add("AM")
        g = A.add("USB", cw=CFG)
        A.ctx.set_profiling(1)
        a, t = [], []
        for F in SPLITS[split](NF[n]):
            A.batch(F)
            a.append(read_client(g, "USB", F)), t.append(g.read_cw(F))
        return cat(a), cat(t), g.read_cw_text(), A.ctx.kernel_stats()
    finally:
        A.close()


@functools.lru_cache(maxsize=None)
def model_run(n):
    (rows, _, nan), _, _, _ = records_run(n, "whole")
    return model(rows, nan, n // 2, **CFG)


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("n", (360, 512))
def test_records_and_text_are_the_models_on_the_clients_own_rows(n, split):
    (rows, _, nan), t, (text, total), stats = records_run(n, split)
    h = n // 2
    assert rows.shape == (NF[n], h) and nan.any() and t[0].dtype == np.uint32 and t[4].dtype == np.int32
    assert_same_bits((rows, nan), records_run(n, "whole")[0][::2], "the rows of every split", ("audio", "nan"))
    want, wtext = model_run(n)
    got = rec_of(t)
    print(f"n {n} split {split}: text {text!r} wpm {got['wpm'][-1]:.2f} pitch {got['pitch_hz'][-1]} level {got['level'].max():.4g}")
    bad = [f for f in range(NF[n]) if got[f].tobytes() != want[f].tobytes()]
    assert not bad, (bad[:8], got[bad[:4]], want[bad[:4]])
    assert text == wtext and total == len(wtext) == got["nchars"][-1]
    assert got["key"].any() and not got["key"][:int(LEAD * RATE / h)].any()
    if split == "3 parts":
        ms, cnt = stats["audio_cw"]
        record("records", n=n, split=split, frames=NF[n] // 3, launches=int(cnt), us_per_launch=1e3 * ms / max(cnt, 1))
        assert cnt == 3


@pytest.mark.parametrize("n", (360, 512))
def test_the_text_is_what_was_sent(n):
    _, t, (text, total), _ = records_run(n, "whole")
    assert text == TEXT and total == len(TEXT)
    got = rec_of(t)
    assert abs(got["pitch_hz"][-1] - PITCH) <= M.DF and abs(got["wpm"][-1] / WPM - 1) < 0.1  # (a lane beside it loses under 1 dB)


# ---- the twin -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twin_run(n):
    """context A: a plain CW client and one with audio blanker, noise reduction and audio filter behind the decoder; context B: the
    same clients without the decoder.  Post chain on."""
    from phantomsdr_amd import design_audio_filter
    sec = [design_audio_filter("highpass", RATE, 300.0)]
    A, B = CCtx(n, 3, post=True), CCtx(n, 3, post=True)
    try:
        cl = []
        for X, cw in ((A, CFG), (B, None)):
            p = X.add("USB", cw=cw)
            q = X.add("USB", cw=cw)
            q.set_audio_blanker("normal"), q.set_noise_reduction("normal"), q.set_audio_filter(sec)
            cl.append((p, q))
        got = [[[] for _ in range(2)] for _ in range(2)]
        for F in SPLITS["3 parts"](NF[n]):
            A.batch(F), B.batch(F)
            for x in range(2):
                for i, g in enumerate(cl[x]):
                    got[x][i].append(read_client(g, "USB", F, pcm=True))
        texts = [g.read_cw_text()[0] for g in cl[0]]
        return [[cat(v) for v in side] for side in got], texts
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("n", (360, 512))
def test_a_twin_without_the_decoder_is_the_same_to_the_bit(n):
    (a, b), texts = twin_run(n)
    for i, what in enumerate(("plain", "blanker + noise reduction + filter")):
        assert_same_bits(a[i], b[i], what, row_names("USB", pcm=True))
        assert a[i][3].any()  # (the chain ran)
    # the decoder saw the rows in front of the blanker, the noise reduction and the filter: the plain client's text
    assert not np.array_equal(a[0][0], a[1][0]) and texts[0] == texts[1] == TEXT
    audio, nan, pcm = a[0][0], a[0][2], a[0][3]
    assert np.array_equal(pcm, oracle_pcm(audio, nan == 0, n // 2))


# ---- lifecycle ----------------------------------------------------------------------------------------------------------------
def test_restart_pause_text_reads_and_errors():
    from phantomsdr_amd import AudioClient, Context, PsdrError
    n, h, F = 360, 180, 86
    A = CCtx(n, 8, maxb=F)
    B = CCtx(n, 2, maxb=F)
    try:
        fill = A.add("AM")
        names = ("KEEP", "RETUNE", "MODE", "AGAIN", "PAUSE", "IQ")
        cl = dict(zip(names, [A.add("USB", cw=CFG) for _ in names[:-1]] + [A.add("USB")]))
        B.add("USB")
        rows = {nm: [] for nm in names}
        recs = {nm: [] for nm in names}
        totals = {nm: [] for nm in names}
        for bi in range(3):
            if bi == 1:
                cl["RETUNE"].set_audio_range(L0 - 1, L0 - 0.7, L0 + 99)
                cl["MODE"].set_audio_demodulation("LSB")
                cl["AGAIN"].set_cw_decoder(False), cl["AGAIN"].set_cw_decoder(True, **CFG)
                assert cl["AGAIN"].read_cw_text() == ("", 0)  # the start is pending
                cl["PAUSE"].set_paused(True)
                cl["IQ"].set_cw_decoder(True, **CFG)  # on as USB, then an IQ client: keeps the setting, is not listed
                cl["IQ"].set_audio_demodulation("IQ")
            if bi == 2:
                cl["PAUSE"].set_paused(False)
                cl["IQ"].set_audio_demodulation("USB")
            A.batch(F), B.batch(F)
            for nm in names:
                g = cl[nm]
                if (nm == "PAUSE" and bi == 1) or (nm == "IQ" and bi < 2):
                    with pytest.raises(PsdrError) as e:
                        g.read_cw(F)
                    assert e.value.code == -7, nm  # PSDR_ERR_NO_DATA
                    continue
                a = g.read_audio(F)
                rows[nm].append((a[0], a[2])), recs[nm].append(rec_of(g.read_cw(F))), totals[nm].append(g.read_cw_text()[1])
        with pytest.raises(PsdrError) as e:
            fill.read_cw(F)
        assert e.value.code == -7
        with pytest.raises(PsdrError) as e:
            fill.read_cw_text()
        assert e.value.code == -7
        with pytest.raises(PsdrError) as e:
            cl["IQ"].set_audio_demodulation("IQ"), cl["IQ"].set_cw_decoder(True)
        assert e.value.code == -1 and "PSDR_IQ" in str(e.value)
        for bad in (dict(pitch_hz=299.0), dict(search_hz=801.0), dict(wpm=float("nan")), dict(track_speed=2), dict(snr_db=41.0)):
            with pytest.raises(PsdrError) as e:
                cl["KEEP"].set_cw_decoder(True, **bad)
            assert e.value.code == -1 and list(bad)[0] in str(e.value)

        def want(nm, parts):
            r, f = cat([rows[nm][i] for i in parts])
            return model(r, f, h, **CFG)

        def got(nm, parts):
            return np.concatenate([recs[nm][i] for i in parts])

        w, wtext = want("KEEP", (0, 1, 2))
        assert got("KEEP", (0, 1, 2)).tobytes() == w.tobytes() and wtext == TEXT
        # the text reads: from 0, from the middle, from total, beyond total
        g = cl["KEEP"]
        assert g.read_cw_text() == (TEXT, len(TEXT)) and g.read_cw_text(3) == (TEXT[3:], len(TEXT)) and g.read_cw_text(len(TEXT)) == ("", len(TEXT))
        with pytest.raises(PsdrError) as e:
            g.read_cw_text(len(TEXT) + 1)
        assert e.value.code == -1 and "beyond" in str(e.value)
        for nm in ("RETUNE", "MODE", "AGAIN"):  # batch 0, then from zero at batch 1: the text count restarts
            w0, w1 = want(nm, (0,)), want(nm, (1, 2))
            assert got(nm, (0,)).tobytes() == w0[0].tobytes() and got(nm, (1, 2)).tobytes() == w1[0].tobytes(), nm
            assert totals[nm][0] == len(w0[1]) and totals[nm][2] == len(w1[1]) and (nm == "MODE" or totals[nm][2] > 0), nm  # (LSB: the carrier is outside)
            assert got(nm, (1,))["nchars"][0] == 0 and not got(nm, (1,))["key"][:40].any(), nm  # the ring fills again: 0.68 s without a key
        # the paused client's state stood still: batch 2 goes on behind batch 0
        assert got("PAUSE", (0, 1)).tobytes() == want("PAUSE", (0, 1))[0].tobytes() and totals["PAUSE"][1] > 0
        assert got("IQ", (0,)).tobytes() == want("IQ", (0,))[0].tobytes() and got("IQ", (0,))["nchars"][0] == 0
        # a context that never had a CW client has launched nothing
        B.ctx.set_profiling(1)
        B.batch(F)
        assert "audio_cw" not in B.ctx.kernel_stats() or B.ctx.kernel_stats()["audio_cw"][1] == 0
    finally:
        A.close()
        B.close()
    # an audio_rate outside [4000, 48000]: PSDR_ERR_STATE, and the defaults refuse it
    _, N, _ = SHAPES[SHAPE]
    ctx = Context(N, False, 4, additional_size=n, audio_fft_size=n, audio_rate=3000, input_format="f32", max_batch=8, max_clients=2)
    try:
        g = AudioClient(ctx)
        with pytest.raises(PsdrError) as e:
            g.set_cw_decoder(True)
        assert e.value.code == -4 and "audio_rate" in str(e.value)
        g.set_cw_decoder(False)
    finally:
        ctx.close()


def test_a_from_older_than_the_ring_reads_no_data():
    """the stream over and over until the text is longer than the ring: what was read pass by pass is the truth for the ring's
    last 1024 characters; one character older reads PSDR_ERR_NO_DATA"""
    from phantomsdr_amd import PsdrError
    n = 360
    A = CCtx(n, 2)
    try:
        g = A.add("USB", cw=CFG)
        text, total = "", 0
        for _ in range(200):
            A.frame = 0
            A.batch(NF[n])
            new, total = g.read_cw_text(since=total)
            text += new
            if total > M.TEXT + 8:
                break
        assert total == len(text) > M.TEXT + 8 and text.startswith(TEXT)
        with pytest.raises(PsdrError) as e:
            g.read_cw_text(total - M.TEXT - 1)
        assert e.value.code == -7 and "older" in str(e.value)
        assert g.read_cw_text(total - M.TEXT) == (text[-M.TEXT:], total)
        assert g.read_cw(NF[n])[0][-1] == total
    finally:
        A.close()

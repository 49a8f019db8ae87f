"""Per-client RTTY decoder on the GPU (include/psdr.h: psdr_client_set_rtty_decoder, psdr_read_rtty, psdr_read_rtty_text).

The decoder's input is the client's own rows and NaN flags, read back; tests/rtty_model.py's records() - a numpy restatement of the
rule in its own f32 arithmetic - on those rows gives the records and the text, compared as bits: there is no tolerance anywhere.
The decoded client has a twin without the decoder in a second context with the same clients, batches and history.

Input (tests/test_gpu_cw_decoder.py's rig: a 2^12-point IQ transform, audio_rate 12000, a USB client whose window's lower edge is
audio zero): unit noise and, behind 0.75 s of noise alone, a carrier of amplitude 4 that the sender of tests/rtty_model.py shifts
between 915 Hz (mark) and 1085 Hz (space) above the window's lower edge in the raw samples, phase-continuous: 0.6 s of idle mark with
one NaN sample 0.1 s into it, `RY 599 K` and CR LF at 75 baud, and mark to the stream's end."""
import functools

import numpy as np
import pytest

import rtty_model as M
import tone_model as TM
from helpers import assert_same_bits, read_client, row_names
from test_gpu_cw_decoder import L0, SHAPE, WINDOW, cat
from test_gpu_cw_decoder import model as cw_model_of
from test_gpu_cw_decoder import rec_of as cw_rec_of
from test_gpu_squelch import RATE, SHAPES, Ctx, oracle_pcm

pytestmark = pytest.mark.gpu

TEXT, BAUD, MARK, SHIFT = "RY 599 K\r\n", 75.0, 915.0, 170.0
LEAD, IDLE, NAN_AT, TAIL = 0.75, 0.6, 0.85, 0.25
CFG = dict(mark_hz=MARK, shift_hz=SHIFT, baud=BAUD)
SPLITS = {"whole": lambda nf: (nf,), "1 per batch": lambda nf: (1,) * nf, "5+6": lambda nf: (5, 6) * (nf // 11) + ((nf % 11,) if nf % 11 else ()),
          "3 parts": lambda nf: (nf // 3,) * 3}


def frames_of(n, text=TEXT, baud=BAUD):
    t = LEAD + sum(r[1] for r in M.line_runs(text, baud, lead=IDLE, tail=TAIL))
    return 3 * int(np.ceil(t * RATE / (n // 2) / 3))


def fsk_raw(n, nf, rate=RATE, text=TEXT, baud=BAUD, mark=MARK, shift=SHIFT, seed=11, nan_at=NAN_AT, lead=LEAD, idle=IDLE):
    """f32 half-frames, flat: unit noise plus the shifted carrier above client bin L0 (the lower edge of the rig's window)"""
    N = SHAPES[SHAPE][1]
    fs = rate * (N // 2) / (n // 2)  # a frame is N / 2 raw samples and n / 2 audio samples
    ns = (nf + 1) * (N // 2)
    rng = np.random.default_rng(seed)
    x = np.empty(ns, np.complex64)
    x.real, x.imag = rng.standard_normal(ns, dtype=np.float32), rng.standard_normal(ns, dtype=np.float32)
    runs = M.line_runs(text, baud, lead=idle, tail=ns / fs)
    edges = np.minimum(np.round((lead + np.cumsum([0.0] + [r[1] for r in runs])) * fs).astype(np.int64), ns)
    hz = np.zeros(ns)
    for (mk, _), a, b in zip(runs, edges[:-1], edges[1:]):
        hz[a:b] = mark if mk else mark + shift
    c = L0 + hz[edges[0]:] * n / rate  # client bin c of an IQ spectrum is frequency index (c + N/2 + 1) mod N
    w = 2 * np.pi * ((c + N // 2 + 1) % N) / N
    x[edges[0]:] += (4.0 * np.exp(1j * np.concatenate([[0.0], np.cumsum(w[:-1])]))).astype(np.complex64)
    raw = x.view(np.float32)
    raw[2 * int(round(nan_at * fs))] = np.nan
    return raw


@functools.lru_cache(maxsize=None)
def raw_of(n):
    return fsk_raw(n, frames_of(n))


class RCtx(Ctx):
    def __init__(self, n, max_clients, maxb=None, **kw):
        super().__init__(SHAPE, n, max_clients, maxb=maxb or frames_of(n), raw=raw_of(n), **kw)

    def add(self, kind="USB", rtty=None, cw=None, tone=None, **kw):
        g = super().add(kind, **kw)
        g.set_audio_range(*WINDOW)  # a sideband window: its lower edge is audio frequency zero
        if rtty is not None:
            g.set_rtty_decoder(True, **rtty)
        if cw is not None:
            g.set_cw_decoder(True, **cw)
        if tone is not None:
            g.set_tone_decoder(True, **tone)
        return g


def rec_of(t):
    r = np.zeros(len(t[0]), M.REC_DTYPE)
    r["nchars"], r["errors"], r["offset_hz"], r["level"], r["quality"], r["present"] = t
    return r


def model(rows, flags, h, **cfg):
    return M.records(rows, flags, h, RATE, **cfg)


def same_records(got, want, what):
    bad = [f for f in range(len(want)) if got[f].tobytes() != want[f].tobytes()]
    assert len(got) == len(want) and not bad, (what, bad[:8], got[bad[:4]], want[bad[:4]])


# ---- records and text ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def records_run(n, split):
    A = RCtx(n, 3)
    try:
        A.add("AM")
        g = A.add("USB", rtty=CFG)
        A.ctx.set_profiling(1)
        a, t = [], []
        for F in SPLITS[split](frames_of(n)):
            A.batch(F)
            a.append(read_client(g, "USB", F)), t.append(g.read_rtty(F))
        return cat(a), cat(t), g.read_rtty_text(), A.ctx.kernel_stats()
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
    h, nf = n // 2, frames_of(n)
    assert rows.shape == (nf, h) and nan.any() and t[0].dtype == np.uint32 and t[1].dtype == np.uint32 and t[5].dtype == np.int32
    assert_same_bits((rows, nan), records_run(n, "whole")[0][::2], "the rows of every split", ("audio", "nan"))
    want, wtext = model_run(n)
    got = rec_of(t)
    print(f"n {n} split {split}: text {text!r} errors {got['errors'][-1]} offset {got['offset_hz'][-1]} level {got['level'].max():.4g} quality {got['quality'][-1]:.4g}")
    same_records(got, want, (n, split))
    assert text == wtext and total == len(wtext) == got["nchars"][-1]
    assert wtext == TEXT and want["errors"][-1] == 0  # the input is decodable: the model alone reads what was sent
    assert got["present"].any() and not got["present"][:int(LEAD * RATE / h)].any()
    assert stats["audio_rtty"][1] == len(SPLITS[split](nf))


# ---- the twin -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twin_run(n):
    """context A: a plain RTTY client and one with audio blanker, noise reduction and audio filter behind the decoder; context B: the
    same clients without the decoder.  Post chain on."""
    from phantomsdr_amd import design_audio_filter
    sec = [design_audio_filter("highpass", RATE, 300.0)]
    A, B = RCtx(n, 3, post=True), RCtx(n, 3, post=True)
    try:
        cl = []
        for X, rt in ((A, CFG), (B, None)):
            p = X.add("USB", rtty=rt)
            q = X.add("USB", rtty=rt)
            q.set_audio_blanker("normal"), q.set_noise_reduction("normal"), q.set_audio_filter(sec)
            cl.append((p, q))
        got = [[[] for _ in range(2)] for _ in range(2)]
        for F in SPLITS["3 parts"](frames_of(n)):
            A.batch(F), B.batch(F)
            for x in range(2):
                for i, g in enumerate(cl[x]):
                    got[x][i].append(read_client(g, "USB", F, pcm=True))
        texts = [g.read_rtty_text()[0] for g in cl[0]]
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


# ---- life cycle ---------------------------------------------------------------------------------------------------------------
def test_restart_pause_text_reads_and_errors():
    from phantomsdr_amd import AudioClient, Context, PsdrError
    n, h = 360, 180
    F = frames_of(n) // 3
    A = RCtx(n, 8, maxb=F)
    B = RCtx(n, 2, maxb=F)
    try:
        fill = A.add("AM")
        names = ("KEEP", "RETUNE", "MODE", "AGAIN", "PAUSE", "IQ")
        cl = dict(zip(names, [A.add("USB", rtty=CFG) for _ in names[:-1]] + [A.add("USB")]))
        B.add("USB")
        rows, recs, totals = ({nm: [] for nm in names} for _ in range(3))
        for bi in range(3):
            if bi == 1:
                cl["RETUNE"].set_audio_range(L0 - 1, L0 - 0.7, L0 + 99)
                cl["MODE"].set_audio_demodulation("LSB")
                cl["AGAIN"].set_rtty_decoder(False), cl["AGAIN"].set_rtty_decoder(True, **CFG)
                assert cl["AGAIN"].read_rtty_text() == ("", 0)  # the start is pending
                cl["PAUSE"].set_paused(True)
                cl["IQ"].set_rtty_decoder(True, **CFG)  # on as USB, then an IQ client: keeps the setting, is not listed
                cl["IQ"].set_audio_demodulation("IQ")
            if bi == 2:
                cl["PAUSE"].set_paused(False)
                cl["IQ"].set_audio_demodulation("USB")
            A.batch(F), B.batch(F)
            for nm in names:
                g = cl[nm]
                if (nm == "PAUSE" and bi == 1) or (nm == "IQ" and bi < 2):
                    with pytest.raises(PsdrError) as e:
                        g.read_rtty(F)
                    assert e.value.code == -7, nm  # PSDR_ERR_NO_DATA
                    continue
                a = g.read_audio(F)
                rows[nm].append((a[0], a[2])), recs[nm].append(rec_of(g.read_rtty(F))), totals[nm].append(g.read_rtty_text()[1])
        for call in (lambda: fill.read_rtty(F), fill.read_rtty_text):
            with pytest.raises(PsdrError) as e:
                call()
            assert e.value.code == -7
        with pytest.raises(PsdrError) as e:
            cl["IQ"].set_audio_demodulation("IQ"), cl["IQ"].set_rtty_decoder(True)
        assert e.value.code == -1 and "PSDR_IQ" in str(e.value)
        for bad in (dict(mark_hz=299.0), dict(shift_hz=84.0), dict(baud=float("nan")), dict(usos=2), dict(search_hz=161.0), dict(snr_db=31.0)):
            with pytest.raises(PsdrError) as e:
                cl["KEEP"].set_rtty_decoder(True, **dict(CFG, **bad))
            assert e.value.code == -1 and list(bad)[0] in str(e.value)
        with pytest.raises(PsdrError) as e:
            cl["KEEP"].set_rtty_decoder(True, mark_hz=300.0, shift_hz=-170.0, baud=75.0)  # the space tone's lowest pair would lie at -30 Hz
        assert e.value.code == -4 and "tones" in str(e.value)

        def want(nm, parts):
            r, f = cat([rows[nm][i] for i in parts])
            return model(r, f, h, **CFG)

        def got(nm, parts):
            return np.concatenate([recs[nm][i] for i in parts])

        w, wtext = want("KEEP", (0, 1, 2))
        same_records(got("KEEP", (0, 1, 2)), w, "KEEP")
        assert wtext == TEXT
        # the text reads: from 0, from the middle, from total, beyond total
        g = cl["KEEP"]
        assert g.read_rtty_text() == (TEXT, len(TEXT)) and g.read_rtty_text(3) == (TEXT[3:], len(TEXT)) and g.read_rtty_text(len(TEXT)) == ("", len(TEXT))
        with pytest.raises(PsdrError) as e:
            g.read_rtty_text(len(TEXT) + 1)
        assert e.value.code == -1 and "beyond" in str(e.value)
        for nm in ("RETUNE", "MODE", "AGAIN"):  # batch 0, then from zero at batch 1: the text count restarts
            w0, w1 = want(nm, (0,)), want(nm, (1, 2))
            same_records(got(nm, (0,)), w0[0], nm), same_records(got(nm, (1, 2)), w1[0], nm)
            assert totals[nm][0] == len(w0[1]) and totals[nm][2] == len(w1[1]), nm
            assert got(nm, (1,))["nchars"][0] == 0 and not got(nm, (1,))["present"][:M.FILL * 16 // h].any(), nm  # the presence fills again
        assert totals["AGAIN"][2] > 0  # (it started inside the idle mark in front of the text's second half)
        # the paused client's state stood still: batch 2 goes on behind batch 0
        same_records(got("PAUSE", (0, 1)), want("PAUSE", (0, 1))[0], "PAUSE")
        same_records(got("IQ", (0,)), want("IQ", (0,))[0], "IQ")
        # a context that never had an RTTY client has launched nothing
        B.ctx.set_profiling(1)
        B.batch(F)
        assert "audio_rtty" not in B.ctx.kernel_stats() or B.ctx.kernel_stats()["audio_rtty"][1] == 0
    finally:
        A.close()
        B.close()
    # an audio_rate outside [4000, 48000]: PSDR_ERR_STATE, and the defaults refuse it
    _, N, _ = SHAPES[SHAPE]
    ctx = Context(N, False, 4, additional_size=n, audio_fft_size=n, audio_rate=3000, input_format="f32", max_batch=8, max_clients=2)
    try:
        g = AudioClient(ctx)
        with pytest.raises(PsdrError) as e:
            g.set_rtty_decoder(True, mark_hz=915.0)
        assert e.value.code == -4 and "audio_rate" in str(e.value)
        g.set_rtty_decoder(False)
    finally:
        ctx.close()


def test_a_from_older_than_the_ring_reads_no_data():
    """the stream over and over until the text is longer than the ring: what was read pass by pass is the truth for the ring's
    last 1024 characters; one character older reads PSDR_ERR_NO_DATA"""
    from phantomsdr_amd import PsdrError
    n = 360
    A = RCtx(n, 2)
    try:
        g = A.add("USB", rtty=CFG)
        text, total = "", 0
        for _ in range(200):
            A.frame = 0
            A.batch(frames_of(n))
            new, total = g.read_rtty_text(since=total)
            text += new
            if total > M.TEXT + 8:
                break
        assert total == len(text) > M.TEXT + 8 and text.startswith(TEXT)
        with pytest.raises(PsdrError) as e:
            g.read_rtty_text(total - M.TEXT - 1)
        assert e.value.code == -7 and "older" in str(e.value)
        assert g.read_rtty_text(total - M.TEXT) == (text[-M.TEXT:], total)
        assert g.read_rtty(frames_of(n))[0][-1] == total
    finally:
        A.close()


# ---- with the others ----------------------------------------------------------------------------------------------------------
def test_tone_cw_and_rtty_on_one_client_in_a_high_slot_give_what_each_gives_alone():
    from phantomsdr_amd import AudioClient
    n, h, S = 360, 180, 128
    keep = (0, 100, 101, 102, 103)
    tone, cw = dict(gate=0, hang_blocks=2), dict(wpm=25.0)
    nf = frames_of(n)
    A = RCtx(n, S)
    try:
        everyone = [AudioClient(A.ctx) for _ in range(S)]
        assert [g.id for g in everyone] == list(range(S))
        for g in everyone:
            if g.id not in keep:
                g.on_close()
        roles = {100: (tone, cw, CFG), 101: (tone, None, None), 102: (None, cw, None), 103: (None, None, CFG)}
        for s, (t, c, r) in roles.items():
            g = everyone[s]
            g.set_audio_range(*WINDOW)
            if t is not None:
                g.set_tone_decoder(True, **t)
            if c is not None:
                g.set_cw_decoder(True, **c)
            if r is not None:
                g.set_rtty_decoder(True, **r)
        out = {s: dict(rows=[], tone=[], cw=[], rtty=[]) for s in roles}
        for F in SPLITS["3 parts"](nf):
            A.batch(F)
            for s, (t, c, r) in roles.items():
                g, o = everyone[s], out[s]
                o["rows"].append(read_client(g, "USB", F))
                if t is not None:
                    o["tone"].append(g.read_tone(F))
                if c is not None:
                    o["cw"].append(g.read_cw(F))
                if r is not None:
                    o["rtty"].append(g.read_rtty(F))
        texts = {s: (everyone[s].read_cw_text() if roles[s][1] is not None else None, everyone[s].read_rtty_text() if roles[s][2] is not None else None) for s in roles}
    finally:
        A.close()
    rows, _, nan = cat(out[100]["rows"])
    for s in (101, 102, 103):
        assert_same_bits(cat(out[s]["rows"]), cat(out[100]["rows"]), f"slots {s} and 100", row_names("USB"))
    for a, b in zip(cat(out[100]["tone"]), cat(out[101]["tone"])):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(cat(out[100]["cw"]), cat(out[102]["cw"])):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(cat(out[100]["rtty"]), cat(out[103]["rtty"])):
        assert a.tobytes() == b.tobytes()
    assert texts[100][0] == texts[102][0] and texts[100][1] == texts[103][1] == (TEXT, len(TEXT))
    # ... and each is its model's on these rows
    want, wtext = model(rows, nan, h, **CFG)
    same_records(rec_of(cat(out[100]["rtty"])), want, "slot 100")
    assert wtext == TEXT
    wcw, wcwtext = cw_model_of(rows, nan, h, **cw)
    assert cw_rec_of(cat(out[100]["cw"])).tobytes() == wcw.tobytes() and texts[100][0] == (wcwtext, len(wcwtext))
    t = np.zeros(len(rows), TM.REC_DTYPE)
    t["tone"], t["level"], t["open"] = cat(out[100]["tone"])
    assert t.tobytes() == TM.records(rows, nan, h, RATE, gate=0, hang=2).tobytes()

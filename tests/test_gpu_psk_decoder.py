"""Per-client PSK31 decoder on the GPU (include/psdr.h: psdr_client_set_psk_decoder, psdr_read_psk, psdr_read_psk_text).

The decoder's input is the client's own rows and NaN flags, read back; tests/psk_model.py's records() - a numpy restatement of the
rule in its own f32 arithmetic - on those rows gives the records and the text, compared as bits: there is no tolerance anywhere.
The decoded client has a twin without the decoder in a second context with the same clients, batches and history.

Input (tests/test_gpu_cw_decoder.py's rig: a 2^12-point IQ transform, audio_rate 12000, a USB client whose window's lower edge is
audio zero): unit noise and, behind 0.75 s of noise alone, a carrier of amplitude 4, 1000 Hz above the window's lower edge in the
raw samples, under the envelope of tests/psk_model.py's sender: 1.5 s of idle reversals with one NaN sample 0.1 s into them, `CQ de`
and LF at 31.25 baud, and the steady carrier to the stream's end."""
import functools

import numpy as np
import pytest

import psk_model as M
import rtty_model as RM
from helpers import assert_same_bits, read_client, row_names
from test_gpu_cw_decoder import L0, SHAPE, WINDOW, cat
from test_gpu_cw_decoder import model as cw_model_of
from test_gpu_cw_decoder import rec_of as cw_rec_of
from test_gpu_squelch import RATE, SHAPES, Ctx, oracle_pcm

pytestmark = pytest.mark.gpu

TEXT, BAUD, CARRIER = "CQ de\n", 31.25, 1000.0
LEAD, IDLE, NAN_AT, TAIL = 0.75, 1.5, 0.85, 0.4
CFG = dict(carrier_hz=CARRIER, baud=BAUD)
SPLITS = {"whole": lambda nf: (nf,), "1 per batch": lambda nf: (1,) * nf, "5+6": lambda nf: (5, 6) * (nf // 11) + ((nf % 11,) if nf % 11 else ()),
          "3 parts": lambda nf: (nf // 3,) * 3}


def bits_of(text, baud, idle):
    """the sent bits without the carrier behind them: idle reversals, the characters"""
    return M.varicode(text, preamble=int(round(idle * baud)), postamble=0)


def frames_of(n, rate=RATE, text=TEXT, baud=BAUD, lead=LEAD, idle=IDLE, tail=TAIL):
    t = lead + len(bits_of(text, baud, idle)) / baud + tail
    return 3 * int(np.ceil(t * rate / (n // 2) / 3))


def psk_raw(n, nf, rate=RATE, text=TEXT, baud=BAUD, carrier=CARRIER, seed=11, nan_at=NAN_AT, lead=LEAD, idle=IDLE):
    """f32 half-frames, flat: unit noise plus the keyed carrier above client bin L0 (the lower edge of the rig's window)"""
    N = SHAPES[SHAPE][1]
    fs = rate * (N // 2) / (n // 2)  # a frame is N / 2 raw samples and n / 2 audio samples
    ns = (nf + 1) * (N // 2)
    rng = np.random.default_rng(seed)
    x = np.empty(ns, np.complex64)
    x.real, x.imag = rng.standard_normal(ns, dtype=np.float32), rng.standard_normal(ns, dtype=np.float32)
    first = int(round(lead * fs))
    bits = bits_of(text, baud, idle)
    bits = bits + [1] * (int(np.ceil((ns - first) * baud / fs)) + 2 - len(bits))  # the carrier to the stream's end
    env = M.envelope(bits, baud, fs)[:ns - first]
    c = L0 + carrier * n / rate  # client bin c of an IQ spectrum is frequency index (c + N/2 + 1) mod N
    w = 2 * np.pi * ((c + N // 2 + 1) % N) / N
    x[first:] += (4.0 * env * np.exp(1j * w * np.arange(len(env), dtype=np.float64))).astype(np.complex64)
    raw = x.view(np.float32)
    raw[2 * int(round(nan_at * fs))] = np.nan
    return raw


@functools.lru_cache(maxsize=None)
def raw_of(n):
    return psk_raw(n, frames_of(n))


class PCtx(Ctx):
    def __init__(self, n, max_clients, maxb=None, **kw):
        super().__init__(SHAPE, n, max_clients, maxb=maxb or frames_of(n), raw=raw_of(n), **kw)

    def add(self, kind="USB", psk=None, rtty=None, cw=None, **kw):
        g = super().add(kind, **kw)
        g.set_audio_range(*WINDOW)  # a sideband window: its lower edge is audio frequency zero
        if psk is not None:
            g.set_psk_decoder(True, **psk)
        if rtty is not None:
            g.set_rtty_decoder(True, **rtty)
        if cw is not None:
            g.set_cw_decoder(True, **cw)
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
    A = PCtx(n, 3)
    try:
        A.add("AM")
        g = A.add("USB", psk=CFG)
        A.ctx.set_profiling(1)
        a, t = [], []
        for F in SPLITS[split](frames_of(n)):
            A.batch(F)
            a.append(read_client(g, "USB", F)), t.append(g.read_psk(F))
        return cat(a), cat(t), g.read_psk_text(), A.ctx.kernel_stats()
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
    ms, cnt = stats["audio_psk"]
    print(f"n {n} split {split}: text {text!r} errors {got['errors'][-1]} offset {got['offset_hz'][-1]} level {got['level'].max():.4g} quality {got['quality'][-1]:.4g}; "
          f"{cnt} launches, {1e3 * ms / max(cnt, 1):.1f} us each")
    same_records(got, want, (n, split))
    assert text == wtext and total == len(wtext) == got["nchars"][-1]
    assert wtext == TEXT and want["errors"][-1] == 0  # the input is decodable: the model alone reads what was sent
    assert got["present"].any() and not got["present"][:int(LEAD * RATE / h)].any()
    assert cnt == len(SPLITS[split](nf))


# ---- the twin -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twin_run(n):
    """context A: a plain PSK client and one with audio blanker, noise reduction and audio filter behind the decoder; context B: the
    same clients without the decoder.  Post chain on."""
    from phantomsdr_amd import design_audio_filter
    sec = [design_audio_filter("highpass", RATE, 300.0)]
    A, B = PCtx(n, 3, post=True), PCtx(n, 3, post=True)
    try:
        cl = []
        for X, pk in ((A, CFG), (B, None)):
            p = X.add("USB", psk=pk)
            q = X.add("USB", psk=pk)
            q.set_audio_blanker("normal"), q.set_noise_reduction("normal"), q.set_audio_filter(sec)
            cl.append((p, q))
        got = [[[] for _ in range(2)] for _ in range(2)]
        for F in SPLITS["3 parts"](frames_of(n)):
            A.batch(F), B.batch(F)
            for x in range(2):
                for i, g in enumerate(cl[x]):
                    got[x][i].append(read_client(g, "USB", F, pcm=True))
        texts = [g.read_psk_text()[0] for g in cl[0]]
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
    A = PCtx(n, 8, maxb=F)
    B = PCtx(n, 2, maxb=F)
    try:
        fill = A.add("AM")
        names = ("KEEP", "RETUNE", "MODE", "AGAIN", "PAUSE", "IQ")
        cl = dict(zip(names, [A.add("USB", psk=CFG) for _ in names[:-1]] + [A.add("USB")]))
        B.add("USB")
        rows, recs, totals = ({nm: [] for nm in names} for _ in range(3))
        for bi in range(3):
            if bi == 1:
                cl["RETUNE"].set_audio_range(L0 - 1, L0 - 0.7, L0 + 99)
                cl["MODE"].set_audio_demodulation("LSB")
                cl["AGAIN"].set_psk_decoder(False), cl["AGAIN"].set_psk_decoder(True, **CFG)
                assert cl["AGAIN"].read_psk_text() == ("", 0)  # the start is pending
                cl["PAUSE"].set_paused(True)
                cl["IQ"].set_psk_decoder(True, **CFG)  # on as USB, then an IQ client: keeps the setting, is not listed
                cl["IQ"].set_audio_demodulation("IQ")
            if bi == 2:
                cl["PAUSE"].set_paused(False)
                cl["IQ"].set_audio_demodulation("USB")
            A.batch(F), B.batch(F)
            for nm in names:
                g = cl[nm]
                if (nm == "PAUSE" and bi == 1) or (nm == "IQ" and bi < 2):
                    with pytest.raises(PsdrError) as e:
                        g.read_psk(F)
                    assert e.value.code == -7, nm  # PSDR_ERR_NO_DATA
                    continue
                a = g.read_audio(F)
                rows[nm].append((a[0], a[2])), recs[nm].append(rec_of(g.read_psk(F))), totals[nm].append(g.read_psk_text()[1])
        for call in (lambda: fill.read_psk(F), fill.read_psk_text):
            with pytest.raises(PsdrError) as e:
                call()
            assert e.value.code == -7
        with pytest.raises(PsdrError) as e:
            cl["IQ"].set_audio_demodulation("IQ"), cl["IQ"].set_psk_decoder(True)
        assert e.value.code == -1 and "PSDR_IQ" in str(e.value)
        for bad in (dict(carrier_hz=299.0), dict(baud=45.45), dict(search_hz=15.625), dict(quality=1.0), dict(quality=float("nan"))):
            with pytest.raises(PsdrError) as e:
                cl["KEEP"].set_psk_decoder(True, **dict(CFG, **bad))
            assert e.value.code == -1 and list(bad)[0] in str(e.value)
        # (at this audio_rate every carrier the call accepts has room for its lanes: tests/test_psk_host.py holds that refusal)

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
        assert g.read_psk_text() == (TEXT, len(TEXT)) and g.read_psk_text(3) == (TEXT[3:], len(TEXT)) and g.read_psk_text(len(TEXT)) == ("", len(TEXT))
        with pytest.raises(PsdrError) as e:
            g.read_psk_text(len(TEXT) + 1)
        assert e.value.code == -1 and "beyond" in str(e.value)
        for nm in ("RETUNE", "MODE", "AGAIN"):  # batch 0, then from zero at batch 1: the text count restarts
            w0, w1 = want(nm, (0,)), want(nm, (1, 2))
            same_records(got(nm, (0,)), w0[0], nm), same_records(got(nm, (1, 2)), w1[0], nm)
            assert totals[nm][0] == len(w0[1]) and totals[nm][2] == len(w1[1]), nm
            assert got(nm, (1,))["nchars"][0] == 0 and not got(nm, (1,))["present"][:int(M.FILL / BAUD * RATE / h) - 2].any(), nm  # the presence fills again
        # the paused client's state stood still: batch 2 goes on behind batch 0
        same_records(got("PAUSE", (0, 1)), want("PAUSE", (0, 1))[0], "PAUSE")
        same_records(got("IQ", (0,)), want("IQ", (0,))[0], "IQ")
        # a context that never had a PSK client has launched nothing
        B.ctx.set_profiling(1)
        B.batch(F)
        assert "audio_psk" not in B.ctx.kernel_stats() or B.ctx.kernel_stats()["audio_psk"][1] == 0
    finally:
        A.close()
        B.close()
    # an audio_rate outside [4000, 48000]: PSDR_ERR_STATE, and the defaults refuse it
    _, N, _ = SHAPES[SHAPE]
    ctx = Context(N, False, 4, additional_size=n, audio_fft_size=n, audio_rate=3000, input_format="f32", max_batch=8, max_clients=2)
    try:
        g = AudioClient(ctx)
        with pytest.raises(PsdrError) as e:
            g.set_psk_decoder(True, carrier_hz=1000.0)
        assert e.value.code == -4 and "audio_rate" in str(e.value)
        g.set_psk_decoder(False)
    finally:
        ctx.close()


def test_a_from_older_than_the_ring_reads_no_data():
    """the stream over and over until the text is longer than the ring: what was read pass by pass is the truth for the ring's
    last 1024 characters; one character older reads PSDR_ERR_NO_DATA"""
    from phantomsdr_amd import PsdrError
    n = 360
    A = PCtx(n, 2)
    try:
        g = A.add("USB", psk=CFG)
        text, total = "", 0
        for _ in range(400):
            A.frame = 0
            A.batch(frames_of(n))
            new, total = g.read_psk_text(since=total)
            text += new
            if total > M.TEXT + 8:
                break
        assert total == len(text) > M.TEXT + 8 and text.startswith(TEXT)
        with pytest.raises(PsdrError) as e:
            g.read_psk_text(total - M.TEXT - 1)
        assert e.value.code == -7 and "older" in str(e.value)
        assert g.read_psk_text(total - M.TEXT) == (text[-M.TEXT:], total)
        assert g.read_psk(frames_of(n))[0][-1] == total
    finally:
        A.close()


# ---- with the others ----------------------------------------------------------------------------------------------------------
def test_cw_rtty_and_psk_on_one_client_in_a_high_slot_give_what_each_gives_alone():
    from phantomsdr_amd import AudioClient
    n, h, S = 360, 180, 128
    keep = (0, 100, 101, 102, 103)
    cw, rtty = dict(wpm=25.0), dict(mark_hz=915.0, shift_hz=170.0, baud=75.0)
    nf = frames_of(n)
    A = PCtx(n, S)
    try:
        everyone = [AudioClient(A.ctx) for _ in range(S)]
        assert [g.id for g in everyone] == list(range(S))
        for g in everyone:
            if g.id not in keep:
                g.on_close()
        roles = {100: (cw, rtty, CFG), 101: (cw, None, None), 102: (None, rtty, None), 103: (None, None, CFG)}
        for s, (c, r, p) in roles.items():
            g = everyone[s]
            g.set_audio_range(*WINDOW)
            if c is not None:
                g.set_cw_decoder(True, **c)
            if r is not None:
                g.set_rtty_decoder(True, **r)
            if p is not None:
                g.set_psk_decoder(True, **p)
        out = {s: dict(rows=[], cw=[], rtty=[], psk=[]) for s in roles}
        for F in SPLITS["3 parts"](nf):
            A.batch(F)
            for s, (c, r, p) in roles.items():
                g, o = everyone[s], out[s]
                o["rows"].append(read_client(g, "USB", F))
                if c is not None:
                    o["cw"].append(g.read_cw(F))
                if r is not None:
                    o["rtty"].append(g.read_rtty(F))
                if p is not None:
                    o["psk"].append(g.read_psk(F))
        texts = {s: (everyone[s].read_cw_text() if roles[s][0] is not None else None, everyone[s].read_rtty_text() if roles[s][1] is not None else None,
                     everyone[s].read_psk_text() if roles[s][2] is not None else None) for s in roles}
    finally:
        A.close()
    rows, _, nan = cat(out[100]["rows"])
    for s in (101, 102, 103):
        assert_same_bits(cat(out[s]["rows"]), cat(out[100]["rows"]), f"slots {s} and 100", row_names("USB"))
    for what, other in (("cw", 101), ("rtty", 102), ("psk", 103)):
        for a, b in zip(cat(out[100][what]), cat(out[other][what])):
            assert a.tobytes() == b.tobytes(), what
    assert texts[100][0] == texts[101][0] and texts[100][1] == texts[102][1] and texts[100][2] == texts[103][2] == (TEXT, len(TEXT))
    # ... and each is its model's on these rows
    want, wtext = model(rows, nan, h, **CFG)
    same_records(rec_of(cat(out[100]["psk"])), want, "slot 100")
    assert wtext == TEXT
    wcw, wcwtext = cw_model_of(rows, nan, h, **cw)
    assert cw_rec_of(cat(out[100]["cw"])).tobytes() == wcw.tobytes() and texts[100][0] == (wcwtext, len(wcwtext))
    wr, wrtext = RM.records(rows, nan, h, RATE, **rtty)
    r = np.zeros(len(rows), RM.REC_DTYPE)
    r["nchars"], r["errors"], r["offset_hz"], r["level"], r["quality"], r["present"] = cat(out[100]["rtty"])
    assert r.tobytes() == wr.tobytes() and texts[100][1] == (wrtext, len(wrtext))

"""Per-client radiofax decoder on the GPU (include/psdr.h: psdr_client_set_fax_decoder, psdr_read_fax, psdr_read_fax_lines).

The decoder's input is the client's own rows and NaN flags, read back; tests/fax_model.py's records() - a numpy restatement of the
rule in its own f32 arithmetic - on those rows gives the records, the kept lines and their meta, compared as bits: there is no
tolerance anywhere.  The decoded client has a twin without the decoder in a second context with the same clients and batches.

Input (tests/decoder_shapes.py's rig: a 2^12-point IQ transform, audio_rate 12000, n = 360, a USB client whose window's lower edge
is audio zero): unit noise and a frequency-keyed carrier of amplitude 4 in the raw samples, tests/fax_model.py's sender: 0.3 s of
noise alone, 1.5 s of 300 Hz start tone, 8 phasing lines, 12 lines of a ramp with a checkerboard, 1.5 s of stop tone, at 240 lines
per minute and 256 pixels; one NaN sample in the second image line."""
import functools

import numpy as np
import pytest

import decoder_shapes as S
import fax_model as M
from helpers import assert_same_bits, read_client, row_names

pytestmark = pytest.mark.gpu

RATE, N_AUDIO, LPM, WIDTH = 12000, 360, 240.0, 256
CFGS = {"auto": dict(mode=M.AUTO, lpm=LPM, width=WIDTH, start_blocks=4, phase_lines=3), "free": dict(mode=M.FREE, lpm=LPM, width=WIDTH)}


def tx_seconds(lpm, lead=0.3, start_s=1.5, phasing=8, lines=12, stop_s=1.5, tail=0.3):
    return lead + start_s + (phasing + lines) * 60.0 / lpm + stop_s + tail


def frames_of(rate, n, seconds):
    return 3 * int(np.ceil(seconds * rate / (n // 2) / 3))


def fax_raw(rate, n, nf, lpm, black_hz=1500.0, white_hz=2300.0, seed=11, nan_at=None, **tx):
    """f32 half-frames, flat: unit noise plus the sender's carrier, audio frequency f above client bin L0"""
    N = S.N
    fs = rate * (N // 2) / (n // 2)  # a frame is N / 2 raw samples and n / 2 audio samples
    ns = (nf + 1) * (N // 2)
    rng = np.random.default_rng(seed)
    x = np.empty(ns, np.complex64)
    x.real, x.imag = rng.standard_normal(ns, dtype=np.float32), rng.standard_normal(ns, dtype=np.float32)
    freq, on = M.tx_freq(fs, M.test_image(tx.pop("lines", 12), 256), lpm=lpm, black_hz=black_hz, white_hz=white_hz, **tx)
    freq, on = freq[:ns], on[:ns]
    # client bin c of an IQ spectrum is frequency index (c + N/2 + 1) mod N; audio frequency f is f n / rate bins above L0
    w = 2 * np.pi * (((S.L0 + N // 2 + 1) % N) + freq * n / rate) / N
    x[:len(w)] += (4.0 * on * np.exp(1j * np.cumsum(w))).astype(np.complex64)
    raw = x.view(np.float32)
    if nan_at is not None:
        raw[2 * int(round(nan_at * fs))] = np.nan
    return raw


NF = frames_of(RATE, N_AUDIO, tx_seconds(LPM))
NAN_AT = 0.3 + 1.5 + 9.5 * 60.0 / LPM


@functools.lru_cache(maxsize=None)
def raw_of():
    return fax_raw(RATE, N_AUDIO, NF, LPM, nan_at=NAN_AT)


def rec_of(t):
    r = np.zeros(len(t[0]), M.REC_DTYPE)
    r["nlines"], r["state"], r["image"], r["ioc"], r["offset_hz"], r["tone_quality"] = t
    return r


def same_records(got, want, what):
    bad = [f for f in range(len(want)) if got[f].tobytes() != want[f].tobytes()]
    assert len(got) == len(want) and not bad, (what, bad[:8], got[bad[:4]], want[bad[:4]])


def batches_of(split, nf=None):
    nf = nf or NF
    return (nf,) if split == "whole" else S.split_of(nf, N_AUDIO // 2)


@functools.lru_cache(maxsize=None)
def records_run(kind, split):
    batches = batches_of(split)
    A = S.open_ctx(RATE, N_AUDIO, max(batches), raw_of())
    try:
        A.add("AM")
        g = A.add("USB")
        g.set_fax_decoder(True, **CFGS[kind])
        A.ctx.set_profiling(1)
        a, t = [], []
        for F in batches:
            A.batch(F)
            a.append(read_client(g, "USB", F)), t.append(g.read_fax(F))
        return S.cat(a), S.cat(t), g.read_fax_lines(), A.ctx.kernel_stats(), batches
    finally:
        A.close()


@functools.lru_cache(maxsize=None)
def model_run(kind):
    (rows, _, nan), _, _, _, _ = records_run(kind, "whole")
    return M.records(rows, nan, N_AUDIO // 2, RATE, **CFGS[kind])


@pytest.mark.parametrize("split", ("whole", "split"))
@pytest.mark.parametrize("kind", ("auto", "free"))
def test_records_lines_and_meta_are_the_models_on_the_clients_own_rows(kind, split):
    (rows, _, nan), t, (lines, meta, total), stats, batches = records_run(kind, split)
    assert rows.shape == (NF, N_AUDIO // 2) and nan.any()
    assert_same_bits((rows, nan), records_run(kind, "whole")[0][::2], "the rows of every split", ("audio", "nan"))
    want, wlines, wmeta = model_run(kind)
    got = rec_of(t)
    ms, cnt = stats["audio_fax"]
    print(f"{kind} {split}: {total} lines, states {sorted(set(got['state']))}, image {got['image'][-1]} ioc {got['ioc'][-1]} offset {got['offset_hz'][-1]:.2f} "
          f"quality {got['tone_quality'].max():.3f}; {cnt} launches, {1e3 * ms / max(cnt, 1):.1f} us each, batches {batches[:8]}")
    same_records(got, want, (kind, split))
    assert total == len(wlines) == got["nlines"][-1] and lines.dtype == np.uint8 and lines.shape == (total, WIDTH)
    assert lines.tobytes() == wlines.tobytes() and meta.tobytes() == wmeta.tobytes()
    assert cnt == len(batches)
    if kind == "auto":  # the input is decodable: the model alone visits the states in order and locks
        st = want["state"]
        assert [int(s) for i, s in enumerate(st) if i == 0 or s != st[i - 1]] == [M.IDLE, M.PHASING, M.IMAGE, M.IDLE]
        assert want["image"][-1] == 1 and want["ioc"][-1] == 576 and 12 <= total <= 18 and (wmeta == (1 << 8 | M.IMAGE)).all()
    else:
        assert (want["state"] == M.IMAGE).all() and total >= 30 and not want["tone_quality"].any()


@functools.lru_cache(maxsize=None)
def launch_times():
    """the launch time of a one-frame batch and of the whole stream in one batch (psdr_set_profiling)"""
    out = {}
    for F in (1, NF):
        A = S.open_ctx(RATE, N_AUDIO, NF, raw_of())
        try:
            g = A.add("USB")
            g.set_fax_decoder(True, **CFGS["auto"])
            A.batch(F)  # (the first launch loads the code)
            A.ctx.set_profiling(1)
            A.frame = 0
            A.batch(F)
            ms, cnt = A.ctx.kernel_stats()["audio_fax"]
            out[F] = 1e3 * ms / cnt
        finally:
            A.close()
    return out


def test_launch_time_is_printed():
    t = launch_times()
    print(f"k_audio_fax: {t[1]:.1f} us for a one-frame batch, {t[NF]:.1f} us for {NF} frames")
    assert t[1] > 0 and t[NF] > 0


# ---- the twin -----------------------------------------------------------------------------------------------------------------
def test_a_twin_without_the_decoder_is_the_same_to_the_bit():
    A, B = S.open_ctx(RATE, N_AUDIO, NF // 3, raw_of(), post=True), S.open_ctx(RATE, N_AUDIO, NF // 3, raw_of(), post=True)
    try:
        cl = []
        for X, on in ((A, True), (B, False)):
            p, q = X.add("USB"), X.add("AM")
            if on:
                p.set_fax_decoder(True, **CFGS["auto"])
            cl.append((p, q))
        B.ctx.set_profiling(1)
        got = [[[] for _ in range(2)] for _ in range(2)]
        for F in (NF // 3,) * 3:
            A.batch(F), B.batch(F)
            for x in range(2):
                for i, (g, kind) in enumerate(zip(cl[x], ("USB", "AM"))):
                    got[x][i].append(read_client(g, kind, F, pcm=True))
        (a, b) = [[S.cat(v) for v in side] for side in got]
        assert cl[0][0].read_fax_lines()[2] >= 12
        stats = B.ctx.kernel_stats()
        assert "audio_fax" not in stats or stats["audio_fax"][1] == 0  # a context without a fax client launches nothing
    finally:
        A.close()
        B.close()
    for i, kind in enumerate(("USB", "AM")):
        assert_same_bits(a[i], b[i], kind, row_names(kind, pcm=True))


# ---- life cycle ---------------------------------------------------------------------------------------------------------------
def test_restart_pause_line_reads_and_errors():
    from phantomsdr_amd import AudioClient, Context, PsdrError
    n, h = N_AUDIO, N_AUDIO // 2
    F = NF // 3
    cfg = CFGS["free"]
    A = S.open_ctx(RATE, n, F, raw_of(), max_clients=8)
    try:
        fill = A.add("AM")
        names = ("KEEP", "RETUNE", "MODE", "AGAIN", "PAUSE", "IQ")
        cl = dict(zip(names, [A.add("USB") for _ in names]))
        for nm in names[:-1]:
            cl[nm].set_fax_decoder(True, **cfg)
        rows, recs, totals = ({nm: [] for nm in names} for _ in range(3))
        for bi in range(3):
            if bi == 1:
                L0 = S.L0
                cl["RETUNE"].set_audio_range(L0 - 1, L0 - 0.7, L0 + 99)
                cl["MODE"].set_audio_demodulation("LSB")
                cl["AGAIN"].set_fax_decoder(False), cl["AGAIN"].set_fax_decoder(True, **cfg)
                assert cl["AGAIN"].read_fax_lines()[2] == 0  # the start is pending
                cl["PAUSE"].set_paused(True)
                cl["IQ"].set_fax_decoder(True, **cfg)  # on as USB, then an IQ client: keeps the setting, is not listed
                cl["IQ"].set_audio_demodulation("IQ")
            if bi == 2:
                cl["PAUSE"].set_paused(False)
                cl["IQ"].set_audio_demodulation("USB")
            A.batch(F)
            for nm in names:
                g = cl[nm]
                if (nm == "PAUSE" and bi == 1) or (nm == "IQ" and bi < 2):
                    with pytest.raises(PsdrError) as e:
                        g.read_fax(F)
                    assert e.value.code == -7, nm  # PSDR_ERR_NO_DATA: paused (not part of the batch), no decoder yet, demodulated as IQ
                    continue
                a = g.read_audio(F)
                rows[nm].append((a[0], a[2])), recs[nm].append(rec_of(g.read_fax(F))), totals[nm].append(g.read_fax_lines()[2])
        for call in (lambda: fill.read_fax(F), fill.read_fax_lines):
            with pytest.raises(PsdrError) as e:
                call()
            assert e.value.code == -7
        with pytest.raises(PsdrError) as e:
            cl["IQ"].set_audio_demodulation("IQ"), cl["IQ"].set_fax_decoder(True)
        assert e.value.code == -1 and "PSDR_IQ" in str(e.value)
        for bad in (dict(black_hz=299.0), dict(lpm=100.0), dict(width=255), dict(tone_ratio=1.0), dict(start_blocks=1), dict(phase_col=WIDTH)):
            with pytest.raises(PsdrError) as e:
                cl["KEEP"].set_fax_decoder(True, **dict(cfg, **bad))
            assert e.value.code == -1 and list(bad)[0].split("_")[0] in str(e.value)

        def want(nm, parts):
            r, f = S.cat([rows[nm][i] for i in parts])
            return M.records(r, f, h, RATE, **cfg)

        def got(nm, parts):
            return np.concatenate([recs[nm][i] for i in parts])

        w, wl, wm = want("KEEP", (0, 1, 2))
        same_records(got("KEEP", (0, 1, 2)), w, "KEEP")
        g = cl["KEEP"]
        lines, meta, total = g.read_fax_lines()
        assert total == len(wl) and lines.tobytes() == wl.tobytes() and meta.tobytes() == wm.tobytes()
        l3, m3, _ = g.read_fax_lines(3)
        assert l3.tobytes() == wl[3:].tobytes() and m3.tobytes() == wm[3:].tobytes() and len(g.read_fax_lines(total)[0]) == 0
        with pytest.raises(PsdrError) as e:
            g.read_fax_lines(total + 1)
        assert e.value.code == -1 and "beyond" in str(e.value)
        for nm in ("RETUNE", "MODE", "AGAIN"):  # batch 0, then from zero at batch 1: the line count restarts
            w0, w1 = want(nm, (0,)), want(nm, (1, 2))
            same_records(got(nm, (0,)), w0[0], nm), same_records(got(nm, (1, 2)), w1[0], nm)
            assert totals[nm][0] == len(w0[1]) and totals[nm][2] == len(w1[1]) and got(nm, (1,))["nlines"][0] == 0, nm
            assert cl[nm].read_fax_lines()[0].tobytes() == w1[1].tobytes(), nm
        # the paused client's state stood still: batch 2 goes on behind batch 0
        same_records(got("PAUSE", (0, 1)), want("PAUSE", (0, 1))[0], "PAUSE")
        same_records(got("IQ", (0,)), want("IQ", (0,))[0], "IQ")
    finally:
        A.close()
    # an audio_rate outside [4000, 48000]: PSDR_ERR_STATE
    ctx = Context(S.N, False, 4, additional_size=n, audio_fft_size=n, audio_rate=3000, input_format="f32", max_batch=8, max_clients=2)
    try:
        g = AudioClient(ctx)
        with pytest.raises(PsdrError) as e:
            g.set_fax_decoder(True, black_hz=500.0, white_hz=900.0)
        assert e.value.code == -4 and "audio_rate" in str(e.value)
        g.set_fax_decoder(False)
    finally:
        ctx.close()


def test_the_ring_wraps_and_a_from_older_than_the_ring_reads_no_data():
    """the stream over and over in FREE mode until more lines are kept than the ring holds: what was read pass by pass is the truth
    for the ring's last R lines; one line older reads PSDR_ERR_NO_DATA"""
    from phantomsdr_amd import PsdrError
    A = S.open_ctx(RATE, N_AUDIO, NF, raw_of())
    try:
        g = A.add("USB")
        g.set_fax_decoder(True, **CFGS["free"])
        R = M.ring_of(M.lq_of(LPM, 0.0, RATE), NF * (N_AUDIO // 2))
        parts, total = [], 0
        for _ in range(12):
            A.frame = 0
            A.batch(NF)
            new, _, total = g.read_fax_lines(total)
            parts.append(new)
            if total > R + 8:
                break
        lines = np.concatenate(parts)
        assert total == len(lines) > R + 8 and R >= 64
        with pytest.raises(PsdrError) as e:
            g.read_fax_lines(total - R - 1)
        assert e.value.code == -7 and "older" in str(e.value)
        got, meta, t2 = g.read_fax_lines(total - R)
        assert t2 == total and got.tobytes() == lines[-R:].tobytes() and (meta == M.IMAGE).all()
        assert g.read_fax(NF)[0][-1] == total
    finally:
        A.close()

"""Per-client audio filter on the GPU (include/psdr.h: psdr_client_set_audio_filter).

Every filtered client has a twin without a filter in the same context, with the same kind, window and history.  The expected
rows are tests/audio_filter_table.cpp's output - the host's run of the blocked evaluation in audiofilterplan.h, the text
k_audio_filter runs - on the TWIN's rows and NaN flags with the same batch lengths: there is no tolerance anywhere, rows are
compared as bits.  Streams, shapes and splits are tests/test_gpu_squelch.py's."""
import functools
import math
from ctypes import POINTER, byref, c_float, c_int32

import numpy as np
import pytest

import audio_filter_model as M
from conftest import ROOT
from helpers import CLIENT_KINDS, assert_same_bits, read_client, row_names, set_client_kind
from test_gpu_squelch import KEY, NF, RATE, SHAPES, SPLITS, STD, Ctx, oracle_pcm, stream

pytestmark = pytest.mark.gpu

AUDIO_KINDS = tuple(k for k in CLIENT_KINDS if CLIENT_KINDS[k][0] != "IQ")
CASES = [("iq12", 360), ("iq12", 124), ("iq12", 8), ("real", 360)]


@functools.lru_cache(maxsize=None)
def presets():
    from phantomsdr_amd import design_audio_filter as d
    return {"two": [d("highpass", RATE, 300.0), d("deemphasis", RATE, 212.0)], "peak": [d("peak", RATE, 700.0, 20.0)],
            "lowpass": [d("lowpass", RATE, 3000.0)]}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gpu_audio_filter")
    exe = M.build_table(tmp, ROOT)
    return lambda jobs: M.run_blocked(exe, tmp, jobs)


class FCtx(Ctx):
    def add(self, kind, sections=None, squelch=None):
        from phantomsdr_amd import AudioClient
        g = AudioClient(self.ctx)
        set_client_kind(g, kind)
        L0 = SHAPES[self.shape][2]
        # (a window is at most audio_fft_size bins wide; both hold the tone on bin L0 + 30)
        g.set_audio_range(*((L0, L0 + 50.3, L0 + 100) if self.n > 100 else (L0 + 28, L0 + 30.3, L0 + 33)))
        if sections is not None:
            g.set_audio_filter(sections)
        if squelch is not None:
            g.set_squelch(True, *squelch)
        return g


def cat(parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(len(parts[0])))


def expect(table, jobs):
    """jobs: [(sections, twin rows [F][h], twin flags [F], batch lengths)] -> filtered rows [F][h]"""
    out = table([(s, rows.reshape(-1), fl, rows.shape[1], list(b)) for s, rows, fl, b in jobs])
    return [o[0].reshape(j[1].shape) for o, j in zip(out, jobs)]


# ---- parity -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def parity_run(shape, n, split):
    """A: per audio kind a client with two sections, one with a peak section and a twin; B: a context that never heard of filters
    with the same 27 clients.  -> per kind: (two, peak, twin, B's twin) as concatenated read_client tuples"""
    P = presets()
    nc = 3 * len(AUDIO_KINDS)
    A, B = FCtx(shape, n, nc + 1), FCtx(shape, n, nc + 1)
    try:
        ga = [(A.add(k, P["two"]), A.add(k, P["peak"]), A.add(k)) for k in AUDIO_KINDS]
        gb = [(B.add(k), B.add(k), B.add(k)) for k in AUDIO_KINDS]
        sizes = SPLITS[split] * (NF // 8)
        got = {k: ([], [], [], []) for k in AUDIO_KINDS}
        for F in sizes:
            A.batch(F), B.batch(F)
            for k, a, b in zip(AUDIO_KINDS, ga, gb):
                for j, g in enumerate(a + (b[2],)):
                    got[k][j].append(read_client(g, k, F))
        return {k: tuple(cat(v) for v in got[k]) for k in AUDIO_KINDS}, sizes
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("shape,n", CASES)
def test_rows_are_the_host_programs_for_every_kind_and_split(table, shape, n, split):
    res, sizes = parity_run(shape, n, split)
    P = presets()
    jobs = []
    for k in AUDIO_KINDS:
        two, peak, twin, other = res[k]
        names = row_names(k)
        assert_same_bits(twin, other, f"{k}: the twin against a context without filters", names)
        assert (twin[2] != 0).any() and (twin[2] == 0).any(), "the stream holds NaN frames"
        for nm, f in (("two", two), ("peak", peak)):
            assert_same_bits(f[1:], twin[1:], f"{k} {nm}: pwr, flags, carrier records", names[1:])
        jobs += [(P["two"], twin[0], twin[2], sizes), (P["peak"], twin[0], twin[2], sizes)]
    want = expect(table, jobs)
    for i, k in enumerate(AUDIO_KINDS):
        two, peak, twin, _ = res[k]
        for nm, f, w in (("two", two, want[2 * i]), ("peak", peak, want[2 * i + 1])):
            bad = [fr for fr in range(NF) if f[0][fr].tobytes() != w[fr].tobytes()]
            assert not bad, (k, nm, "frames that differ from the host program", bad[:8])
            flagged = twin[2] != 0
            assert f[0][flagged].tobytes() == twin[0][flagged].tobytes(), (k, nm, "a flagged frame's row was touched")
            assert f[0][~flagged].tobytes() != twin[0][~flagged].tobytes(), (k, nm, "nothing was filtered")


# ---- lifecycle at batch boundaries --------------------------------------------------------------------------------------------
def test_lifecycle(table):
    """eight batches of 4 frames; every client has a twin that does the same without a filter"""
    P = presets()
    two, peak = P["two"], P["peak"]
    names = ("ON", "NEW", "OFF", "PAUSE", "MODE", "IQ", "TIQ", "READD")
    start = dict(ON=("USB", None), NEW=("AM", two), OFF=("FM", two), PAUSE=("USB", two), MODE=("USB", two), IQ=("IQ", two), TIQ=("TIQ", two), READD=("AM", two))
    A = FCtx("iq12", 360, 2 * len(names))
    try:
        g = {nm: A.add(*start[nm]) for nm in names}
        t = {nm: A.add(start[nm][0]) for nm in names}
        kind = {nm: start[nm][0] for nm in names}
        rows = {nm: [] for nm in names}  # per batch: (filtered client's tuple, twin's tuple) or None while paused
        for b in range(8):
            if b == 2:
                g["ON"].set_audio_filter(two)
                for c in (g["MODE"], t["MODE"]):
                    set_client_kind(c, "FM")
                kind["MODE"] = "FM"
            if b == 3:
                for c in (g["MODE"], t["MODE"]):
                    set_client_kind(c, "USB")
                kind["MODE"] = "USB"
                g["NEW"].set_audio_filter(peak)
                g["PAUSE"].set_paused(True), t["PAUSE"].set_paused(True)
            if b == 4:
                g["OFF"].set_audio_filter([])
                g["PAUSE"].set_paused(False), t["PAUSE"].set_paused(False)
                for nm in ("IQ", "TIQ"):
                    for c in (g[nm], t[nm]):
                        set_client_kind(c, "USB")
                    kind[nm] = "USB"
                for d in (g, t):
                    slot = d["READD"].id
                    A.ctx.lib.psdr_client_remove(A.ctx.h, slot)
                    d["READD"] = A.add("AM")
                    assert d["READD"].id == slot
            A.batch(4)
            for nm in names:
                if nm == "PAUSE" and b == 3:
                    rows[nm].append(None)
                    continue
                rows[nm].append((read_client(g[nm], kind[nm], 4), read_client(t[nm], kind[nm], 4)))
    finally:
        A.close()

    def twin_rows(nm, batches):
        return np.concatenate([rows[nm][b][1][0] for b in batches]), np.concatenate([rows[nm][b][1][2] for b in batches])

    def got_rows(nm, batches):
        return np.concatenate([rows[nm][b][0][0] for b in batches])

    def same_as_twin(nm, batches):
        for b in batches:
            assert_same_bits(rows[nm][b][0], rows[nm][b][1], f"{nm} batch {b}: the twin's bits")

    runs = [("ON", two, range(2, 8)), ("NEW", two, range(0, 3)), ("NEW", peak, range(3, 8)), ("OFF", two, range(0, 4)),
            ("PAUSE", two, [0, 1, 2, 4, 5, 6, 7]), ("MODE", two, range(0, 8)), ("IQ", two, range(4, 8)), ("TIQ", two, range(4, 8)), ("READD", two, range(0, 4))]
    jobs = []
    for nm, sec, bs in runs:
        r, fl = twin_rows(nm, bs)
        jobs.append((sec, r, fl, [4] * len(list(bs))))
    for (nm, sec, bs), w in zip(runs, expect(table, jobs)):
        assert got_rows(nm, bs).tobytes() == w.tobytes(), (nm, list(bs))
        for b in bs:  # pwr and flags are the twin's
            assert_same_bits(rows[nm][b][0][1:], rows[nm][b][1][1:], f"{nm} batch {b}")
    same_as_twin("ON", range(0, 2))      # not yet on
    same_as_twin("OFF", range(4, 8))     # off: the twin's bits again
    same_as_twin("IQ", range(0, 4))      # an IQ client with a setting: untouched
    same_as_twin("TIQ", range(0, 4))
    same_as_twin("READD", range(4, 8))   # remove + add on the same slot: no filter
    # (the carried state matters: a run that starts over gives other bits - looked for in front of the NaN frames 18 and 19, whose
    # 360 zeros let any state decay below the rows' last place)
    r, fl = twin_rows("MODE", [3])
    assert expect(table, [(two, r, fl, [4])])[0].tobytes() != got_rows("MODE", [3]).tobytes()
    r, fl = twin_rows("PAUSE", [4])
    assert expect(table, [(two, r, fl, [4])])[0].tobytes() != got_rows("PAUSE", [4]).tobytes()


# ---- silence ------------------------------------------------------------------------------------------------------------------
def test_silence_decays_through_subnormals_to_zero(table):
    raw = stream("iq12").copy()
    N = SHAPES["iq12"][1]
    raw[2 * 6 * (N // 2):] = 0  # zeros behind half-frame 6 (and no NaN any more)
    lp = presets()["lowpass"]
    A = FCtx("iq12", 360, 4, raw=raw)
    try:
        cl = [(k, A.add(k, lp), A.add(k)) for k in ("USB", "AM")]
        parts = {k: ([], []) for k, _, _ in cl}
        for b in range(4):
            A.batch(8)
            for k, g, t in cl:
                parts[k][0].append(read_client(g, k, 8)), parts[k][1].append(read_client(t, k, 8))
    finally:
        A.close()
    tiny = np.finfo(np.float32).tiny
    for k in parts:
        f, t = cat(parts[k][0]), cat(parts[k][1])
        assert not t[2].any() and t[0][:5].any() and not t[0][8:].any(), "the twin's rows: a signal, then exact zeros"
        w, = expect(table, [(lp, t[0], t[2], [8] * 4)])
        assert f[0].tobytes() == w.tobytes(), k
        assert ((f[0] != 0) & (np.abs(f[0]) < tiny)).any() and not f[0][-8:].any(), (k, "subnormals are kept, then the state is zero")


# ---- the post chain -----------------------------------------------------------------------------------------------------------
CHAIN_KEY = tuple(KEY[:32] * 4 + [0])
NFC = len(CHAIN_KEY) - 1


@pytest.mark.parametrize("n,agc,pcm16", [(n, agc, p16) for n in (360, 128) for agc in (1, 0) for p16 in (0, 1)])
def test_chain_hears_the_filtered_rows(table, n, agc, pcm16):
    """the chain's PCM is the oracle's chain on the host-filtered twin rows; one client sits out a batch (a work-group gathers);
    a squelch client on top: closed frames are dropped as before.  (With AGC on k_pc_ma2 is DIRECT here only in the batches whose
    streams are all whole - no NaN frame, the FM gate open throughout, nobody paused; test_chain_in_the_direct_form has it in
    every batch.)"""
    two = presets()["two"]
    raw = stream("iq", CHAIN_KEY)
    A = FCtx("iq", n, 8, post=True, agc=agc, pcm16=pcm16, raw=raw)
    try:
        spec = [("USB", False, None), ("AM", True, None), ("FM", False, STD), ("SAM", False, None)]  # (kind, paused for batch 5, squelch)
        cl = [(k, p, sq, A.add(k, two, sq), A.add(k, None, sq)) for k, p, sq in spec]
        out = [dict(f=[], t=[], open=[], at=[]) for _ in cl]
        for b in range(NFC // 8):
            for k, p, sq, g, t in cl:
                if p:
                    g.set_paused(b == 5), t.set_paused(b == 5)
            A.batch(8)
            for o, (k, p, sq, g, t) in zip(out, cl):
                if p and b == 5:
                    continue
                o["f"].append(read_client(g, k, 8, pcm=True)), o["t"].append(read_client(t, k, 8, pcm=True))
                o["open"].append(g.read_squelch(8).copy()), o["at"].append(8)
                assert np.array_equal(o["open"][-1], t.read_squelch(8))
    finally:
        A.close()
    total = 0
    for o, (k, p, sq, _, _) in zip(out, cl):
        f, t, opened = cat(o["f"]), cat(o["t"]), np.concatenate(o["open"])
        w, = expect(table, [(two, t[0], t[2], o["at"])])
        assert f[0].tobytes() == w.tobytes(), k
        assert_same_bits(f[1:-1], t[1:-1], f"{k}: pwr, flags, carrier records", row_names(k)[1:])
        keep = (opened == 1) & (f[2] == 0)
        want = oracle_pcm(w, keep, n // 2)
        pcm = f[-1]
        assert not pcm[~keep].any(), (k, "a closed or NaN frame has PCM")
        bad = [fr for fr in range(len(pcm)) if not np.array_equal(pcm[fr], want[fr])]
        assert not bad, (k, bad[:8])
        assert not np.array_equal(pcm, t[-1]), (k, "the chain did not see the filter")
        if sq is not None:
            assert (opened == 0).any() and (opened == 1).any()
        total += int(np.count_nonzero(want))
    assert total > 1000, "the chain was not exercised"


@pytest.mark.parametrize("n,pcm16", [(360, 0), (360, 1), (128, 0)])
def test_chain_in_the_direct_form(table, n, pcm16):
    """AGC on, no squelch client, nobody paused, no NaN frame: every stream of every work-group is whole in every batch, so
    k_pc_ma2 reads the filtered rows themselves (DIRECT) throughout - the plan's form is asked of the library by name"""
    from ctypes import c_int
    two = presets()["two"]
    A = FCtx("iq", n, 4, post=True, agc=1, pcm16=pcm16, raw=stream("iq", CHAIN_KEY, None))
    try:
        cl = [(k, A.add(k, two), A.add(k)) for k in ("USB", "FM")]
        out = [dict(f=[], t=[]) for _ in cl]
        for b in range(NFC // 8):
            A.batch(8)
            direct = c_int(-1)
            assert A.ctx.lib.psdr_debug_post_direct(A.ctx.h, byref(direct)) == 0 and direct.value == 1, (b, direct.value)
            for o, (k, g, t) in zip(out, cl):
                o["f"].append(read_client(g, k, 8, pcm=True)), o["t"].append(read_client(t, k, 8, pcm=True))
    finally:
        A.close()
    for o, (k, _, _) in zip(out, cl):
        f, t = cat(o["f"]), cat(o["t"])
        assert not t[2].any(), "no NaN frame"
        w, = expect(table, [(two, t[0], t[2], [8] * (NFC // 8))])
        assert f[0].tobytes() == w.tobytes(), k
        want = oracle_pcm(w, np.ones(NFC, bool), n // 2)
        bad = [fr for fr in range(NFC) if not np.array_equal(f[-1][fr], want[fr])]
        assert not bad and np.count_nonzero(want) > 1000, (k, bad[:8])
        assert not np.array_equal(f[-1], t[-1]), (k, "the chain did not see the filter")


# ---- fetch --------------------------------------------------------------------------------------------------------------------
def test_fetch_delivers_the_filtered_rows():
    two = presets()["two"]
    A = FCtx("iq12", 360, 4)
    try:
        cl = [A.add("USB", two), A.add("AM"), A.add("FM", presets()["peak"])]
        h = 180
        A.batch(8)
        for b in range(3):  # pipelined: the copies of batch b run beside batch b + 1
            A.ctx.fetch_begin(A.ctx.FETCH_AUDIO)
            want = [g.read_audio(8) for g in cl]
            if b < 2:
                A.batch(8)
            A.ctx.fetch_end()
            for g, w in zip(cl, want):
                for fr in range(8):
                    p, pw, nf = POINTER(c_float)(), c_float(), c_int32()
                    assert A.ctx.lib.psdr_fetched_audio(A.ctx.h, g.id, fr, byref(p), byref(pw), byref(nf), None) == 0
                    got = np.ctypeslib.as_array(p, (h,)).copy()
                    assert got.tobytes() == w[0][fr].tobytes() and nf.value == w[2][fr]
    finally:
        A.close()


# ---- refusals, profiling ------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_no_filter_no_trace():
    from phantomsdr_amd import _lib
    A = FCtx("iq12", 360, 4)
    try:
        g, t = A.add("USB"), A.add("USB")
        lib, hh = A.ctx.lib, A.ctx.h
        arr = lambda *secs: (_lib.psdr_biquad * len(secs))(*[_lib.psdr_biquad(*s) for s in secs])  # noqa: E731
        good = (0.2, 0.4, 0.2, -0.5, 0.3)
        bad = [(3, 1, arr(good)), (-1, 1, arr(good)), (g.id, 3, arr(good, good, good)), (g.id, -1, arr(good)), (g.id, 1, None), (g.id, 2, None),
               (g.id, 1, arr((1.0, math.nan, 0.0, -0.5, 0.3))), (g.id, 1, arr((1.0, 0.0, 0.0, -0.5, math.inf))), (g.id, 1, arr((1.0, 0.0, 0.0, -1.96, 0.95))),
               (g.id, 1, arr((1.0, 0.0, 0.0, 0.0, 1.0))), (g.id, 1, arr((1.0, 0.0, 0.0, -1.9, 0.9995))), (g.id, 2, arr(good, (1.0, 0.0, 0.0, -0.9996, 0.0))), (3, 0, None)]
        A.ctx.set_profiling(1)

        def allocated():
            from ctypes import c_void_p
            ptrs = (c_void_p * 2)()
            assert lib.psdr_debug_audio_filter_ptrs(hh, ptrs) == 0
            assert bool(ptrs[0]) == bool(ptrs[1])  # table and state: both or none
            return bool(ptrs[0])
        for i, n, p in bad:
            assert lib.psdr_client_set_audio_filter(hh, i, n, p) == -1, (i, n)  # PSDR_ERR_INVALID
            assert b"audio" in lib.psdr_last_error() or b"client" in lib.psdr_last_error()
            assert not allocated(), (i, n, "a refused call allocated")
        assert lib.psdr_client_set_audio_filter(hh, g.id, 0, None) == 0 and not allocated()  # off needs nothing either
        A.batch(8)
        A.ctx.synchronize()
        assert_same_bits(g.read_audio(8), t.read_audio(8), "after the refused calls")
        assert "audio_filter" not in A.ctx.kernel_stats()  # no filter client: nothing was launched
        g.set_audio_filter([good])
        assert allocated()
        A.batch(8)
        A.ctx.synchronize()
        assert A.ctx.kernel_stats()["audio_filter"][1] == 1
        assert g.read_audio(8)[0].tobytes() != t.read_audio(8)[0].tobytes()
        for i, n, p in bad:
            assert lib.psdr_client_set_audio_filter(hh, i, n, p) == -1
        g.set_audio_filter([])  # off and accepted at the limit
        assert lib.psdr_client_set_audio_filter(hh, g.id, 0, None) == 0
        A.batch(8)
        assert_same_bits(g.read_audio(8), t.read_audio(8), "off again")
    finally:
        A.close()

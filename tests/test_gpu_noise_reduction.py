"""Per-client noise reduction on the GPU (include/psdr.h: psdr_client_set_noise_reduction).

Every noise-reduction client has a twin without it in the same context and batch, with the same kind, window and history
(tests/test_gpu_mixed_clients.py: the twin's rows are bit-identical to what k_audio_nr reads).  The expected rows are
tests/nr_plan_table.cpp's output - the host's run of nr_stream in nrplan.h, the text k_audio_nr runs - on the TWIN's rows and NaN
flags with the same batch lengths: there is no tolerance anywhere, rows are compared as the bits of their words."""
import functools
from ctypes import POINTER, byref, c_double, c_int

import numpy as np
import pytest

import audio_filter_model as AF
import nr_model as M
from conftest import ROOT
from helpers import CLIENT_KINDS, assert_same_bits, read_client, set_client_kind
from test_gpu_squelch import RATE, SHAPES, Ctx, oracle_pcm, stream

pytestmark = pytest.mark.gpu

SHAPES.setdefault("real13", (True, 1 << 13, 1000))  # (stream() looks its shapes up by name)
AUDIO_KINDS = tuple(k for k in CLIENT_KINDS if CLIENT_KINDS[k][0] != "IQ")
SIZES = (1, 3, 70)          # the batches, in sequence: the state is carried, the stream ends inside a block
NF = sum(SIZES)
NAN_HALF = 40               # one NaN sample: frames 39 and 40 are flagged, in mid-stream
KEY = tuple(1 if (i // 5) % 3 else 0 for i in range(NF + 1))
CASES = [("iq12", 8), ("iq12", 12), ("iq12", 360), ("real13", 8), ("real13", 360)]
NORMAL = (14.0, 1.5)


def raw_of(shape):
    return stream(shape, key=KEY, nan_half=NAN_HALF)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_nr")


@pytest.fixture(scope="module")
def table(tmp):
    exe = M.build_table(tmp, ROOT)
    return lambda jobs: M.run_streams(exe, tmp, jobs, rate=RATE)


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_words(got, want, what):
    g, w = words(got), words(want)
    assert g.shape == w.shape, what
    bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
    assert not len(bad), (what, "frames that differ from the host program", bad[:8].tolist())


class NCtx(Ctx):
    def __init__(self, shape, n, max_clients, **kw):
        super().__init__(shape, n, max_clients, maxb=max(SIZES), raw=raw_of(shape), **kw)

    def add(self, kind, nr=None, sections=None):
        from phantomsdr_amd import AudioClient
        g = AudioClient(self.ctx)
        set_client_kind(g, kind)
        L0 = SHAPES[self.shape][2]
        g.set_audio_range(*((L0, L0 + 50.3, L0 + 100) if self.n > 100 else (L0 + 28, L0 + 30.3, L0 + 31 + self.n // 4)))
        if nr is not None:
            g.set_noise_reduction("normal", *nr)
        if sections is not None:
            g.set_audio_filter(sections)
        return g


def expect(table, jobs):
    """jobs: [(depth, beta, twin rows [F][h], twin flags [F], batch lengths)] -> reduced rows [F][h]"""
    out = table([(d, b, rows.reshape(-1), fl, rows.shape[1], list(bl)) for d, b, rows, fl, bl in jobs])
    return [o[0].reshape(j[2].shape) for o, j in zip(out, jobs)]


def cat(parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(len(parts[0])))


# ---- every kind, both store widths, the carried state -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def parity_run(shape, n):
    """per audio kind a twin and, behind all the twins, a noise-reduction client: the last one sits in the highest slot"""
    A = NCtx(shape, n, 2 * len(AUDIO_KINDS))
    try:
        tw = [A.add(k) for k in AUDIO_KINDS]
        nr = [A.add(k, NORMAL) for k in AUDIO_KINDS]
        assert nr[-1].id == 2 * len(AUDIO_KINDS) - 1
        got = {k: ([], []) for k in AUDIO_KINDS}
        for F in SIZES:
            A.batch(F)
            for k, a, b in zip(AUDIO_KINDS, nr, tw):
                got[k][0].append(read_client(a, k, F)), got[k][1].append(read_client(b, k, F))
        stats = A.ctx.kernel_stats()
        return {k: (cat(v[0]), cat(v[1])) for k, v in got.items()}, stats
    finally:
        A.close()


@pytest.mark.parametrize("shape,n", CASES)
def test_rows_are_the_host_programs_for_every_kind(table, shape, n):
    res, _ = parity_run(shape, n)
    want = expect(table, [NORMAL + (res[k][1][0], res[k][1][2], SIZES) for k in AUDIO_KINDS])
    for k, w in zip(AUDIO_KINDS, want):
        got, twin = res[k]
        flagged = twin[2] != 0
        assert flagged.any() and not flagged.all(), "the stream holds NaN frames in its middle"
        assert_same_bits(got[1:], twin[1:], f"{k}: pwr, flags, carrier records", ("pwr", "nan flags", "carrier level", "carrier offset"))
        same_words(got[0], w, (shape, n, k))
        assert got[0][flagged].tobytes() == twin[0][flagged].tobytes(), (k, "a flagged frame's row was touched")
        assert got[0][~flagged].tobytes() != twin[0][~flagged].tobytes(), (k, "nothing was reduced")
        assert not words(got[0].reshape(-1)[:M.M][~np.repeat(flagged, n // 2)[:M.M]]).any(), (k, "the first 256 outputs are +0.0")


# ---- lifecycle at batch boundaries ----------------------------------------------------------------------------------------------
def test_lifecycle(table):
    """eight batches of 3 frames at h = 180; every client has a twin that does the same without noise reduction"""
    names = ("PAUSE", "MODE", "TUNE", "OFFON", "LATE")
    kind0 = dict(PAUSE="USB", MODE="USB", TUNE="AM", OFFON="FM", LATE="LSB")
    A = NCtx("iq12", 360, 2 * len(names))
    L0 = SHAPES["iq12"][2]
    try:
        g = {nm: A.add(kind0[nm], None if nm == "LATE" else NORMAL) for nm in names}
        t = {nm: A.add(kind0[nm]) for nm in names}
        kind = dict(kind0)
        rows = {nm: [] for nm in names}
        for b in range(8):
            if b == 3:
                g["PAUSE"].set_paused(True), t["PAUSE"].set_paused(True)
                for c in (g["MODE"], t["MODE"]):
                    set_client_kind(c, "AM")
                kind["MODE"] = "AM"
                for c in (g["TUNE"], t["TUNE"]):
                    c.set_audio_range(L0 + 10, L0 + 60.3, L0 + 110)
                g["OFFON"].set_noise_reduction(None)
                g["LATE"].set_noise_reduction("strong")
            if b == 4:
                g["PAUSE"].set_paused(False), t["PAUSE"].set_paused(False)
            if b == 5:
                g["OFFON"].set_noise_reduction("normal")
            A.batch(3)
            for nm in names:
                rows[nm].append(None if nm == "PAUSE" and b == 3 else (read_client(g[nm], kind[nm], 3), read_client(t[nm], kind[nm], 3)))
    finally:
        A.close()

    def twin(nm, bs):
        return np.concatenate([rows[nm][b][1][0] for b in bs]), np.concatenate([rows[nm][b][1][2] for b in bs])

    def got(nm, bs):
        return np.concatenate([rows[nm][b][0][0] for b in bs])

    strong = (22.0, 2.0)
    # a pause carries the state; a mode change, a retune and switching on again are resets: a stream of its own from there
    runs = [("PAUSE", NORMAL, [0, 1, 2, 4, 5, 6, 7]), ("MODE", NORMAL, [0, 1, 2]), ("MODE", NORMAL, [3, 4, 5, 6, 7]), ("TUNE", NORMAL, [0, 1, 2]),
            ("TUNE", NORMAL, [3, 4, 5, 6, 7]), ("OFFON", NORMAL, [0, 1, 2]), ("OFFON", NORMAL, [5, 6, 7]), ("LATE", strong, [3, 4, 5, 6, 7])]
    want = expect(table, [par + twin(nm, bs) + ([3] * len(bs),) for nm, par, bs in runs])
    for (nm, par, bs), w in zip(runs, want):
        same_words(got(nm, bs), w, (nm, bs))
    for nm, bs in (("OFFON", [3, 4]), ("LATE", [0, 1, 2])):  # off: the twin's bits
        for b in bs:
            assert_same_bits(rows[nm][b][0], rows[nm][b][1], f"{nm} batch {b}: the twin's bits")


# ---- in front of the audio filter, the post chain and the fetches ---------------------------------------------------------------
@pytest.mark.parametrize("n", (12, 360))
def test_the_audio_filter_sees_the_reduced_rows(table, tmp, n):
    from phantomsdr_amd import design_audio_filter as d
    sec = [d("highpass", RATE, 300.0), d("deemphasis", RATE, 212.0)]
    A = NCtx("iq12", n, 2)
    try:
        both, tw = A.add("USB", NORMAL, sec), A.add("USB")
        parts = ([], [])
        for F in SIZES:
            A.batch(F)
            parts[0].append(read_client(both, "USB", F)), parts[1].append(read_client(tw, "USB", F))
        stats = A.ctx.kernel_stats()
    finally:
        A.close()
    got, twin = cat(parts[0]), cat(parts[1])
    (reduced,) = expect(table, [NORMAL + (twin[0], twin[2], SIZES)])
    exe = AF.build_table(tmp, ROOT)
    (filtered, _), = AF.run_blocked(exe, tmp, [(sec, reduced.reshape(-1), twin[2], n // 2, list(SIZES))])
    same_words(got[0], filtered.reshape(got[0].shape), ("nr_stream then af_stream", n))
    assert "audio_nr" not in stats  # (profiling is off: no launch is counted)


@pytest.mark.parametrize("n", (12, 360))
def test_the_post_chain_and_the_fetches_read_the_reduced_rows(table, n):
    A = NCtx("iq12", n, 2, post=True)
    try:
        g, tw = A.add("AM", NORMAL), A.add("AM")
        parts, fetched = ([], []), []
        for F in SIZES:
            A.batch(F)
            A.ctx.fetch_begin(A.ctx.FETCH_AUDIO)
            A.ctx.fetch_end()
            fetched.append(np.stack([A.ctx.fetched_audio(g.id, f)[0] for f in range(F)]))
            parts[0].append(read_client(g, "AM", F, pcm=True)), parts[1].append(read_client(tw, "AM", F, pcm=True))
    finally:
        A.close()
    got, twin = cat(parts[0]), cat(parts[1])
    (reduced,) = expect(table, [NORMAL + (twin[0], twin[2], SIZES)])
    same_words(got[0], reduced, ("rows", n))
    same_words(np.concatenate(fetched), reduced, ("psdr_fetched_audio", n))
    keep = twin[2] == 0
    assert np.array_equal(got[3], oracle_pcm(np.where(keep[:, None], reduced, 0), keep, n // 2)), "the PCM is the oracle's chain over the reduced rows"


# ---- a context that never switches it on ----------------------------------------------------------------------------------------
def test_never_switched_on_launches_nothing_and_changes_nothing():
    def run(touch):
        A = NCtx("iq12", 360, 4)
        try:
            if touch:  # every call that allocates and launches nothing: refused ones, the preset, switching off
                A.ctx.set_option(A.ctx.OPT_NOISE_REDUCTION, 0)
            g = [A.add(k) for k in ("USB", "AM", "FM")]
            if touch:
                g[0].set_noise_reduction(None)
            A.ctx.set_profiling(1)
            out = []
            for F in SIZES:
                A.batch(F)
                out.append([read_client(c, k, F) for c, k in zip(g, ("USB", "AM", "FM"))])
            ptrs = (POINTER(c_int) * 2)()
            assert A.ctx.lib.psdr_debug_noise_reduction_ptrs(A.ctx.h, ptrs) == 0
            return out, A.ctx.kernel_stats(), [bool(p) for p in ptrs]
        finally:
            A.close()
    (a, sa, pa), (b, sb, pb) = run(False), run(True)
    assert "audio_nr" not in sa and "audio_nr" not in sb and pa == pb == [False, False]  # nothing launched, nothing allocated
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert_same_bits(u, v, "a context that never switched noise reduction on")


def test_switched_on_launches_once_per_batch():
    A = NCtx("iq12", 360, 2)
    try:
        A.ctx.set_option(A.ctx.OPT_NOISE_REDUCTION, 2)  # a new client comes with PSDR_NR_NORMAL
        g = A.add("USB")
        A.ctx.set_profiling(1)
        A.batch(3), A.batch(1)
        g.read_audio(1)
        assert A.ctx.kernel_stats()["audio_nr"][1] == 2
    finally:
        A.close()


# ---- refusals through the C-ABI -------------------------------------------------------------------------------------------------
def test_refusals():
    from phantomsdr_amd import PsdrError, _lib
    A = NCtx("iq12", 360, 4)
    try:
        usb, iq = A.add("USB"), A.add("IQ")
        lib, h = A.ctx.lib, A.ctx.h

        def refused(args, text, code=-1):
            rc = lib.psdr_client_set_noise_reduction(h, args[0], args[1], c_double(args[2]), c_double(args[3]))
            assert rc == code and text in lib.psdr_last_error().decode(), (args, rc, lib.psdr_last_error())
        refused((-1, 1, 14, 1.5), "outside 0..3"), refused((4, 1, 14, 1.5), "outside 0..3")
        refused((3, 1, 14, 1.5), "no audio client with id 3"), refused((3, 0, 0, 0), "no audio client with id 3")
        refused((iq.id, 1, 14, 1.5), "PSDR_IQ client")
        refused((usb.id, 1, float("nan"), 1.5), "not a finite number"), refused((usb.id, 1, 14, float("inf")), "not a finite number")
        refused((usb.id, 1, -1, 1.5), "depth_db -1 outside [0, 40]"), refused((usb.id, 1, 41, 1.5), "depth_db 41 outside [0, 40]")
        refused((usb.id, 1, 14, 0.4), "beta 0.4 outside [0.5, 4]"), refused((usb.id, 1, 14, 5), "beta 5 outside [0.5, 4]")
        refused((usb.id, 1, float("nan"), 9), "not a finite number"), refused((usb.id, 1, 99, 9), "depth_db 99")  # the order
        for v in (-1, 4):
            with pytest.raises(PsdrError):
                A.ctx.set_option(A.ctx.OPT_NOISE_REDUCTION, v)
        d, b = c_double(0), c_double(0)
        assert lib.psdr_noise_reduction_preset(0, byref(d), byref(b)) == -1 and lib.psdr_noise_reduction_preset(2, None, byref(b)) == -1
        assert lib.psdr_noise_reduction_preset(3, byref(d), byref(b)) == 0 and (d.value, b.value) == (22.0, 2.0)
        assert lib.psdr_client_set_noise_reduction(h, iq.id, 0, c_double(0), c_double(0)) == 0  # an IQ client may switch it off
        assert _lib is not None
    finally:
        A.close()

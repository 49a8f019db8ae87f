"""Per-client audio blanker on the GPU (include/psdr.h: psdr_client_set_audio_blanker).

Every blanker client has a twin without it in the same context and batch, with the same kind, window and history
(tests/test_gpu_noise_reduction.py's scheme: the twin's rows are bit-identical to what k_audio_nb reads).  The expected rows are
tests/anb_plan_table.cpp's output - the host's run of anb_stream in anbplan.h, the text k_audio_nb runs - on the TWIN's rows and NaN
flags with the same batch lengths: there is no tolerance anywhere, rows are compared as the bits of their words."""
import functools
import json
import os
from ctypes import POINTER, byref, c_double, c_int, c_uint64

import numpy as np
import pytest

import anb_model as M
import audio_filter_model as AF
import nr_model as NR
from conftest import ROOT
from helpers import CLIENT_KINDS, assert_same_bits, read_client, set_client_kind
from test_gpu_squelch import RATE, SHAPES, Ctx, oracle_pcm, stream

pytestmark = pytest.mark.gpu

SHAPES.setdefault("real13", (True, 1 << 13, 1000))  # (stream() looks its shapes up by name)
AUDIO_KINDS = tuple(k for k in CLIENT_KINDS if CLIENT_KINDS[k][0] != "IQ")
# the batches, in sequence.  The state is carried; the stream passes the delay by more than two blocks and ends inside a block;
# many batch boundaries, so that gaps cross some; one batch of several groups of four blocks
SIZES_SMALL = (1, 3) + (37,) * 8 + (320,)   # h = 4: 2480 samples, h = 6: 3720
SIZES_180 = (1, 3) + (5,) * 6 + (40,)       # 13320 samples
CASES = [("iq12", 8), ("iq12", 12), ("iq12", 360), ("real13", 8), ("real13", 360)]
PARITY = (2.0, 15)   # the threshold's minimum - plain noise yields detections in nearly every block - and the widest gap
NORMAL = (4.5, 7)


def sizes_of(n):
    return SIZES_180 if n == 360 else SIZES_SMALL


def raw_of(shape, n):
    nf = sum(sizes_of(n))
    key = tuple(1 if (i // 5) % 3 else 0 for i in range(nf + 1))
    return stream(shape, key=key, nan_half=40 if n == 360 else 150)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_anb")


@pytest.fixture(scope="module")
def table(tmp):
    exe = M.build_table(tmp, ROOT)
    return lambda jobs: M.run_streams(exe, tmp, jobs)


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_words(got, want, what):
    g, w = words(got), words(want)
    assert g.shape == w.shape, what
    bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
    assert not len(bad), (what, "frames that differ from the host program", bad[:8].tolist())


class BCtx(Ctx):
    def __init__(self, shape, n, max_clients, **kw):
        super().__init__(shape, n, max_clients, maxb=max(sizes_of(n)), raw=raw_of(shape, n), **kw)

    def add(self, kind, nb=None, nr=None, sections=None):
        from phantomsdr_amd import AudioClient
        g = AudioClient(self.ctx)
        set_client_kind(g, kind)
        L0 = SHAPES[self.shape][2]
        g.set_audio_range(*((L0, L0 + 50.3, L0 + 100) if self.n > 100 else (L0 + 28, L0 + 30.3, L0 + 31 + self.n // 4)))
        if nb is not None:
            g.set_audio_blanker("normal", *nb)
        if nr is not None:
            g.set_noise_reduction("normal", *nr)
        if sections is not None:
            g.set_audio_filter(sections)
        return g


def expect(table, jobs):
    """jobs: [(threshold, width, twin rows [F][h], twin flags [F], batch lengths)] -> [(rows [F][h], last state, trace)]"""
    out = table([(t, w, rows.reshape(-1), fl, rows.shape[1], list(bl)) for t, w, rows, fl, bl in jobs])
    return [(o[0].reshape(j[2].shape), o[1][-1], o[2]) for o, j in zip(out, jobs)]


def cat(parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(len(parts[0])))


def record(name, **figures):
    d = os.path.join(ROOT, "build", "records")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "anb_gpu.jsonl"), "a") as f:
        f.write(json.dumps(dict(test=name, **figures)) + "\n")


# ---- every kind, both store widths, the carried state -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def parity_run(shape, n):
    """per audio kind a twin and, behind all the twins, a blanker client: the last one sits in the highest slot.  With the h = 180
    run one more pair, for the cost: a noise reduction client, so that both kernels are timed in one context"""
    A = BCtx(shape, n, 2 * len(AUDIO_KINDS) + 1)
    try:
        tw = [A.add(k) for k in AUDIO_KINDS]
        nrc = A.add("USB", nr=(14.0, 1.5))
        nb = [A.add(k, PARITY) for k in AUDIO_KINDS]
        assert nb[-1].id == 2 * len(AUDIO_KINDS)
        A.ctx.set_profiling(1)
        got = {k: ([], []) for k in AUDIO_KINDS}
        counts = {}
        for F in sizes_of(n):
            A.batch(F)
            for k, a, b in zip(AUDIO_KINDS, nb, tw):
                got[k][0].append(read_client(a, k, F)), got[k][1].append(read_client(b, k, F))
        for k, a in zip(AUDIO_KINDS, nb):
            counts[k] = a.audio_blanker_counts()
        nrc.read_audio(sizes_of(n)[-1])
        stats = A.ctx.kernel_stats()
        return {k: (cat(v[0]), cat(v[1])) for k, v in got.items()}, counts, stats
    finally:
        A.close()


@pytest.mark.parametrize("shape,n", CASES)
def test_rows_and_totals_are_the_host_programs_for_every_kind(table, shape, n):
    res, counts, _ = parity_run(shape, n)
    sizes, h = sizes_of(n), n // 2
    want = expect(table, [PARITY + (res[k][1][0], res[k][1][2], sizes) for k in AUDIO_KINDS])
    bounds = np.cumsum([s * h for s in sizes])[:-1]
    pl = (PARITY[1] - 1) // 2
    for k, (w, st, tr) in zip(AUDIO_KINDS, want):
        got, twin = res[k]
        flagged = twin[2] != 0
        assert flagged.any() and not flagged.all(), "the stream holds NaN frames in its middle"
        # the host program's run is worth comparing against: gaps, one across a block boundary, one across a batch boundary
        c = tr["centres"]
        lo, hi = c - pl, c + pl
        assert len(c) >= 8, (k, len(c))
        assert np.any(lo // M.B != hi // M.B), (k, "no gap crosses a block boundary")
        assert np.any((lo[:, None] < bounds[None, :]) & (hi[:, None] >= bounds[None, :])), (k, "no gap crosses a batch boundary")
        assert len(w) * h >= M.D + 2 * M.B and (len(w) * h) % M.B != 0
        assert_same_bits(got[1:], twin[1:], f"{k}: pwr, flags, carrier records", ("pwr", "nan flags", "carrier level", "carrier offset"))
        same_words(got[0], w, (shape, n, k))
        assert got[0][flagged].tobytes() == twin[0][flagged].tobytes(), (k, "a flagged frame's row was touched")
        first = got[0].reshape(-1)[:M.D][~np.repeat(flagged, h)[:M.D]]
        assert not words(first).any(), (k, "the first 536 outputs are +0.0")
        assert counts[k] == (int(st["impulses"]), int(st["samples"])) and counts[k][0] == len(c), (k, counts[k])


def test_cost_beside_the_noise_reduction():
    """no bound: a time at this size says nothing about the step (the instruction count is the cost)"""
    _, _, stats = parity_run("iq12", 360)
    nb_ms, nb_n = stats["audio_nb"]
    nr_ms, nr_n = stats["audio_nr"]
    assert nb_n == nr_n == len(SIZES_180)
    fig = dict(h=180, batches=list(SIZES_180), nb_clients=len(AUDIO_KINDS), nr_clients=1, audio_nb_ms_per_launch=nb_ms / nb_n, audio_nr_ms_per_launch=nr_ms / nr_n,
               audio_nb_us_per_client_launch=1e3 * nb_ms / nb_n / len(AUDIO_KINDS), audio_nr_us_per_client_launch=1e3 * nr_ms / nr_n)
    print(fig)
    record("cost", **fig)


# ---- lifecycle at batch boundaries ----------------------------------------------------------------------------------------------
def test_lifecycle(table):
    """ten batches of 10 frames at h = 180 (every stretch passes the delay); every client has a twin that does the same without"""
    names = ("PAUSE", "MODE", "TUNE", "OFFON", "LATE", "OPT")
    kind0 = dict(PAUSE="USB", MODE="USB", TUNE="AM", OFFON="FM", LATE="LSB", OPT="USB")
    A = BCtx("iq12", 360, 2 * len(names))
    L0 = SHAPES["iq12"][2]
    NB, F = 10, 6
    try:
        g = {nm: A.add(kind0[nm], None if nm == "LATE" else PARITY) for nm in names if nm != "OPT"}
        A.ctx.set_option(A.ctx.OPT_AUDIO_BLANKER, 3)  # a new client comes with PSDR_ANB_STRONG; existing clients keep theirs
        g["OPT"] = A.add("USB")
        A.ctx.set_option(A.ctx.OPT_AUDIO_BLANKER, 0)
        t = {nm: A.add(kind0[nm]) for nm in names}
        kind = dict(kind0)
        rows = {nm: [] for nm in names}
        for b in range(NB):
            if b == 4:
                g["PAUSE"].set_paused(True), t["PAUSE"].set_paused(True)
                for c in (g["MODE"], t["MODE"]):
                    set_client_kind(c, "AM")
                kind["MODE"] = "AM"
                for c in (g["TUNE"], t["TUNE"]):
                    c.set_audio_range(L0 + 10, L0 + 60.3, L0 + 110)
                g["OFFON"].set_audio_blanker(None)
                g["LATE"].set_audio_blanker("strong")
            if b == 5:
                g["PAUSE"].set_paused(False), t["PAUSE"].set_paused(False)
                g["OFFON"].set_audio_blanker("normal", *PARITY)
            A.batch(F)
            for nm in names:
                rows[nm].append(None if nm == "PAUSE" and b == 4 else (read_client(g[nm], kind[nm], F), read_client(t[nm], kind[nm], F)))
    finally:
        A.close()

    def twin(nm, bs):
        return np.concatenate([rows[nm][b][1][0] for b in bs]), np.concatenate([rows[nm][b][1][2] for b in bs])

    def got(nm, bs):
        return np.concatenate([rows[nm][b][0][0] for b in bs])

    strong = (3.5, 11)
    early, late = list(range(4)), list(range(4, NB))
    # a pause carries the state; a mode change, a retune and switching on again are resets: a stream of its own from there
    runs = [("PAUSE", PARITY, early + late[1:]), ("MODE", PARITY, early), ("MODE", PARITY, late), ("TUNE", PARITY, early), ("TUNE", PARITY, late),
            ("OFFON", PARITY, early), ("OFFON", PARITY, late[1:]), ("LATE", strong, late), ("OPT", strong, early + late)]
    want = expect(table, [par + twin(nm, bs) + ([F] * len(bs),) for nm, par, bs in runs])
    for (nm, par, bs), (w, st, tr) in zip(runs, want):
        same_words(got(nm, bs), w, (nm, bs))
        if len(bs) * F * 180 >= M.D + 2 * M.B and par == PARITY:
            assert len(tr["centres"]) > 0, (nm, bs)
    for nm, bs in (("OFFON", [4]), ("LATE", early)):  # off: the twin's bits
        for b in bs:
            assert_same_bits(rows[nm][b][0], rows[nm][b][1], f"{nm} batch {b}: the twin's bits")


# ---- in front of the noise reduction, the audio filter and the post chain -------------------------------------------------------
@pytest.mark.parametrize("n", (12, 360))
def test_the_chain_blanker_noise_reduction_audio_filter_post_chain(table, tmp, n):
    from phantomsdr_amd import design_audio_filter as d
    sec = [d("highpass", RATE, 300.0), d("deemphasis", RATE, 212.0)]
    nrp = (14.0, 1.5)
    sizes = sizes_of(n)
    A = BCtx("iq12", n, 2, post=True)
    try:
        allc, tw = A.add("AM", PARITY, nrp, sec), A.add("AM")
        parts = ([], [])
        for F in sizes:
            A.batch(F)
            parts[0].append(read_client(allc, "AM", F, pcm=True)), parts[1].append(read_client(tw, "AM", F, pcm=True))
    finally:
        A.close()
    got, twin = cat(parts[0]), cat(parts[1])
    ((blanked, _, tr),) = expect(table, [PARITY + (twin[0], twin[2], sizes)])
    assert len(tr["centres"]) >= 8
    nr_exe = NR.build_table(tmp, ROOT)
    ((reduced, _, _),) = NR.run_streams(nr_exe, tmp, [nrp + (blanked.reshape(-1), twin[2], n // 2, list(sizes))], rate=RATE)
    af_exe = AF.build_table(tmp, ROOT)
    (filtered, _), = AF.run_blocked(af_exe, tmp, [(sec, reduced, twin[2], n // 2, list(sizes))])
    filtered = filtered.reshape(got[0].shape)
    same_words(got[0], filtered, ("anb_stream, nr_stream, then af_stream", n))
    keep = twin[2] == 0
    assert np.array_equal(got[3], oracle_pcm(np.where(keep[:, None], filtered, 0), keep, n // 2)), "the PCM is the oracle's chain over the processed rows"


# ---- a context that never switches it on ----------------------------------------------------------------------------------------
def test_never_switched_on_launches_nothing_and_changes_nothing():
    def run(touch):
        A = BCtx("iq12", 360, 4)
        try:
            if touch:  # every call that allocates and launches nothing: refused ones, the preset, switching off
                A.ctx.set_option(A.ctx.OPT_AUDIO_BLANKER, 0)
            g = [A.add(k) for k in ("USB", "AM", "FM")]
            if touch:
                g[0].set_audio_blanker(None)
                assert A.ctx.lib.psdr_client_set_audio_blanker(A.ctx.h, g[1].id, 1, c_double(1.0), 7) == -1
            A.ctx.set_profiling(1)
            out = []
            for F in SIZES_180[:4]:
                A.batch(F)
                out.append([read_client(c, k, F) for c, k in zip(g, ("USB", "AM", "FM"))])
            ptrs = (POINTER(c_int) * 2)()
            assert A.ctx.lib.psdr_debug_audio_blanker_ptrs(A.ctx.h, ptrs) == 0
            return out, A.ctx.kernel_stats(), [bool(p) for p in ptrs]
        finally:
            A.close()
    (a, sa, pa), (b, sb, pb) = run(False), run(True)
    assert "audio_nb" not in sa and "audio_nb" not in sb and pa == pb == [False, False]  # nothing launched, nothing allocated
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert_same_bits(u, v, "a context that never switched the audio blanker on")


def test_switched_on_launches_once_per_batch_in_front_of_nothing_else():
    A = BCtx("iq12", 360, 2)
    try:
        A.ctx.set_option(A.ctx.OPT_AUDIO_BLANKER, 2)  # a new client comes with PSDR_ANB_NORMAL
        g = A.add("USB")
        A.ctx.set_profiling(1)
        A.batch(3), A.batch(1)
        g.read_audio(1)
        stats = A.ctx.kernel_stats()
        assert stats["audio_nb"][1] == 2 and "audio_nr" not in stats
        n, smp = g.audio_blanker_counts()  # (720 samples: two blocks are complete)
        assert 0 <= n <= 32 and n * 3 <= smp <= n * 7
    finally:
        A.close()


# ---- refusals through the C-ABI -------------------------------------------------------------------------------------------------
def test_refusals():
    from phantomsdr_amd import PsdrError
    A = BCtx("iq12", 360, 4)
    NO_DATA = -7
    try:
        usb, iq = A.add("USB"), A.add("IQ")
        lib, h = A.ctx.lib, A.ctx.h

        def refused(args, text, code=-1):
            rc = lib.psdr_client_set_audio_blanker(h, args[0], args[1], c_double(args[2]), args[3])
            assert rc == code and text in lib.psdr_last_error().decode(), (args, rc, lib.psdr_last_error())
        refused((-1, 1, 4.5, 7), "outside 0..3"), refused((4, 1, 4.5, 7), "outside 0..3")
        refused((3, 1, 4.5, 7), "no audio client with id 3"), refused((3, 0, 0, 0), "no audio client with id 3")
        refused((iq.id, 1, 4.5, 7), "PSDR_IQ client")
        refused((usb.id, 1, float("nan"), 7), "not a finite number"), refused((usb.id, 1, float("inf"), 7), "not a finite number")
        refused((usb.id, 1, 1.9, 7), "threshold 1.9 outside [2, 12]"), refused((usb.id, 1, 12.5, 7), "threshold 12.5 outside [2, 12]")
        for wd in (1, 4, 17, -3):
            refused((usb.id, 1, 4.5, wd), "width %d is not an odd number in 3..15" % wd)
        refused((iq.id, 1, float("nan"), 4), "PSDR_IQ client"), refused((usb.id, 1, float("nan"), 4), "not a finite number")  # the order
        refused((usb.id, 1, 99, 4), "threshold 99")
        for v in (-1, 4):
            with pytest.raises(PsdrError):
                A.ctx.set_option(A.ctx.OPT_AUDIO_BLANKER, v)
        t, w = c_double(0), c_int(0)
        assert lib.psdr_audio_blanker_preset(0, byref(t), byref(w)) == -1 and lib.psdr_audio_blanker_preset(2, None, byref(w)) == -1
        assert lib.psdr_audio_blanker_preset(3, byref(t), byref(w)) == 0 and (t.value, w.value) == (3.5, 11)
        assert lib.psdr_client_set_audio_blanker(h, iq.id, 0, c_double(0), 0) == 0  # an IQ client may switch it off
        # psdr_read_audio_blanker: psdr_read_audio's rule, and a client without the blanker has nothing to read
        a, b = c_uint64(0), c_uint64(0)
        assert lib.psdr_read_audio_blanker(h, usb.id, byref(a), byref(b)) == NO_DATA  # no batch yet
        assert lib.psdr_read_audio_blanker(h, 7, byref(a), byref(b)) == -1 and lib.psdr_read_audio_blanker(h, usb.id, None, byref(b)) == -1
        A.batch(3)
        assert lib.psdr_read_audio_blanker(h, usb.id, byref(a), byref(b)) == NO_DATA and "no audio blanker" in lib.psdr_last_error().decode()
        assert lib.psdr_read_audio_blanker(h, iq.id, byref(a), byref(b)) == NO_DATA
        usb.set_audio_blanker("light")
        assert lib.psdr_read_audio_blanker(h, usb.id, byref(a), byref(b)) == NO_DATA  # in force from the next batch
        A.batch(3)
        assert lib.psdr_read_audio_blanker(h, usb.id, byref(a), byref(b)) == 0
        usb.set_paused(True)
        A.batch(1)
        assert lib.psdr_read_audio_blanker(h, usb.id, byref(a), byref(b)) == NO_DATA
    finally:
        A.close()

"""The band scan on the GPU (include/psdr.h: psdr_scan_set).  Every expectation is tests/scan_model.py - the rule in numpy
integers - fed the GPU's OWN ctx.read_quantized(f) of every frame, so trace, floors, list and total are compared bit for bit and
the comparison does not depend on FFT rounding.  The inputs carry signals whose runs are known by construction - a narrow tone, a
wide signal, one across a segment border, one at each band edge, two tones `gap` and `gap + 1` cold bins apart - and the tests
assert that the model finds exactly those among its runs: a scan that listed nothing would fail them.  The oracle's pyramid of
the same frames (CPU) is held to the same expectation at the smallest shape and for the comb."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import quantize_raw

import scan_model as M

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

THR, GAP, SHIFT = 40, 2, 2  # 20 dB above the floor; a tone under the Hann window is 3 bins wide
SIGMA, AMP = 2.0 ** -9, 0.02
# client bins at level 0 (every shape here has at least 4096): (centre bins of the tones, the run they must give)
NARROW = ([1000], (999, 1002))
WIDE = (list(range(2000, 2012)), (1999, 2013))
BORDER = ([255, 256], (254, 258))
PAIR_JOINED = ([3000, 3000 + 3 + GAP], (2999, 3000 + 3 + GAP + 2))          # GAP cold bins between the two: one run
PAIR_SPLIT = ([3500, 3500 + 4 + GAP], (3499, 3502), (3500 + 3 + GAP, 3500 + 6 + GAP))  # GAP + 1: two runs


def tones(R):
    return NARROW[0] + WIDE[0] + BORDER[0] + PAIR_JOINED[0] + PAIR_SPLIT[0] + [0, R - 1]


def expected_runs(R):
    """the runs the signals give at level 0; the two edge tones leak one bin across the band's end"""
    return [NARROW[1], WIDE[1], BORDER[1], PAIR_JOINED[1], PAIR_SPLIT[1], PAIR_SPLIT[2]]


@functools.lru_cache(maxsize=None)
def stream(N, is_real, nframes, seed=3):
    """noise + the tones, exactly on bin centres, as raw s16"""
    h = N // 2
    ns = (nframes + 1) * h
    rng = np.random.default_rng(seed)
    t = np.arange(ns, dtype=np.float64)
    R = h if is_real else N
    if is_real:
        x = rng.standard_normal(ns) * SIGMA
        for c in tones(R):
            x += 2 * AMP * np.cos(2 * np.pi * (c / N) * t + rng.uniform(0, 6.28))
    else:
        x = (rng.standard_normal(ns) + 1j * rng.standard_normal(ns)) * SIGMA
        for c in tones(R):
            k = (c + N // 2 + 1) % N  # client bin c is bin k of the transform
            x += AMP * np.exp(1j * (2 * np.pi * ((k * t) % N) / N + rng.uniform(0, 6.28)))
    return quantize_raw(x, "s16", bool(is_real))


def levels_for(R, floor_bins=256):
    lv = 0
    while (R >> lv) >= floor_bins:
        lv += 1
    return lv


class Rig:
    """one context and its stream; batch() processes frames, reports them to psdr_scan_batch and keeps what the model needs"""

    def __init__(self, N, is_real, F, nframes, raw=None, levels=None, **kw):
        from phantomsdr_amd import Context
        self.N, self.is_real = N, is_real
        self.R = N // 2 if is_real else N
        self.levels = levels or levels_for(self.R)
        self.ctx = Context(N, is_real, self.levels, input_format="s16", max_batch=F, **kw)
        raw = stream(N, is_real, nframes) if raw is None else raw
        self.d = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.d, raw)
        self.s, self.next, self.cfg = None, None, None

    def set(self, level, avg_shift=SHIFT, threshold=THR, gap=GAP):
        self.ctx.scan_set(level, avg_shift, threshold, gap)
        self.cfg, self.s, self.next = (level, avg_shift, threshold, gap), None, None

    def process(self, start, nf):
        self.ctx.process_batch(self.d, nf, offset_bytes=start * self.ctx.half_frame_bytes())
        self.nf = nf

    def scan(self, first, read=True):
        """psdr_scan_batch for the batch just processed, and the model's step from the GPU's own int8 values.  read=False: the
        call alone - nothing is read back, no stream is waited for and the model's trace stays as it is (the caller's matter)"""
        level, a, _, _ = self.cfg
        self.ctx.scan_batch(first)
        if not read:
            self.next, self.last = first + self.nf, first + self.nf - 1
            return None
        q = np.stack([self.ctx.quantized_level(self.ctx.read_quantized(f), level) for f in range(self.nf)])
        fresh = self.next is None or first != self.next
        self.s = M.trace(self.s, q, fresh, a)
        self.next, self.last = first + self.nf, first + self.nf - 1
        return q

    def batch(self, start, nf, first=None):
        self.process(start, nf)
        return self.scan(start if first is None else first)

    def check(self, tag=""):
        """trace, floors, list, total and frame number against the model; returns the model's runs"""
        _, _, thr, gap = self.cfg
        F, runs = M.runs(self.s, thr, gap)
        got_s = self.ctx.read_scan_trace()
        assert got_s.dtype == np.uint16 and np.array_equal(got_s, self.s), (tag, int((got_s != self.s).sum()))
        assert np.array_equal(self.ctx.read_scan_floor(), F), tag
        sig, total, fn = self.ctx.read_signals()
        want, passed, wtotal = M.listed(runs)
        assert total == wtotal and fn == self.last, (tag, total, wtotal, fn, self.last)
        assert len(sig) == passed and np.array_equal(sig.astype(M.SIGNAL), want), (tag, len(sig), passed)
        return runs

    def close(self):
        self.ctx.dev_free(self.d)
        self.ctx.close()


def assert_signals_found(runs, R, tag=""):
    have = {(int(r["first"]), int(r["end"])) for r in runs}
    for want in expected_runs(R):
        assert want in have, (tag, want, sorted(have)[:40])
    assert any(f == 0 for f, _ in have) and any(e == R for _, e in have), (tag, "band edges")


def oracle_frames(N, is_real, nframes, levels, raw):
    from oracle import oracle as O
    hv = O.convert(raw, "s16")
    hv = (hv if is_real else hv.view(np.complex64)).reshape(nframes + 1, N // 2)
    fo = O.FFT(N, is_real, levels, 0, 0)
    out = []
    for f in range(nframes):
        fo.load(hv[f], hv[f + 1])
        fo.execute()
        out.append(np.array(fo.quantized(), np.int8))
    return out


# ---- smallest shapes, every address form --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,is_real", [(1 << 12, False), (1 << 13, True)])
def test_smallest_shape_every_level(N, is_real):
    """IQ 2^12: levels 0 .. 4 cover the tiled records (level 0 .. tiled_lt), the first level-major level and the level with one
    segment (n = 256); real 2^13 has no tiled records at all"""
    rig = Rig(N, is_real, 3, 6)
    R = rig.R
    assert R == 4096 and rig.levels == 5
    try:
        for level in range(5):
            rig.set(level)
            for k, (start, nf) in enumerate(((0, 2), (2, 1), (3, 3))):
                rig.batch(start, nf)
                runs = rig.check(f"level {level} batch {k}")
            if level == 0:
                assert_signals_found(runs, R, "gpu values")
            if level == 4:
                assert len(rig.ctx.read_scan_floor()) == 1
        # the CPU's pyramid of the same frames gives the same signals
        oq = oracle_frames(N, is_real, 6, rig.levels, stream(N, is_real, 6))
        s = M.trace(None, np.stack([q[:R] for q in oq]), True, SHIFT)
        assert_signals_found(M.runs(s, THR, GAP)[1], R, "oracle values")
    finally:
        rig.close()


# ---- large tiled layouts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,is_real,levels_tested", [(1 << 20, False, (0, 3, 5)), (1 << 21, True, (0, 2, 4))])
def test_large_tiled_layouts(N, is_real, levels_tested):
    """IQ 2^20: tile-major lines, tiled_lt = 4 (levels 0 and 3 tiled, 5 level-major); fused real 2^21: record pairs, tiled_lt = 3"""
    rig = Rig(N, is_real, 2, 3, levels=11)
    try:
        for level in levels_tested:
            rig.set(level)
            rig.batch(0, 2)
            rig.batch(2, 1)
            runs = rig.check(f"level {level}")
            if level == 0:
                assert_signals_found(runs, rig.R)
    finally:
        rig.close()


# ---- runs of frames -----------------------------------------------------------------------------------------------------------
def test_split_invariance():
    results = []
    for split in ((1,) * 12, (5, 7), (12,)):
        rig = Rig(1 << 12, False, 12, 12)
        try:
            rig.set(0, avg_shift=3)
            at = 0
            for nf in split:
                rig.batch(at, nf)
                at += nf
            rig.check(str(split))
            results.append((rig.ctx.read_scan_trace(), rig.ctx.read_scan_floor(), rig.ctx.read_signals()))
        finally:
            rig.close()
    for tr, fl, (sig, total, fn) in results[1:]:
        assert np.array_equal(tr, results[0][0]) and np.array_equal(fl, results[0][1])
        assert np.array_equal(sig, results[0][2][0]) and (total, fn) == results[0][2][1:] and fn == 11


def test_run_restart():
    rig = Rig(1 << 12, False, 4, 12)
    try:
        rig.set(1, avg_shift=4)
        rig.batch(0, 4)
        rig.batch(4, 2)
        rig.check("continued")
        continued = rig.s.copy()
        q = rig.batch(6, 3, first=100)  # a jump in first_frame_num: the trace starts again from this batch's first frame
        rig.check("jump")
        assert np.array_equal(rig.s, M.trace(None, q, True, 4)) and not np.array_equal(rig.s, M.trace(continued, q, False, 4))
        rig.batch(9, 1, first=103)      # ... and goes on from there
        rig.check("after the jump")
        rig.set(1, avg_shift=4)         # a second psdr_scan_set: a new run although the frame numbers go on
        with pytest.raises(Exception) as e:
            rig.ctx.read_scan_trace()
        assert e.value.code == -7
        q = rig.batch(10, 2, first=104)
        rig.check("second set")
        assert np.array_equal(rig.s, M.trace(None, q, True, 4))
    finally:
        rig.close()


# ---- cap and long run ---------------------------------------------------------------------------------------------------------
def test_cap_and_one_run_over_the_band():
    """impulses every N/4 samples: under the Hann window three bins of every four are up and one is at zero.  The impulses
    alternate in sign, which moves the comb by two bins: with same-sign impulses the zero falls on client bins 1 mod 4, the band
    starts in the middle of a group of three and has 16 385 runs; this way the zeros are the client bins 3 mod 4.  gap = 0:
    16 384 runs, of which the list holds the first 8192; gap = 1: one run over the band, by the same kernels within the same time"""
    N = 1 << 16
    x = np.zeros(2 * (N // 2), np.complex128)
    x[::N // 4] = 0.5 * (-1.0) ** np.arange(4)
    raw = quantize_raw(x, "s16", False)
    rig = Rig(N, False, 1, 1, raw=raw, levels=7)
    try:
        rig.set(0, avg_shift=0, threshold=THR, gap=0)
        q = rig.batch(0, 1)[0]
        oq = oracle_frames(N, False, 1, 7, raw)[0][:N]
        for name, v in (("gpu", q), ("oracle", oq)):  # the comb is what the docstring says, on the CPU too
            up = v.astype(int) > -128 + THR
            assert np.array_equal(up.reshape(-1, 4), np.tile(up[:4], (N // 4, 1))) and up[:4].sum() == 3, name
            assert len(M.runs(M.trace(None, v[None], True, 0), THR, 0)[1]) == N // 4, name
        runs = rig.check("gap 0")
        sig, total, _ = rig.ctx.read_signals()
        assert len(runs) == total == N // 4 and len(sig) == M.CAP
        sig3, total3, _ = rig.ctx.read_signals(min_width=4)
        assert len(sig3) == 0 and total3 == N // 4
        rig.set(0, avg_shift=0, threshold=THR, gap=1)
        rig.scan(0)  # the same batch again under the new setting
        runs = rig.check("gap 1")
        assert len(runs) == 1 and int(runs[0]["end"]) - int(runs[0]["first"]) >= N - 2
    finally:
        rig.close()


# ---- nothing else changes -----------------------------------------------------------------------------------------------------
def test_every_other_output_is_unchanged():
    from phantomsdr_amd import AudioClient, WaterfallClient
    N, F = 1 << 16, 4
    out = []
    for scan in (False, True):
        rig = Rig(N, False, F, F, levels=7, audio_fft_size=248, max_clients=2, max_waterfall_clients=2)
        try:
            ctx = rig.ctx
            ctx.set_profiling(1)
            a = AudioClient(ctx)
            a.set_audio_demodulation("USB")
            a.set_audio_range(33768 + 200, 33768 + 200.0, 33768 + 260)
            w = WaterfallClient(ctx)
            w.set_waterfall_range(1, 100, 3000)
            if scan:
                rig.set(0)
            rows = []
            for start in (0, 2):
                rig.process(start, 2)
                if scan:
                    rig.scan(start)
                ctx.waterfall_batch(start)
                ctx.demod_batch(start)
                rows.append((w.read_waterfall()[0].copy(), [ctx.read_quantized(f) for f in range(2)], [np.array(v) for v in a.read_audio(2)]))
            if scan:
                rig.check("beside the other consumers")
            stats = ctx.kernel_stats()
            out.append((rows, stats))
        finally:
            rig.close()
    (r0, s0), (r1, s1) = out
    for (wa, qa, aa), (wb, qb, ab) in zip(r0, r1):
        assert np.array_equal(wa, wb) and all(np.array_equal(x, y) for x, y in zip(qa, qb))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(aa, ab))
    assert not [k for k in s0 if k.startswith("scan_")], s0
    assert sorted(k for k in s1 if k.startswith("scan_")) == ["scan_emit", "scan_floor", "scan_hot", "scan_mark", "scan_trace"]
    assert all(s1[k][1] == 2 for k in s1 if k.startswith("scan_"))


# ---- error codes --------------------------------------------------------------------------------------------------------------
def test_error_codes():
    from phantomsdr_amd import PsdrError
    rig = Rig(1 << 12, False, 2, 2)
    ctx = rig.ctx

    def code(fn, *a):
        with pytest.raises(PsdrError) as e:
            fn(*a)
        return e.value.code, str(e.value)

    try:
        assert code(ctx.scan_batch, 0)[0] == -4                      # off
        assert code(ctx.read_signals)[0] == -7 and code(ctx.read_scan_floor)[0] == -7 and code(ctx.read_scan_trace)[0] == -7
        texts = []
        for bad in ((5, 9, 0, 65), (-1, 3, 12, 2), (4, 9, 0, 65), (4, 8, 0, 65), (4, 8, 255, 65)):
            c, t = code(ctx.scan_set, *bad)
            assert c == -1
            texts.append(t)
        assert "level" in texts[0] and "avg_shift" in texts[2] and "threshold" in texts[3] and "gap" in texts[4]
        assert code(ctx.scan_batch, 0)[0] == -4                      # a refused call changed nothing: still off
        ctx.scan_set(0)
        assert code(ctx.scan_batch, 0)[0] == -4                      # on, but no batch was processed
        assert code(ctx.read_signals)[0] == -7
        rig.process(0, 2)
        assert code(ctx.read_scan_trace)[0] == -7                    # processed, not yet evaluated
        ctx.scan_batch(0)
        sig, total, fn = ctx.read_signals()
        assert fn == 1 and total >= len(sig) > 0
        assert code(ctx.scan_set, 0, 3, 256, 2)[0] == -1             # refused: setting and results stand
        assert ctx.read_signals()[2] == 1
        ctx.scan_set(None)
        assert code(ctx.read_signals)[0] == -7 and code(ctx.scan_batch, 2)[0] == -4
    finally:
        rig.close()

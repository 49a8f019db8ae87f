"""The inputs of tests/band_scan_masks.py on the CPU oracle's pyramid, without a GPU: every condition that makes
tests/test_gpu_band_scan_masks.py worth running is asserted here on the reference's values alone - the noise masks reach every
counter of cover() somewhere in the sweep, the gap_edges input gives exactly the joined and split blobs its placement predicts, the
decay input lets bins fall for a long time.  A condition that fails here is a fault of the input, not of the scan.  On the same
traces the host table program (tests/scan_plan_table.cpp: the kernels' own steps) is held bit for bit to the model over the whole
sweep: real traces with varying floors, where tests/test_scan_host.py has flat ones."""
import functools
import os
import re

import numpy as np
import pytest

import band_scan_masks as B
import create_plan_table
import scan_model as M
from conftest import ROOT


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("band_scan_masks")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


@functools.lru_cache(maxsize=None)
def oracle_pyramid(name, N, is_real, nframes):
    """int8 [nframes][q_len]: the oracle's pyramid of an input, as tests/test_gpu_band_scan.py's oracle_frames()"""
    from oracle import oracle as O
    raw = getattr(B, name)(N, *(() if name == "decay" else (is_real,)), nframes)
    hv = O.convert(raw, "s16")
    hv = (hv if is_real else hv.view(np.complex64)).reshape(nframes + 1, N // 2)
    fo = O.FFT(N, is_real, B.levels_of(N, is_real), 0, 0)
    out = []
    for f in range(nframes):
        fo.load(hv[f], hv[f + 1])
        fo.execute()
        out.append(np.array(fo.quantized(), np.int8))
    return np.stack(out)


def frames_of(name, N, is_real, nframes, level):
    R = B.bins_of(N, is_real)
    return np.stack([B.level_of(q, R, level) for q in oracle_pyramid(name, N, is_real, nframes)])


def same(exe, tmp, s, thr, gap):
    """the table program against the model on one evaluation"""
    F, runs = M.runs(s, thr, gap)
    t = M.table_eval(exe, tmp, s, thr, gap)
    want, passed, total = M.listed(runs)
    assert np.array_equal(t["Q"], M.quartiles(s)) and np.array_equal(t["F"], F), (thr, gap)
    assert t["total"] == total and np.array_equal(t["list"], runs[:M.CAP]), (thr, gap, t["total"], total)
    assert t["passed"] == passed and np.array_equal(t["out"], want), (thr, gap)


@pytest.mark.parametrize("N,is_real,level", B.SHAPES)
def test_noise_masks_reach_every_counter(exe, tmp, N, is_real, level):
    n = B.bins_of(N, is_real) >> level
    per = B.words_per_thread(n)
    for nf, a in B.NOISE_TRACES:
        q = frames_of("noise", N, is_real, 3, level)[:nf]
        assert q.min() > -128 and q.max() < 127
        s = M.trace(None, q, True, a)
        covers = {(t, g): B.cover(s, t, g, per) for t, g in B.sweep()}
        density = {t: round(float(M.hot_bins(s, M.floors(M.quartiles(s)), t).mean()), 4) for t in B.THRESHOLDS}
        reached = {k: sum(1 for c in covers.values() if c[k]) for k in B.COUNTERS}
        print(f"noise {N} real {is_real} level {level} frames {nf} shift {a}: density {density} pairs reaching {reached}")
        assert not B.broken_rules(n, covers, a), B.broken_rules(n, covers, a)
        assert density[1] > 0.5 and density[16] <= density[8] < density[4] < density[2] < density[1] and density[16] < 0.25 and density[255] == 0
        for t, g in B.sweep():  # the kernels' steps on the host, bit for bit (some 10 ms an evaluation at 131 072 bins)
            same(exe, tmp, s, t, g)


@pytest.mark.parametrize("N,is_real", [(1 << 12, False), (1 << 13, True)])
def test_gap_edges_give_the_predicted_runs(exe, tmp, N, is_real):
    s = M.trace(None, frames_of("gap_edges", N, is_real, 1, 0), True, 0)
    hot = M.hot_bins(s, M.floors(M.quartiles(s)), B.EDGE_THR)
    blobs = np.zeros(B.EDGE_BINS, bool)
    for lo, _ in B.edge_blobs():
        blobs[lo:lo + 3] = True
    assert np.array_equal(hot, blobs), np.flatnonzero(hot != blobs)[:20]  # three hot bins a tone and nothing else
    for gap in B.EDGE_GAPS:
        runs = M.runs(s, B.EDGE_THR, gap)[1]
        assert [(int(r["first"]), int(r["end"])) for r in runs] == B.gap_edge_runs(gap), gap
        same(exe, tmp, s, B.EDGE_THR, gap)
        c = B.cover(s, B.EDGE_THR, gap, 1)
        assert c["cold_eq_gap"] and (c["cold_eq_gap1"] or gap == 64), (gap, c)  # (65 cold bins are the last the placement has)
        if gap >= 62:
            assert c["cold_eq_gap"] >= 2 and c["cold_eq_gap1"] >= 2, (gap, c)
        inside = np.zeros(B.EDGE_BINS, bool)
        for r in runs:
            inside[r["first"]:r["end"]] = True
        word = lambda w: inside[64 * w:64 * w + 64]
        assert not hot[64 * B.ALIGNED_WORD:64 * B.ALIGNED_WORD + 64].any() and not hot[64 * B.BEYOND_WORD:64 * B.BEYOND_WORD + 64].any()
        assert not word(B.BEYOND_WORD).any()
        if gap == 64:
            assert word(B.ALIGNED_WORD).all() and c["cold_words_inside"] == 1
            (r,) = [r for r in runs if r["first"] == 64 * B.ALIGNED_WORD - 3]
            assert r["end"] == 64 * (B.ALIGNED_WORD + 1) + 3 and r["peak_bin"] == 64 * (B.ALIGNED_WORD + 1) + 1  # the upper blob's centre
            assert r["peak"] > s[64 * B.ALIGNED_WORD - 3:64 * B.ALIGNED_WORD].max() and r["peak"] < 255 << 8
        else:
            assert not word(B.ALIGNED_WORD).any() and c["cold_words_inside"] == 0
    # the placement itself: 62 .. 65 cold bins inside two words of a segment, across a segment border, around a whole word
    groups = {g: [(lo, cold) for gg, lo, cold, _ in B.PAIRS if gg == g] for g in ("close", "words", "border", "aligned", "beyond")}
    assert [c for _, c in groups["close"]] == [0, 1, 2, 3, 4, 7, 8, 9]
    for g in ("words", "border"):
        assert [c for _, c in groups[g]] == [62, 63, 64, 65]
    for lo, cold in groups["words"]:
        assert ((lo + 3) >> 6) + 1 == (lo + 2 + cold) >> 6 and lo >> 8 == (lo + 5 + cold) >> 8
    for lo, cold in groups["border"]:
        assert (lo + 3) >> 8 != (lo + 2 + cold) >> 8
    assert [((lo + 2) & 63, (lo + 3 + cold) & 63) for lo, cold in groups["aligned"] + groups["beyond"]] == [(63, 0), (63, 1)]
    firsts = [lo for _, lo, _, _ in B.PAIRS]
    ends = [lo + 6 + cold for _, lo, cold, _ in B.PAIRS]
    assert all(b - a > 80 for a, b in zip(ends, firsts[1:])) and firsts[0] > 65 and ends[-1] < B.EDGE_BINS - 65
    assert M.runs(np.zeros(B.EDGE_BINS, np.int64), B.EDGE_THR, 64)[1].size == 0 and B.gap_edge_runs(0)  # a scan that lists nothing cannot pass


def test_decay_lets_bins_fall_for_a_long_time(exe, tmp):
    N, nf = 1 << 12, B.DECAY_FRAMES
    q = frames_of("decay", N, False, nf, 0)
    on = B.decay_on(nf)
    comb = np.array(B.decay_comb(N))
    assert q[:on, comb].min() > q[on + 1:].max()  # the comb stands above everything that follows it
    for a in B.DECAY_SHIFTS:
        top = M.trace(None, q[:on], True, a)
        s = M.trace(top, q[on:], False, a)
        print(f"decay shift {a}: bins fallen by more than 2^8 steps {B.fallen(top, s)}, comb trace {int(top[comb].min())} -> {int(s[comb].max())}")
        assert B.fallen(top, s) >= len(comb) and np.all(top[comb] - s[comb] > 1 << 8)
        assert np.array_equal(M.table_trace(exe, tmp, top, q[on:], False, a), s)
        # in the test's batches, on the host program: the same bits
        t, at = None, 0
        for k in B.DECAY_BATCHES:
            t = M.table_trace(exe, tmp, t, q[at:at + k], at == 0, a)
            at += k
        assert np.array_equal(t, s)
        same(exe, tmp, s, 12, 2)


def test_the_tables():
    hdr = open(os.path.join(ROOT, "phantomsdr_amd", "csrc", "scan.h")).read()
    assert re.search(r"constexpr int SCAN_MARK_THREADS = (\d+);", hdr).group(1) == str(B.MARK_THREADS)
    assert B.THRESHOLDS == (1, 2, 4, 8, 16, 255) and B.GAPS == (0, 1, 2, 7, 31, 62, 63, 64)
    want = {(1 << 12, False, 0): (4096, 64, 1), (1 << 12, False, 4): (256, 4, 1), (1 << 13, True, 0): (4096, 64, 1), (1 << 13, True, 2): (1024, 16, 1),
            (1 << 17, False, 0): (131072, 2048, 2), (1 << 17, False, 1): (65536, 1024, 1)}
    for N, is_real, level in B.SHAPES:
        n = B.bins_of(N, is_real) >> level
        assert (n, n // 64, B.words_per_thread(n)) == want[(N, is_real, level)]
        assert level < B.levels_of(N, is_real)
    for N, is_real in {(N, r) for N, r, _ in B.SHAPES}:  # psdr_create takes every shape, with the batches the tests use
        create_plan_table.plan(N, int(is_real), levels=B.levels_of(N, is_real), batch=8)
    assert "tied_peaks" in B.noise_rules(4096, 0) and "tied_peaks" not in B.noise_rules(4096, 3)
    assert B.noise_rules(131072) == B.noise_rules(4096) + ["stretch_border_runs", "over_cap", "cap_inside_word"]
    assert B.noise_rules(65536) == B.noise_rules(4096) + ["over_cap", "cap_inside_word"]
    # cover() on masks whose counters are known by hand: a flat trace, bins at 100 counts are hot
    def flat(n, hot, top=()):
        s = np.full(n, 50 << 8, np.int64)
        s[list(hot)] = 100 << 8
        s[list(top)] = 120 << 8
        return s
    c = B.cover(flat(512, [10, 12, 20, 126, 127, 128, 200], top=[127, 128]), 20, 1, 2)  # runs [10, 13) [20, 21) [126, 129) [200, 201)
    assert (c["runs"], c["multi_run_words"], c["single_run_words"], c["tied_peaks"], c["cold_eq_gap"], c["cold_eq_gap1"]) == (4, 1, 1, 2, 1, 0), c
    assert c["stretch_border_runs"] == 1 and not c["zero_runs"] and not c["over_cap"] and c["cold_words_inside"] == 0
    c = B.cover(flat(512, [63, 128]), 20, 64, 1)
    assert (c["runs"], c["cold_words_inside"], c["cold_eq_gap"], c["stretch_border_runs"]) == (1, 1, 1, 1), c
    assert B.cover(flat(512, [63, 128]), 20, 63, 1)["cold_words_inside"] == 0 and B.cover(flat(512, []), 20, 0, 1)["zero_runs"]
    n = 1 << 16
    c = B.cover(flat(n, np.flatnonzero(np.arange(n) % 4 == 1)), 20, 0, 1)  # run CAP is the first of word 512
    assert c["runs"] == n // 4 and c["over_cap"] and not c["cap_inside_word"]
    c = B.cover(flat(n, 8 + np.flatnonzero(np.arange(n - 8) % 4 == 1)), 20, 0, 1)  # ... the third
    assert c["runs"] == n // 4 - 2 and c["over_cap"] and c["cap_inside_word"]
    assert B.broken_rules(4096, {}) != [] and "zero_runs" in B.broken_rules(4096, {(1, 0): c})

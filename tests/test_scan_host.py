"""The band scan's host side (phantomsdr_amd/csrc/scanplan.h) without a GPU: tests/scan_plan_table.cpp is compiled with the host
C++ compiler - the header is plain C++17, and its steps are the text the kernels of scan.hip run - and compared with
tests/scan_model.py, the rule in numpy integers written from the words of include/psdr.h.  Every comparison is exact: the rule is
integer arithmetic."""
import os
import re

import numpy as np
import pytest

import scan_model as M
from conftest import ROOT

COLD, HOT, THR = 50 << 8, 100 << 8, 20  # a flat trace: the floor is COLD, a bin at HOT is 50 counts above it


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("scan_host")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


def flat(n, hot=()):
    s = np.full(n, COLD, np.int64)
    s[list(hot)] = HOT
    return s


def same(exe, tmp, s, thr, gap, min_width=1, cap=M.CAP):
    """the table program against the model on one trace; returns the model's runs"""
    F, runs = M.runs(s, thr, gap)
    t = M.table_eval(exe, tmp, s, thr, gap, min_width, cap)
    want, passed, total = M.listed(runs, min_width, cap)
    assert np.array_equal(t["Q"], M.quartiles(s)) and np.array_equal(t["F"], F)
    assert t["total"] == total and np.array_equal(t["list"], runs[:M.CAP])
    assert t["passed"] == passed and np.array_equal(t["out"], want)
    return runs


# ---- trace ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", range(9))
def test_trace_recurrence(exe, tmp, a):
    rng = np.random.default_rng(100 + a)
    n, F = 512, 40
    q = rng.integers(-128, 128, (F, n)).astype(np.int8)
    q[:, 0], q[:, 1] = -128, 127                       # u = 0 and u = 255 throughout
    q[::2, 2], q[1::2, 2] = -128, 127                  # ... and alternating: the largest steps both ways
    q[:, 3] = np.where(np.arange(F) < 20, 127, -128)   # a long fall: the floor shift must reach 0 from above
    want = M.trace(None, q, True, a)
    assert np.array_equal(M.table_trace(exe, tmp, None, q, True, a), want)
    if a == 0:
        assert np.array_equal(want, (q[-1].astype(np.int64) + 128) << 8)  # the last frame itself
    assert want[0] == 0 and want[1] == 255 * 256
    # any split into batches: the same bits
    for split in ((1,) * F, (5, 35), (17, 3, 20)):
        s, at = None, 0
        for k in split:
            s = M.table_trace(exe, tmp, s, q[at:at + k], at == 0, a)
            at += k
        assert np.array_equal(s, want), split
    # a fresh start forgets the trace
    assert np.array_equal(M.table_trace(exe, tmp, want, q[:3], True, a), M.trace(None, q[:3], True, a))


def test_trace_floor_shift_is_arithmetic(exe, tmp):
    # s = 256, u = 0, a = 8: d = -256, d >> 8 = -1; s = 255, d = -255, d >> 8 = -1 (floor, not truncation to 0) ... down to 0
    q = np.full((300, 256), -128, np.int8)
    q[0] = -127
    got = M.table_trace(exe, tmp, None, q, True, 8)
    assert np.all(got == 0) and np.all(M.trace(None, q, True, 8) == 0)
    assert np.all(M.table_trace(exe, tmp, None, q[:100], True, 8) == 256 - 99)


# ---- floor ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (256, 512, 4096))
def test_quartile_and_neighbour_minimum(exe, tmp, n):
    rng = np.random.default_rng(n)
    s = rng.integers(0, 255 * 256 + 1, n)
    s[:256] = rng.integers(0, 4, 256) * 7000  # many equal values: ties need no rule
    t = M.table_eval(exe, tmp, s, 255, 0)
    Q = M.quartiles(s)
    assert np.array_equal(t["Q"], Q) and np.array_equal(t["F"], M.floors(Q))
    if n == 256:
        assert len(t["F"]) == 1 and t["F"][0] == Q[0]  # G = 1: no neighbour
    else:
        assert t["F"][0] == min(Q[0], Q[1]) and t["F"][-1] == min(Q[-1], Q[-2])


def test_a_crowded_segment_does_not_lift_its_floor(exe, tmp):
    s = flat(1024)
    s[256:512] = HOT          # segment 1 is full of signal: its own quartile is HOT
    s[256:300] = HOT + 2560   # ... and carries something stronger still
    runs = same(exe, tmp, s, THR, 0)
    assert M.quartiles(s)[1] == HOT and np.all(M.floors(M.quartiles(s)) == COLD)
    assert len(runs) == 1 and (runs[0]["first"], runs[0]["end"]) == (256, 512)


# ---- runs of bins -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", (0, 1, 5, 63, 64))
def test_start_and_end_rule(exe, tmp, gap):
    n = 1024
    # at bin 0 and at n - 1; across the segment border 255 | 256; two tones gap cold bins apart (one run) and gap + 1 apart (two)
    a0, b0 = 400, 400 + gap + 1
    a1, b1 = 600, 600 + gap + 2
    s = flat(n, [0, n - 1, 254, 255, 256, 257, a0, b0, a1, b1])
    runs = same(exe, tmp, s, THR, gap)
    got = [(int(r["first"]), int(r["end"])) for r in runs]
    assert got == [(0, 1), (254, 258), (a0, b0 + 1), (a1, a1 + 1), (b1, b1 + 1), (n - 1, n)], got
    # words w - 2 and w + 2 matter at gap 64 only: a pair exactly 65 bins apart from a word's first bit
    s = flat(n, [127, 192, 320, 385])
    runs = same(exe, tmp, s, THR, gap)
    assert len(runs) == (2 if gap == 64 else 4)


def test_runs_on_random_masks(exe, tmp):
    rng = np.random.default_rng(7)
    for gap in (0, 2, 31, 64):
        for density in (0.002, 0.02, 0.2):
            s = flat(4096)
            s[rng.random(4096) < density] = HOT
            s += rng.integers(0, 200, 4096)
            same(exe, tmp, s, THR, gap)


def test_peak_ties_take_the_lowest_bin(exe, tmp):
    s = flat(512, range(100, 110))
    s[[103, 107]] = HOT + 300
    runs = same(exe, tmp, s, THR, 0)
    assert len(runs) == 1 and runs[0]["peak_bin"] == 103 and runs[0]["peak"] == HOT + 300 and runs[0]["floor"] == COLD
    s[100:110] = HOT  # all equal: the run's first bin
    assert same(exe, tmp, s, THR, 0)[0]["peak_bin"] == 100


def test_cap_total_and_one_run_over_the_band(exe, tmp):
    n = 1 << 16
    s = flat(n)
    s[np.arange(n) % 4 != 3] = HOT  # three bins up, one down: the quartile is COLD all the same
    assert M.quartiles(s).max() == COLD
    runs = same(exe, tmp, s, THR, 0)
    assert len(runs) == n // 4
    t = M.table_eval(exe, tmp, s, THR, 0)
    assert t["total"] == n // 4 and len(t["list"]) == M.CAP and t["list"][-1]["first"] == 4 * (M.CAP - 1)
    runs = same(exe, tmp, s, THR, 1)
    assert len(runs) == 1 and (runs[0]["first"], runs[0]["end"], runs[0]["peak_bin"]) == (0, n - 1, 0)


def test_min_width_filter_and_cap(exe, tmp):
    s = flat(2048, [10, 20, 21, 30, 31, 32, 40, 41, 42, 43, 50, 60, 61, 62])
    for mw, cap in ((0, 8192), (1, 8192), (2, 8192), (3, 1), (3, 0), (4, 5), (5, 5)):
        same(exe, tmp, s, THR, 0, mw, cap)
    t = M.table_eval(exe, tmp, s, THR, 0, 3, 2)
    assert t["passed"] == 3 and [int(f) for f in t["out"]["first"]] == [30, 40] and t["total"] == 6


# ---- the call ---------------------------------------------------------------------------------------------------------------
def test_rejections_in_order_with_their_texts(exe):
    R, levels = 4096, 6
    cases = [  # (level, shift, threshold, gap) -> verdict, a word of its text
        ((0, 3, 12, 2), 0, ""), ((4, 0, 1, 0), 0, ""), ((4, 8, 255, 64), 0, ""),
        ((-1, 9, 0, 65), 1, "level"), ((6, 9, 0, 65), 1, "level"),
        ((5, 9, 0, 65), 2, "128 bins"),
        ((4, 9, 0, 65), 3, "avg_shift"), ((4, -1, 0, 65), 3, "avg_shift"),
        ((4, 8, 0, 65), 4, "threshold"), ((4, 8, 256, 65), 4, "threshold"),
        ((4, 8, 255, 65), 5, "gap"), ((4, 8, 255, -1), 5, "gap"),
    ]
    out = M.run(exe, "".join(f"check {R} {levels} {c[0]} {c[1]} {c[2]} {c[3]}\n" for c, _, _ in cases))
    texts = set()
    for ln, (c, verdict, word) in zip(out, cases):
        f = M.fields(ln)
        assert int(f["verdict"]) == verdict, (c, ln)
        assert (word in f["text"]) if verdict else f["text"] == "", (c, ln)
        if verdict:
            texts.add(re.sub(r"-?\d+", "#", f["text"]))
    assert len(texts) == 5  # a text of its own each


def test_run_rule_as_a_state_machine(exe):
    script = "set\nstep 100 8\nstep 108 8\nstep 116 1\nstep 117 5\nstep 117 5\nstep 130 2\nstep 0 4\nstep 4 4\nset\nstep 8 4\nstep 12 4\n"
    out = [M.fields(ln) for ln in M.run(exe, script)]
    assert out[0] == dict(run="0", evaluated="0") and out[9] == dict(run="0", evaluated="0")
    fresh = [int(o["fresh"]) for o in out if "fresh" in o]
    #        first  cont  cont  cont  repeat  jump  back  cont | set: first cont
    assert fresh == [1, 0, 0, 0, 1, 1, 1, 0, 1, 0]
    assert [int(o["last"]) for o in out if "last" in o] == [107, 115, 116, 121, 121, 131, 3, 7, 11, 15]
    assert all(o["evaluated"] == "1" for o in out if "fresh" in o)


def test_launch_plan(exe):
    # IQ 2^20: tile-major records of 16 channels, levels 0..4 tiled; level 5 is level-major
    out = [M.fields(ln) for ln in M.run(exe, "".join(f"launch {1 << 20} 11 4 16 {lv}\n" for lv in range(7)))]
    for lv, o in enumerate(out):
        n = (1 << 20) >> lv
        assert int(o["n"]) == n and int(o["G"]) == n // 256 and int(o["words"]) == n // 64
        if lv <= 4:
            assert (int(o["tiled"]), int(o["per"]), int(o["loff"])) == (1, 16 >> lv, (0, 16, 24, 28, 30)[lv])
            assert int(o["trace_blocks"]) == (1 << 16) // 256  # a lane per record
        else:
            assert (int(o["tiled"]), int(o["per"])) == (0, 16) and int(o["qoff"]) == sum((1 << 20) >> t for t in range(lv))
            assert int(o["trace_blocks"]) * 256 * 16 >= n
    # no tiled records at all
    o = M.fields(M.run(exe, "launch 4096 3 -1 16 2\n")[0])
    assert (int(o["tiled"]), int(o["qoff"]), int(o["n"]), int(o["G"])) == (0, 4096 + 2048, 1024, 4)


def test_abi_is_additive():
    import ctypes

    import phantomsdr_amd as p
    from phantomsdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "psdr.h")).read()
    assert "#define PSDR_ABI_VERSION 3" in hdr and "#define PSDR_SCAN_MAX_SIGNALS 8192" in hdr
    names = [s[0] for s in _lib.SYMBOLS]
    for fn in ("psdr_scan_set", "psdr_scan_batch", "psdr_read_signals", "psdr_read_scan_floor", "psdr_read_scan_trace"):
        assert re.search(r"\bint %s\(" % fn, hdr) and fn in names
    assert ctypes.sizeof(_lib.psdr_scan_config) == 16 and p.SIGNAL_DTYPE.itemsize == 20 == M.SIGNAL.itemsize
    assert p.SCAN_MAX_SIGNALS == M.CAP

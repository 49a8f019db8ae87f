"""The noise floor's host side (phantomsdr_amd/csrc/noiseplan.h) without a GPU: tests/noise_plan_table.cpp is compiled with the
host C++ compiler - the header is plain C++17, and its steps are the text k_noise_floor runs - and driven by the scripts below.
The model the numbers are held against is the few lines of numpy in this file, written from the words of include/psdr.h: the
selection is numpy.sort on the sums' bit patterns."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_demod_plan import client, kind

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
RING = 8
N_AUDIO = 360  # audio_fft_size of the table program's contexts: the widest window


def build(tmp, name, extra=()):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(ROOT, "phantomsdr_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "noise_plan_table.cpp"), "-o", exe])
    return exe


def run(exe, text, timeout=120):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def fields(ln):
    return dict(kv.split("=", 1) for kv in ln.split()[1:])


def bits(v):
    return np.asarray(v, F32).view(np.uint32)


def from_bits(s):
    return np.array([int(x) for x in s.split(",")], np.uint32).view(F32) if s else np.zeros(0, F32)


def bit_list(v):
    return " ".join(str(int(b)) for b in np.atleast_1d(bits(v)))


# ---- the model ---------------------------------------------------------------------------------------------------------------
def rank(length):
    return (length - 1) // 4


def select(sums, k):
    """the k-th smallest in the order of the bit patterns as unsigned integers"""
    return np.sort(bits(sums))[k:k + 1].view(F32)[0]


def estimate(ring):
    m = INF
    for x in ring:
        m = x if x < m else m
    return m if m < INF else F32(0)


class Model:
    """one client's state: sums, ring, frame counter; frame(p): the powers of the window's bins in one frame -> W"""

    def __init__(self, length, period):
        self.len, self.period = length, period
        self.acc, self.ring, self.cnt, self.evals = np.zeros(max(length, 0), F32), [], 0, 0

    def frame(self, p):
        if self.len <= 0:
            return F32(0)
        with np.errstate(all="ignore"):
            self.acc = (self.acc + np.asarray(p, F32)).astype(F32)
            self.cnt += 1
            if self.cnt >= self.period:
                e = F32(select(self.acc, rank(self.len))) / F32(self.period)
                self.ring = (self.ring + [e])[-RING:]
                self.acc[:] = 0
                self.cnt = 0
                self.evals += 1
            return F32(estimate(self.ring) * F32(self.len))


def frames_line(x, period, lens):
    """x: complex64 [NF][LEN] -> the `frames` operation"""
    x = np.ascontiguousarray(x, np.complex64)
    nf, length = x.shape
    assert sum(lens) == nf
    return "frames %d %d %d %d %s %s" % (length, period, nf, len(lens), " ".join(map(str, lens)), " ".join(map(str, x.view(np.uint32).ravel().tolist())))


def all_splits(nf):
    for mask in range(1 << (nf - 1)):
        lens, at = [], 0
        for f in range(nf):
            if f + 1 == nf or (mask >> f) & 1:
                lens.append(f + 1 - at)
                at = f + 1
        yield lens


# ---- selection ---------------------------------------------------------------------------------------------------------------
def select_cases():
    rng = np.random.default_rng(20261020)
    cases = []
    for length in (1, 4, 5, 64, 65, N_AUDIO):
        base = (rng.standard_normal(length) ** 2 * 10.0 ** rng.uniform(-6, 6)).astype(F32)
        cases.append(("random", base))
        cases.append(("all equal", np.full(length, F32(3.25))))
        cases.append(("all zero", np.zeros(length, F32)))
        v = base.copy()
        v[rng.integers(0, length, max(1, length // 8))] = INF
        v[rng.integers(0, length, max(1, length // 8))] = NAN
        cases.append(("inf and nan", v))
        cases.append(("all inf", np.full(length, INF)))
        cases.append(("all nan", np.full(length, NAN)))
        one = np.uint32(bits(F32(1.0)))
        cases.append(("last bit", (one + rng.integers(0, 2, length).astype(np.uint32)).view(F32)))  # 1.0 and its neighbour above
        cases.append(("last bits", (one + rng.permutation(length).astype(np.uint32)).view(F32)))    # all different, one ulp apart
        cases.append(("subnormal", (rng.integers(0, 1 << 23, length).astype(np.uint32)).view(F32)))
    return cases


SELECT_CASES = select_cases()


def select_input():
    lines = []
    for _, v in SELECT_CASES:
        ks = sorted({0, rank(len(v)), len(v) // 2, len(v) - 1})
        lines += ["select %d %d %s" % (len(v), k, bit_list(v)) for k in ks]
    return lines


# ---- the plan scripts ----------------------------------------------------------------------------------------------------------
RESETS = ["case resets", *client(0, "USB"), *client(1, "AM"), *client(2, "FM"), *client(3, "IQ"),
          "noise 0 1", "noise 1 1", "noise 2 1", "pause 2", "batch",  # 0: 0 and 1 listed and fresh; 2 paused: its start is still to come; 3 has none
          "batch",  # 1: nobody fresh
          kind(0, "SAM"), "window 1 10 17.5 20", "notch 0 0 12 14", "batch",  # 2: a mode change, audio_mid alone, a notch: no reset
          "window 1 11 17.5 20", "batch",  # 3: [l, r) moved: slot 1 from zero
          "window 1 11 17.5 21", "batch",  # 4: ... r alone
          "resume 2", "batch",  # 5: switched on while paused: from zero now
          "pause 0", "batch", "window 0 12 15.25 20", "window 0 10 15.25 20", "batch", "resume 0", "batch",  # 6, 7, 8: a paused client stands still
          "noise 1 0", "batch", "noise 1 1", "batch",  # 9, 10: off, and on again: from zero
          "pause 1", "noise 1 0", "noise 1 1", "batch", "resume 1", "batch",  # 11, 12: off and on while paused
          "remove 2", "add 2", kind(2, "FM"), "window 2 10 15.25 20", "batch",  # 13: a fresh occupant comes without the feature
          "noise 2 1", "batch",  # 14
          "window 3 30 35.0 30", "noise 3 1", "batch",  # 15: an empty window is listed (its W rows are written: zeros)
          "noise 0 0", "noise 1 0", "noise 2 0", "noise 3 0", "batch"]  # 16: nobody
SPAN = ["case span", "size 8 360 5", *client(0, "USB"), *client(1, "AM"), *client(3, "USB"), *client(5, "IQ"), *client(7, "FM"),
        "noise 1 1", "noise 5 1", "squelch 1 1 6.0 3.0 1 0", "squelch 7 1 -20.0 -23.0 1 0", "ref 1 1", "batch",  # 0: slots 1 and 5 of 8: a span with a gap
        "pause 5", "batch",  # 1
        "ref 1 0", "resume 5", "squelch 5 1 6.0 6.0 1 0", "ref 5 1", "batch"]  # 2
REFUSALS = [("noise: unknown id", "noise 4 1", "BAD_ID"), ("noise: id below 0", "noise -1 1", "BAD_ID"), ("noise: id past the slots", "noise 8 0", "BAD_ID"),
            ("ref: unknown id", "ref 4 1", "BAD_ID"), ("ref: unknown id and value", "ref 4 7", "BAD_ID"), ("ref: unknown value", "ref 1 2", "BAD_VALUE"),
            ("ref: negative value", "ref 1 -1", "BAD_VALUE"), ("ref: noise without the noise floor", "ref 0 1", "NOISE_OFF"),
            ("noise: off under a noise-referenced squelch", "noise 1 0", "IN_USE")]
VALIDATION = ["case validation", *client(0, "USB"), *client(1, "AM"), "noise 1 1", "ref 1 1", "dump"]
for _, line, _ in REFUSALS:
    VALIDATION += [line, "dump"]
# the rate comes before the reference in use; an unknown id before the rate
VALIDATION += ["rate 0", "noise 4 1", "dump", "noise 0 1", "dump", "noise 1 0", "dump", "rate -5", "noise 0 1", "dump", "rate 12000",
               "ref 1 0", "dump", "noise 1 0", "dump", "noise 0 1", "dump", "noise 0 1", "dump"]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("noise_plan")


@pytest.fixture(scope="module")
def exe(tmp):
    return build(tmp, "noise_plan_table")


def test_selection_is_numpys_sort_on_the_bit_patterns(exe):
    out = [fields(ln) for ln in run(exe, "\n".join(select_input()) + "\n").splitlines()]
    at = 0
    seen = set()
    for what, v in SELECT_CASES:
        assert (bits(v) < 0x80000000).all()  # non-negative: the order of the bit patterns is numeric order, Inf above, NaN above Inf
        for k in sorted({0, rank(len(v)), len(v) // 2, len(v) - 1}):
            g = out[at]
            at += 1
            assert (int(g["len"]), int(g["k"]), int(g["rank"])) == (len(v), k, (len(v) - 1) // 4)
            assert int(g["bits"]) == int(bits(select(v, k))), (what, len(v), k)
        seen.add((what, len(v)))
    assert at == len(out) and {n for _, n in seen} == {1, 4, 5, 64, 65, N_AUDIO}
    # by hand: finite < +Inf < NaN, and the rank of the lower quartile
    assert [rank(n) for n in (1, 4, 5, 8, 9, 64, 65, 360)] == [0, 0, 1, 1, 2, 15, 16, 89]
    v = np.array([NAN, 2.0, INF, 1.0, 0.0], F32)
    assert [float(select(v, k)) for k in range(3)] == [0.0, 1.0, 2.0] and select(v, 3) == INF and np.isnan(select(v, 4))


RING_CASES = [("fewer than 8", [3.0, 2.0, 5.0]), ("exactly 8", [9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.5, 3.25]),
              ("wrap-around: the minimum leaves", [1.0] + [4.0] * 7 + [5.0, 6.0]), ("wrap-around twice", [float(20 - i) for i in range(19)]),
              ("inf and nan among them", [INF, 2.0, NAN, 3.0, INF]), ("non-finite first", [NAN, INF]),
              ("all non-finite gives 0", [2.0] + [INF, NAN] * 4 + [INF]), ("zero is a value", [1.0, 0.0, 2.0]),
              ("last bit", [1.0, float(np.nextafter(F32(1.0), F32(0))), 1.0])]


def test_ring_and_minimum(exe):
    text = "".join("ring %d %s\n" % (len(e), bit_list(np.array(e, F32))) for _, e in RING_CASES)
    out = [fields(ln) for ln in run(exe, text).splitlines()]
    at = 0
    for what, e in RING_CASES:
        e = [F32(x) for x in e]
        for j in range(len(e) + 1):
            g = out[at]
            at += 1
            want = estimate(e[max(0, j - RING):j])
            assert int(g["at"]) == j and int(g["bits"]) == int(bits(want)), (what, j)
            assert (int(g["fill"]), int(g["pos"])) == (min(j, RING), j % RING), (what, j)
    assert at == len(out)
    by = dict(RING_CASES)
    e = [F32(x) for x in by["all non-finite gives 0"]]
    assert estimate(e[:8]) == F32(2.0) and estimate(e[1:9]) == 0 and estimate(e[2:10]) == 0  # 0 only once all 8 entries are non-finite
    assert estimate([]) == 0 and estimate([F32(x) for x in by["wrap-around: the minimum leaves"]][1:9]) == F32(4.0)


def test_frames_against_the_model_under_every_split(exe):
    rng = np.random.default_rng(11)
    cases = []
    for length, period, nf in ((1, 1, 9), (5, 2, 9), (4, 3, 10), (64, 4, 9), (65, 2, 7), (N_AUDIO, 3, 7), (0, 2, 4)):
        # amplitudes k / 8 with im = 0 or another small dyadic: every product and sum is exact, whatever way it is rounded
        re = rng.integers(-40, 41, (nf, max(length, 0))) / 8.0
        im = rng.integers(-8, 9, (nf, max(length, 0))) / 4.0
        x = (re + 1j * im).astype(np.complex64)
        cases.append((x, length, period, list(all_splits(nf)) if nf <= 9 and length <= 65 else [[nf], [1] * nf, [3, nf - 3]]))
    # inexact sums (im = 0: fmaf(re, re, 0) is the rounded square), and non-finite bins away from the selected rank and at it
    x = rng.standard_normal((9, 64)).astype(np.complex64)
    cases.append((x, 64, 4, [[9], [1] * 9, [4, 5], [5, 4]]))
    y = x.copy()
    y[2, 60], y[3, 61] = np.inf, np.nan
    cases.append((y, 64, 4, [[9], [1] * 9, [2, 7]]))
    z = x.copy()
    z[0:4] = np.inf
    cases.append((z, 64, 4, [[9], [3, 6]]))
    text = "".join(frames_line(x, period, lens) + "\n" if length else "frames 0 %d %d %d %s\n" % (period, len(x), len(lens), " ".join(map(str, lens)))
                   for x, length, period, splits in cases for lens in splits)
    out = [fields(ln) for ln in run(exe, text).splitlines()]
    at = 0
    for x, length, period, splits in cases:
        m = Model(length, period)
        with np.errstate(all="ignore"):
            p = (x.real.astype(F32) * x.real.astype(F32) + (x.imag.astype(F32) * x.imag.astype(F32))).astype(F32)
        want = np.array([m.frame(p[f]) for f in range(len(x))], F32)
        for lens in splits:
            g = out[at]
            at += 1
            got = from_bits(g["bits"])
            assert got.tobytes() == want.tobytes(), (length, period, lens, got, want)
            assert (int(g["fill"]), int(g["pos"]), int(g["cnt"])) == (min(m.evals, RING), m.evals % RING, m.cnt)
        if length:
            assert want[:period - 1].tolist() == [0.0] * (period - 1)  # before the first evaluation
            assert from_bits(g["acc"]).tobytes() == m.acc.tobytes()
        else:
            assert not want.any()
    assert at == len(out)
    # the two non-finite cases by hand: a NaN and an Inf bin above the rank leave the estimate finite and positive; a window that
    # is Inf throughout gives an Inf entry, which is never the minimum - 0 until a finite evaluation arrives
    assert np.isfinite(want).all() and want[3] == 0 and want[7] > 0


def parse_batches(out, case):
    res, on = [], False
    for ln in out.splitlines():
        if ln.startswith("case "):
            on = fields(ln)["name"] == case
        elif on and ln.startswith("nf "):
            res.append([fields(ln)])
        elif on and ln.startswith("sq ") and res:
            res[-1].append(fields(ln))
    return res


def ints(s):
    return [int(v) for v in s.split(",")] if s else []


def listed(nf):
    return [tuple(int(v) for v in e.split(":")) for e in nf["list"].split(",")] if nf["list"] else []


def test_plan_who_is_listed_and_who_starts_from_zero(exe):
    b = [nf for nf, _ in parse_batches(run(exe, "\n".join(RESETS) + "\n"), "resets")]
    assert len(b) == 17
    w = (10, 20, 0)
    assert listed(b[0]) == [(0,) + w, (1,) + w] and ints(b[0]["zero"]) == [0, 1] and (b[0]["lo"], b[0]["nspan"]) == ("0", "2")
    assert listed(b[1]) == [(0,) + w, (1,) + w] and ints(b[1]["zero"]) == []
    assert listed(b[2]) == [(0,) + w, (1,) + w] and ints(b[2]["zero"]) == []  # mode, audio_mid alone, a notch
    assert listed(b[3])[1] == (1, 11, 20, 0) and ints(b[3]["zero"]) == [1]
    assert listed(b[4])[1] == (1, 11, 21, 0) and ints(b[4]["zero"]) == [1]
    assert [e[0] for e in listed(b[5])] == [0, 1, 2] and ints(b[5]["zero"]) == [2]  # switched on while paused
    assert [e[0] for e in listed(b[6])] == [1, 2] and [e[0] for e in listed(b[7])] == [1, 2]
    assert [e[0] for e in listed(b[8])] == [0, 1, 2] and ints(b[6]["zero"]) == ints(b[7]["zero"]) == ints(b[8]["zero"]) == []  # stood still
    assert [e[0] for e in listed(b[9])] == [0, 2] and ints(b[9]["zero"]) == []
    assert [e[0] for e in listed(b[10])] == [0, 1, 2] and ints(b[10]["zero"]) == [1]  # off and on again
    assert [e[0] for e in listed(b[11])] == [0, 2] and ints(b[11]["zero"]) == []
    assert ints(b[12]["zero"]) == [1]  # off and on while paused
    assert [e[0] for e in listed(b[13])] == [0, 1] and ints(b[13]["zero"]) == []  # a fresh occupant comes without
    assert [e[0] for e in listed(b[14])] == [0, 1, 2] and ints(b[14]["zero"]) == [2]
    assert listed(b[15])[-1] == (3, 30, 30, 0) and ints(b[15]["zero"]) == [3] and (b[15]["lo"], b[15]["nspan"]) == ("0", "4")
    assert b[16]["any"] == "0" and listed(b[16]) == [] and (b[16]["lo"], b[16]["nspan"], b[16]["fetch_n"]) == ("0", "0", "0")


def test_span_and_the_squelch_tables_reference_flag(exe):
    b = parse_batches(run(exe, "\n".join(SPAN) + "\n"), "span")
    assert len(b) == 3
    nf, sq = b[0]
    assert [e[0] for e in listed(nf)] == [1, 5] and (nf["lo"], nf["nspan"], nf["fetch_lo"], nf["fetch_n"]) == ("1", "5", "1", "5")  # the gap travels
    assert sq["list"] == "1:1,7:0" and sq["any_ref"] == "1"  # SquelchEntry::pad carries the reference
    nf, sq = b[1]
    assert [e[0] for e in listed(nf)] == [1] and (nf["lo"], nf["nspan"], nf["fetch_lo"], nf["fetch_n"]) == ("1", "1", "1", "1")
    nf, sq = b[2]
    assert (nf["lo"], nf["nspan"]) == ("1", "5") and sq["list"] == "1:0,5:1,7:0" and sq["any_ref"] == "1"


def test_validation_order_and_refusals_change_nothing(exe):
    out = run(exe, "\n".join(VALIDATION) + "\n").splitlines()
    sets = [(i, fields(ln)) for i, ln in enumerate(out) if ln.startswith("set ")]
    dump_at = [i for i, ln in enumerate(out) if ln.startswith("nfs slot=0 ")]
    dumps = [out[i:i + 8] for i in dump_at]
    assert [f["verdict"] for _, f in sets[:2]] == ["OK", "OK"]
    base = dumps[0]
    assert (fields(base[1])["on"], fields(base[1])["ref"], fields(base[1])["fresh"]) == ("1", "1", "1") and fields(base[0])["on"] == "0"
    for k, (what, _, verdict) in enumerate(REFUSALS):
        assert sets[2 + k][1]["verdict"] == verdict, what
        assert dumps[1 + k] == base, what
    a, d = 2 + len(REFUSALS), 1 + len(REFUSALS)
    tail = [f["verdict"] for _, f in sets[a:]]
    # rate 0: the id first, then the rate, for on = 1 and on = 0 - the rate before the reference in use; rate -5 the same
    assert tail[:4] == ["BAD_ID", "NO_RATE", "NO_RATE", "NO_RATE"] and dumps[d:d + 4] == [base] * 4
    # the reference back to absolute, then the noise floor may go; switching on twice keeps ONE fresh start
    assert tail[4:] == ["OK", "OK", "OK", "OK"]
    assert (fields(dumps[d + 4][1])["ref"], fields(dumps[d + 4][1])["on"]) == ("0", "1") and fields(dumps[d + 5][1])["on"] == "0"
    assert (fields(dumps[d + 6][0])["on"], fields(dumps[d + 6][0])["fresh"]) == ("1", "1") and dumps[d + 7] == dumps[d + 6]
    assert sets[0][1]["period"] == "33"  # 12000 / 360, the auto-notch detector's period


def test_relative_squelch_by_hand(exe):
    t = bits(F32(4.0))
    p = np.array([1.0, 5.0, 9.0, np.nan, np.inf, 0.0, 3.0, 3.0, 3.0], F32)
    w = np.array([0.0, 2.0, 2.0, 0.0, np.inf, 0.0, np.nan, np.inf, 1.0], F32)
    out = fields(run(exe, "relwalk %d %d 1 0 %d %s %s\n" % (t, t, len(p), bit_list(p), bit_list(w))).splitlines()[0])
    # W = 0: any power that is not NaN is at or above the threshold (0 >= 0 too); a NaN or Inf W compares false for a finite power
    assert out["flags"] == "101011000"
    with np.errstate(all="ignore"):
        assert [int(a >= F32(4.0) * b) for a, b in zip(p, w)] == [int(c) for c in out["flags"]]


def test_estimate_ignores_a_strong_signal():
    """Complex Gaussian noise of unit power per bin in a 64-bin window, period 4, 64 frames (16 evaluations); then a bin-centred
    tone 40 dB above the window's noise power (64), with -20 dB of it in each neighbour: three occupied bins shift the rank of the
    selected value by at most three places.  Observed with this seed: the estimate moves by a factor of 1.054 (0.576 -> 0.607 of
    the mean bin power), pwr by 40.1 dB.  The bound of 2 is loose on purpose."""
    rng = np.random.default_rng(3)
    nf, length, period = 64, 64, 4
    x = ((rng.standard_normal((nf, length)) + 1j * rng.standard_normal((nf, length))) / np.sqrt(2)).astype(np.complex64)
    y = x.copy()
    amp = np.sqrt(1e4 * length)
    y[:, 20] += amp
    y[:, 19] += 0.1 * amp
    y[:, 21] += 0.1 * amp
    res = []
    for s in (x, y):
        m = Model(length, period)
        p = (np.abs(s.astype(np.complex128)) ** 2).astype(F32)
        res.append((np.array([m.frame(p[f]) for f in range(nf)], F32)[-1] / length, float(p.sum(axis=1).mean())))
    (n0, pw0), (n1, pw1) = res
    ratio, step_db = float(n1 / n0), 10 * np.log10(pw1 / pw0)
    print(f"estimate per bin {n0:.3f} -> {n1:.3f} (ratio {ratio:.3f}), pwr +{step_db:.1f} dB")
    assert 0 < n0 < 1.0  # biased below the mean bin power (1.0): thresholds are relative to this number
    assert 0.5 < ratio < 2.0
    assert step_db > 30.0


def test_sanitizers(tmp, exe):
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    probe = tmp / "sanitizer_probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17", *flags, str(probe), "-o", str(tmp / "sanitizer_probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime to link against")
    san = build(tmp, "noise_plan_table_san", flags)  # (a program of its own: nothing of it is loaded into Python)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((7, N_AUDIO)).astype(np.complex64)
    text = "\n".join(select_input() + RESETS + SPAN + VALIDATION + [frames_line(x, 2, [3, 4]), frames_line(x[:, :1], 1, [7]), "frames 0 2 3 1 3"]) + "\n"
    text += "".join("ring %d %s\n" % (len(e), bit_list(np.array(e, F32))) for _, e in RING_CASES)
    r = subprocess.run([san], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == run(exe, text)


def test_abi_symbols_resolve():
    names = ("psdr_client_set_noise_floor", "psdr_client_set_squelch_reference", "psdr_read_noise", "psdr_fetched_noise")
    lib = ctypes.CDLL(os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so"))
    for name in names:
        assert hasattr(lib, name), name
    from phantomsdr_amd import _lib
    assert set(names) <= {s[0] for s in _lib.SYMBOLS}
    with open(os.path.join(ROOT, "include", "psdr.h")) as f:
        hdr = f.read()
    assert "PSDR_SQ_ABSOLUTE = 0, PSDR_SQ_NOISE = 1" in hdr and "#define PSDR_ABI_VERSION 3" in hdr  # additions only
    with open(os.path.join(ROOT, "phantomsdr_amd", "csrc", "squelchplan.h")) as f:
        assert "sizeof(SquelchEntry) == 24" in f.read()

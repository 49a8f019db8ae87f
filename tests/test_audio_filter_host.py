"""The audio filter's host side (phantomsdr_amd/csrc/audiofilterplan.h) without a GPU: tests/audio_filter_table.cpp is compiled
with the host C++ compiler - the header is plain C++17, and its step, zero-state pass, combine and true pass are the text
k_audio_filter runs - and driven by the scripts below.  The model is tests/audio_filter_model.py, written from the words of
include/psdr.h.

The blocked evaluation against float64 (test_blocked_against_float64), measured here with g++ on x86-64, RMS error relative to the
output's RMS, worst case over the stream lengths and splits of each (filter, input): the figures are in DESIGN 3.14."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import audio_filter_model as M
from conftest import ROOT
from helpers import CLIENT_KINDS
from test_demod_plan import client, kind

RATE = 12000.0
HALF_DB = 10 * math.log10(0.5)  # "-3.01 dB"
SPLITS = {"8": (8,), "1+7": (1, 7), "3+5": (3, 5), "1x8": (1,) * 8}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("audio_filter")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


def run(exe, text, timeout=120):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def fields(ln):
    return dict(kv.split("=", 1) for kv in ln.split()[1:])


def design(exe, kind_, rate, f0, q):
    g = fields(run(exe, "design %d %r %r %r\n" % (kind_, rate, f0, q)))
    return g["verdict"], tuple(float(g[k]) for k in ("b0", "b1", "b2", "a1", "a2"))


def ok(exe, kind_, f0, q=math.sqrt(0.5), rate=RATE):
    v, sec = design(exe, kind_, rate, f0, q)
    assert v == "OK", (kind_, f0, q, v)
    return sec


def fmt(sec):
    return " ".join(repr(float(v)) for v in sec)


# ---- validation ---------------------------------------------------------------------------------------------------------------
GOOD = (0.2, 0.4, 0.2, -0.5, 0.3)
UNSTABLE = (1.0, 0.0, 0.0, -1.96, 0.95)  # |a1| >= 1 + a2
POLE = (1.0, 0.0, 0.0, -1.9, 0.9995)     # stable; sqrt(a2) above AF_POLE_MAX
NONFINITE = (1.0, float("nan"), 0.0, -0.5, 0.3)
REFUSALS = [
    ("unknown id", "filter 4 1 " + fmt(GOOD), "BAD_ID"), ("id below 0", "filter -1 1 " + fmt(GOOD), "BAD_ID"), ("id past the slots", "filter 8 1 " + fmt(GOOD), "BAD_ID"),
    ("unknown id, off", "filter 4 0", "BAD_ID"),
    ("3 sections", "filter 0 3 " + fmt(GOOD) + " " + fmt(GOOD) + " " + fmt(GOOD), "BAD_COUNT"), ("-1 sections", "filter 0 -1", "BAD_COUNT"),
    ("null", "filter 0 1 null", "NULL"), ("null, two", "filter 0 2 null", "NULL"),
    ("NaN b1", "filter 0 1 " + fmt(NONFINITE), "NONFINITE"), ("Inf a2", "filter 0 1 1.0 0.0 0.0 -0.5 inf", "NONFINITE"),
    ("-Inf b0 in the second", "filter 0 2 " + fmt(GOOD) + " -inf 0.0 0.0 -0.5 0.3", "NONFINITE"), ("b0 beyond f32", "filter 0 1 1e39 0.0 0.0 -0.5 0.3", "NONFINITE"),
    ("a2 = 1", "filter 0 1 1.0 0.0 0.0 0.0 1.0", "UNSTABLE"), ("a2 = -1", "filter 0 1 1.0 0.0 0.0 0.0 -1.0", "UNSTABLE"),
    ("|a1| = 1 + a2", "filter 0 1 1.0 0.0 0.0 1.5 0.5", "UNSTABLE"), ("|a1| above 1 + a2", "filter 0 1 " + fmt(UNSTABLE), "UNSTABLE"),
    ("unstable second", "filter 0 2 " + fmt(GOOD) + " " + fmt(UNSTABLE), "UNSTABLE"),
    ("complex poles outside", "filter 0 1 " + fmt(POLE), "POLE"), ("real pole outside", "filter 0 1 1.0 0.0 0.0 -0.9996 0.0", "POLE"),
    ("real poles outside", "filter 0 1 1.0 0.0 0.0 -1.4998 0.4999", "POLE"), ("second's pole outside", "filter 0 2 " + fmt(GOOD) + " " + fmt(POLE), "POLE"),
    # the precedence: id, count, null, non-finite, stability, pole radius - each looked for in every section before the next
    ("id before count", "filter 4 3 null", "BAD_ID"), ("count before null", "filter 0 3 null", "BAD_COUNT"),
    ("non-finite in the second before unstable in the first", "filter 0 2 " + fmt(UNSTABLE) + " " + fmt(NONFINITE), "NONFINITE"),
    ("unstable in the second before the first's pole", "filter 0 2 " + fmt(POLE) + " " + fmt(UNSTABLE), "UNSTABLE"),
    ("non-finite before the pole", "filter 0 2 " + fmt(POLE) + " " + fmt(NONFINITE), "NONFINITE"),
]
AT_THE_LIMIT = M.pole_section(M.POLE_MAX, 0.3)
ACCEPTED = ["filter 0 2 " + fmt(GOOD) + " " + fmt(AT_THE_LIMIT), "filter 0 1 1.0 0.0 0.0 -0.9995 0.0", "filter 0 0 null", "filter 0 0"]
VALIDATION = ["case validation", *client(0, "USB"), *client(1, "AM"), "filter 1 1 " + fmt(GOOD), "dump"]
for _, line, _ in REFUSALS:
    VALIDATION += [line, "dump"]
for line in ACCEPTED:
    VALIDATION += [line, "dump"]


def test_validation_refuses_in_order_and_changes_nothing(exe):
    out = run(exe, "\n".join(VALIDATION) + "\n").splitlines()
    sets = [i for i, ln in enumerate(out) if ln.startswith("set ")]
    dumps = [out[i + 1:i + 9] for i in sets]
    assert all(len(d) == 8 and all(ln.startswith("afs ") for ln in d) for d in dumps)
    assert fields(out[sets[0]])["verdict"] == "OK"
    base = dumps[0]
    f1 = fields(base[1])
    assert (f1["n"], f1["fresh"]) == ("1", "1") and fields(base[0])["n"] == "0"
    assert [int(v) for v in f1["sec0"].split(":")[:5]] == [int(np.float32(v).view(np.uint32)) for v in GOOD]
    assert {v for _, _, v in REFUSALS} == {"BAD_ID", "BAD_COUNT", "NULL", "NONFINITE", "UNSTABLE", "POLE"}  # every refusal code
    for k, (what, _, verdict) in enumerate(REFUSALS, 1):
        assert fields(out[sets[k]])["verdict"] == verdict, what
        assert dumps[k] == base, what  # nothing changed
    a = len(REFUSALS) + 1
    assert [fields(out[sets[a + k]])["verdict"] for k in range(len(ACCEPTED))] == ["OK"] * len(ACCEPTED)
    assert (fields(dumps[a][0])["n"], fields(dumps[a][0])["fresh"]) == ("2", "1")  # AF_POLE_MAX itself passes, complex ...
    assert fields(dumps[a + 1][0])["n"] == "1"  # ... and real
    assert fields(dumps[a + 2][0])["n"] == "0" and dumps[a + 2][1] == base[1]  # off ignores the pointer


# ---- design -------------------------------------------------------------------------------------------------------------------
def test_design_deemphasis(exe):
    for rate, f0 in ((12000.0, 212.0), (48000.0, 212.0), (12000.0, 3183.1)):
        sec = ok(exe, M.DEEMPHASIS, f0, rate=rate)
        assert sec[2] == 0.0 and sec[4] == 0.0
        assert abs(M.response_db(sec, f0, rate) - HALF_DB) < 1e-9
        assert abs(M.response_db(sec, 0.0, rate)) < 1e-9
        # the analogue prototype 1 / (1 + (F / F0)^2) on the warped axis F = tan(pi f / rate) - this IS the bilinear transform
        f = np.geomspace(f0 / 10, rate / 2 * 0.999, 60)
        want = -10 * np.log10(1 + (np.tan(np.pi * f / rate) / np.tan(np.pi * f0 / rate)) ** 2)
        assert np.abs(M.response_db(sec, f, rate) - want).max() < 1e-9
    # -20 dB per decade above f0, before the warp: at 48 kHz between 2 and 4 kHz (10 to 20 x f0, a twelfth of Nyquist and
    # below) the slope is -20 dB per decade within the two terms the formula gives - the prototype's own approach,
    # 10 log10((1 + 400) / (1 + 100) / 4), and the warp, 20 log10(tan(pi 4000 / 48000) / tan(pi 2000 / 48000) / 2)
    sec = ok(exe, M.DEEMPHASIS, 212.0, rate=48000.0)
    step = float(M.response_db(sec, 4240.0, 48000.0) - M.response_db(sec, 2120.0, 48000.0))
    K0 = math.tan(math.pi * 212.0 / 48000.0)
    t2, t4 = math.tan(math.pi * 2120.0 / 48000.0) / K0, math.tan(math.pi * 4240.0 / 48000.0) / K0
    assert abs(step - (-10 * math.log10((1 + t4 * t4) / (1 + t2 * t2)))) < 1e-9
    assert abs(step / math.log10(2.0) - (-20.0)) < 0.6  # dB per decade: 20 within 3 % with the warp still small


def test_design_second_order(exe):
    for rate in (12000.0, 48000.0):
        for f0 in (300.0, 700.0, 2700.0):
            hp, lp = ok(exe, M.HIGHPASS, f0, rate=rate), ok(exe, M.LOWPASS, f0, rate=rate)
            assert abs(M.response_db(hp, f0, rate) - HALF_DB) < 1e-9 and abs(M.response_db(lp, f0, rate) - HALF_DB) < 1e-9
            assert abs(M.response_db(lp, 0.0, rate)) < 1e-9 and abs(M.response_db(hp, rate / 2, rate)) < 1e-9
            for q in (0.5, 5.0, 20.0):
                pk = ok(exe, M.PEAK, f0, q, rate)
                assert abs(M.response_db(pk, f0, rate)) < 1e-9
                # the band edges the formula defines: the prototype's, W = sqrt(1 + 1 / 4q^2) -+ 1 / 2q, warped back
                K = math.tan(math.pi * f0 / rate)
                for sign in (-1, 1):
                    W = math.sqrt(1 + 1 / (4 * q * q)) + sign / (2 * q)
                    fe = math.atan(K * W) * rate / math.pi
                    assert abs(M.response_db(pk, fe, rate) - HALF_DB) < 1e-9, (rate, f0, q, sign)
    # bandwidth f0 / q where the warp is small
    K = math.tan(math.pi * 700.0 / 48000.0)
    lo, hi = (math.atan(K * (math.sqrt(1 + 1 / 1600) + s / 40)) * 48000.0 / math.pi for s in (-1, 1))
    assert abs((hi - lo) - 700.0 / 20) < 0.1


def test_design_refusals(exe):
    for args, want in (((7, RATE, 300.0, 1.0), "BAD_KIND"), ((-1, RATE, 300.0, 1.0), "BAD_KIND"), ((1, 0.0, 300.0, 1.0), "BAD_RATE"),
                       ((1, float("nan"), 300.0, 1.0), "BAD_RATE"), ((1, float("inf"), 300.0, 1.0), "BAD_RATE"), ((1, RATE, 0.0, 1.0), "BAD_F0"),
                       ((1, RATE, 6000.0, 1.0), "BAD_F0"), ((1, RATE, -5.0, 1.0), "BAD_F0"), ((1, RATE, float("nan"), 1.0), "BAD_F0"),
                       ((2, RATE, 300.0, 0.0), "BAD_Q"), ((3, RATE, 300.0, -1.0), "BAD_Q"), ((3, RATE, 300.0, float("nan")), "BAD_Q"),
                       ((3, RATE, 50.0, 100.0), "REFUSED"), ((0, RATE, 0.5, 1.0), "REFUSED")):  # pole radius above AF_POLE_MAX
        assert design(exe, *args)[0] == want, args
    assert design(exe, M.DEEMPHASIS, RATE, 212.0, -1.0)[0] == "OK"  # q ignored
    for rate in (12000.0, 48000.0):  # what AF_POLE_MAX is there to admit
        assert design(exe, M.PEAK, rate, 700.0, 20.0)[0] == "OK"


# ---- the table ----------------------------------------------------------------------------------------------------------------
def test_table_powers_are_the_matrix_powers(exe):
    secs = [ok(exe, M.DEEMPHASIS, 212.0), ok(exe, M.HIGHPASS, 300.0), ok(exe, M.LOWPASS, 2700.0), ok(exe, M.PEAK, 700.0, 20.0), AT_THE_LIMIT,
            ok(exe, M.PEAK, 700.0, 20.0, 48000.0), (1.0, 0.0, 0.0, -0.9995, 0.0)]
    out = run(exe, "".join("table %s\n" % fmt(s) for s in secs)).splitlines()
    for sec, ln in zip(secs, out):
        v = np.array([int(t) for t in fields(ln)["sec"].split(":")], np.uint32).view(np.float32)
        assert np.array_equal(v[:5], np.asarray(sec, np.float32))  # rounded once
        A = M.state_matrix(sec)
        for k in range(6):
            want = np.linalg.matrix_power(A, M.CHUNK << k).reshape(-1)
            got = v[5 + 4 * k:9 + 4 * k].astype(np.float64)
            assert np.all(np.abs(got - want) <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)), (sec, k, got, want)


# ---- the blocked evaluation against float64 -----------------------------------------------------------------------------------
HS, FS = (4, 62, 180), (1, 5, 8, 37)
NMAX = max(HS) * max(FS)


@functools.lru_cache(maxsize=None)
def inputs():
    rng = np.random.default_rng(20261019)
    t = np.arange(NMAX)
    return {"noise": rng.standard_normal(NMAX).astype(np.float32), "tone": np.cos(2 * np.pi * 1000.0 * t / RATE + 0.3).astype(np.float32)}


def filters(exe):
    hp, de = ok(exe, M.HIGHPASS, 300.0), ok(exe, M.DEEMPHASIS, 212.0)
    return {"deemphasis 212": [de], "highpass 300": [hp], "lowpass 2700": [ok(exe, M.LOWPASS, 2700.0)], "peak 700 q20": [ok(exe, M.PEAK, 700.0, 20.0)],
            "highpass 300 + deemphasis 212": [hp, de], "AF_POLE_MAX": [M.pole_section(M.POLE_MAX, 2 * np.pi * 700.0 / RATE, 1 - M.POLE_MAX)]}


def rel_rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2)) / np.sqrt(np.mean(np.asarray(b, np.float64) ** 2)))


def test_blocked_against_float64(exe, tmp):
    """the blocked form's error against float64 is at most 4 x the sequential f32 form's, on each input: every (filter, input,
    stream length h * F, split)"""
    x = inputs()
    names = list(x)
    X = np.stack([x[k] for k in names])
    worst = {}
    for fname, secs in filters(exe).items():
        T, S = M.truth(secs, X), M.sequential(secs, X)
        jobs, keys = [], []
        for i, iname in enumerate(names):
            for h in HS:
                for F in FS:
                    for sname, split in SPLITS.items():
                        jobs.append((secs, X[i, :h * F], np.zeros(F, np.int32), h, M.batches_of(split, F)))
                        keys.append((i, iname, h * F, sname))
        for (i, iname, n, sname), (rows, states) in zip(keys, M.run_blocked(exe, tmp, jobs)):
            eb, es = rel_rms(rows, T[i, :n]), rel_rms(S[i, :n], T[i, :n])
            w = worst.setdefault((fname, iname), [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], eb), max(w[1], es), max(w[2], eb / es)
            assert eb <= 4 * es, (fname, iname, n, sname, eb, es)
            assert np.isfinite(states).all()
    for (fname, iname), (eb, es, ratio) in worst.items():
        print(f"{fname:32s} {iname:6s} blocked {eb:.3e} sequential {es:.3e} worst ratio {ratio:.2f}")


def test_blocked_with_a_flagged_frame(exe, tmp):
    """a flagged frame enters as zeros, the state advances, and its row is left alone - NaN bits included"""
    x = inputs()
    secs = filters(exe)["highpass 300 + deemphasis 212"]
    for h in HS:
        F = 8
        flags = np.zeros(F, np.int32)
        flags[3] = 1
        for iname in x:
            rows = x[iname][:h * F].copy()
            rows[3 * h + 1] = np.nan
            rows[3 * h + 2:4 * h].view(np.uint32)[:] = 0x7FC01234
            clean = np.where(np.repeat(flags, h) != 0, 0, rows)[None]
            T, S = M.truth(secs, clean)[0], M.sequential(secs, clean)[0]
            jobs = [(secs, rows, flags, h, M.batches_of(split, F)) for split in SPLITS.values()]
            for got, states in M.run_blocked(exe, tmp, jobs, "flag"):
                keep = np.repeat(flags, h) == 0
                assert got[~keep].tobytes() == rows[~keep].tobytes()
                assert np.isfinite(got[keep]).all() and np.isfinite(states).all()  # NaN never enters the state
                assert rel_rms(got[keep], T[keep]) <= 4 * rel_rms(S[keep], T[keep]), (h, iname)


def test_blocked_through_subnormals_to_zero(exe, tmp):
    """a tone, then zeros: the state of a filter whose poles lie inside 0.5 decays through the subnormals to exactly zero"""
    h, F = 62, 37
    secs = [ok(exe, M.LOWPASS, 3000.0)]
    rows = np.zeros(h * F, np.float32)
    rows[:200] = inputs()["tone"][:200]
    T, S = M.truth(secs, rows[None])[0], M.sequential(secs, rows[None])[0]
    tiny = np.finfo(np.float32).tiny
    for split in SPLITS.values():
        (got, states), = M.run_blocked(exe, tmp, [(secs, rows, np.zeros(F, np.int32), h, M.batches_of(split, F))], "zero")
        sub = (got != 0) & (np.abs(got) < tiny)
        assert sub.any() and not got[-h:].any() and not states[-1].any(), "the subnormals are kept, and the state ends at zero"
        assert rel_rms(got, T) <= 4 * rel_rms(S, T)


# ---- the plan -----------------------------------------------------------------------------------------------------------------
NAMES = list(CLIENT_KINDS)
AUDIO_KINDS = [k for k in NAMES if CLIENT_KINDS[k][0] != "IQ"]
TWO = fmt(GOOD) + " " + fmt((0.5, 0.0, -0.5, -0.2, 0.1))


def entries(af):
    return [tuple(int(v) for v in e.split(":")) for e in af["list"].split(",")] if af["list"] else []


def zero(af):
    return [int(v) for v in af["zero"].split(",")] if af["zero"] else []


def test_plan_who_is_listed_and_whose_state_is_fresh(exe):
    P = len(NAMES)  # the paused client's slot
    lines = ["case plan", "size 16 360 5"]
    for i, k in enumerate(NAMES):
        lines += client(i, k) + ["filter %d 2 %s" % (i, TWO)]
    lines += client(P, "USB") + ["filter %d 1 %s" % (P, fmt(GOOD)), "pause %d" % P, "batch",  # 0
                                 "batch",  # 1: nobody fresh
                                 "filter 0 2 " + TWO, "resume %d" % P, "batch",  # 2: new coefficients: fresh; switched on while paused: fresh now
                                 kind(NAMES.index("IQ"), "USB"), kind(NAMES.index("AM"), "FM"), "window 1 30 35.5 40", "batch",  # 3: IQ -> USB: its first filtered batch
                                 kind(NAMES.index("IQ"), "IQ"), "batch", kind(NAMES.index("IQ"), "USB"), "batch",  # 4, 5: USB -> IQ -> USB: the state stood still
                                 "filter 2 0", "remove 3", "add 3", kind(3, "FM"), "window 3 10 15.25 20", "batch",  # 6: off; a fresh slot comes without
                                 ]
    for i in range(P + 1):
        lines.append("filter %d 0" % i)
    lines += ["batch"]  # 7: no filter client
    out = run(exe, "\n".join(lines) + "\n")
    b = [fields(ln) for ln in out.splitlines() if ln.startswith("af ")]
    audio = [NAMES.index(k) for k in AUDIO_KINDS]
    iq = NAMES.index("IQ")
    assert len(audio) == 9 and [e[0] for e in entries(b[0])] == audio and zero(b[0]) == audio  # every kind that writes audio rows; IQ, TIQ and the paused one are not listed
    assert all(e[1] == 2 for e in entries(b[0]))
    assert [e[0] for e in entries(b[1])] == audio and zero(b[1]) == []
    assert [e[0] for e in entries(b[2])] == audio + [P] and zero(b[2]) == [0, P] and entries(b[2])[-1][1] == 1
    assert [e[0] for e in entries(b[3])] == sorted(audio + [P, iq]) and zero(b[3]) == [iq]  # a retune and a mode change reset nothing
    assert iq not in [e[0] for e in entries(b[4])] and zero(b[4]) == []
    assert iq in [e[0] for e in entries(b[5])] and zero(b[5]) == []
    assert [e[0] for e in entries(b[6])] == [i for i in sorted(audio + [P, iq]) if i not in (2, 3)] and zero(b[6]) == []
    assert b[7]["any"] == "0" and entries(b[7]) == [] and zero(b[7]) == []  # nothing to upload, zero or launch
    # the second section's place holds zeros for a client with one
    assert entries(b[2])[-1][3] == 0


def test_plan_of_a_context_without_filter_clients(exe):
    lines = ["case none", *client(0, "USB"), *client(1, "AM"), "batch", "batch"]
    b = [fields(ln) for ln in run(exe, "\n".join(lines) + "\n").splitlines() if ln.startswith("af ")]
    assert len(b) == 2 and all(x["have"] == "0" and x["any"] == "0" and x["list"] == "" for x in b)


def test_the_demodulation_plan_does_not_know_the_filter(exe):
    def script(with_filter):
        out = ["case ring", "size 12 360 5", "post on"]
        for i, k in ((0, "USB"), (1, "IQ"), (2, "TUSB"), (3, "SAMU"), (7, "FM"), (8, "TIQ")):
            out += client(i, k) + (["filter %d 2 %s" % (i, TWO)] if with_filter else [])
        return out + ["batch", "pause 2", "batch", "post off", "resume 2", "batch"]
    plan = lambda text: [ln for ln in text.splitlines() if not ln.startswith(("af ", "set "))]  # noqa: E731
    assert plan(run(exe, "\n".join(script(True)) + "\n")) == plan(run(exe, "\n".join(script(False)) + "\n"))


def test_sanitizers(tmp, exe):
    """the table program under AddressSanitizer and UBSan on the ragged cases: every stream length that ends inside a chunk, a
    block of one sample, frames shorter than a chunk, the flagged frame"""
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    probe = tmp / "sanitizer_probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17", *flags, str(probe), "-o", str(tmp / "sanitizer_probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime to link against")
    san = M.build_table(tmp, ROOT, flags, "audio_filter_table_san")
    x = inputs()["noise"]
    secs = filters(exe)["highpass 300 + deemphasis 212"]
    jobs = []
    for h, F in ((4, 1), (4, 5), (62, 1), (62, 5), (62, 37), (180, 8), (180, 37), (1, 1), (1, 17), (1, 1025)):
        fl = np.zeros(F, np.int32)
        fl[F // 2] = F > 4
        for split in SPLITS.values():
            jobs.append((secs, x[:h * F], fl, h, M.batches_of(split, F)))
    a, b = M.run_blocked(san, tmp, jobs, "san"), M.run_blocked(exe, tmp, jobs, "ref")
    for (ra, sa), (rb, sb) in zip(a, b):
        assert ra.tobytes() == rb.tobytes() and sa.tobytes() == sb.tobytes()
    text = "\n".join(VALIDATION) + "\n"
    r = subprocess.run([san], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == run(exe, text)


def test_abi_symbols_and_constants():
    lib = ctypes.CDLL(os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so"))
    for name in ("psdr_client_set_audio_filter", "psdr_audio_filter_design"):
        assert hasattr(lib, name), name
    import re

    import phantomsdr_amd as p
    from phantomsdr_amd import _lib
    assert {"psdr_client_set_audio_filter", "psdr_audio_filter_design"} <= {s[0] for s in _lib.SYMBOLS}
    hdr = open(os.path.join(ROOT, "include", "psdr.h")).read()
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(PSDR_AF_[A-Z]+|PSDR_AUDIO_FILTER_SECTIONS)\s+(\d+)", hdr))
    assert defs == {"PSDR_AF_DEEMPHASIS": p.AF_DEEMPHASIS, "PSDR_AF_HIGHPASS": p.AF_HIGHPASS, "PSDR_AF_LOWPASS": p.AF_LOWPASS, "PSDR_AF_PEAK": p.AF_PEAK,
                    "PSDR_AUDIO_FILTER_SECTIONS": p.AUDIO_FILTER_SECTIONS}
    assert "#define PSDR_ABI_VERSION 3" in hdr and ctypes.sizeof(_lib.psdr_biquad) == 40
    # the design helper needs no context (and no device): the library's answer is the table program's formula
    sec = p.design_audio_filter("peak", 12000, 700, 20)
    K = math.tan(math.pi * 700 / 12000)
    N = 1 / (1 + K / 20 + K * K)
    want = (K / 20 * N, 0.0, -(K / 20 * N), 2 * (K * K - 1) * N, (1 - K / 20 + K * K) * N)
    assert all(abs(a - b) <= 4 * np.spacing(abs(b)) for a, b in zip(sec, want)), (sec, want)  # (another libm's tan may differ in the last place)
    with pytest.raises(p.PsdrError) as e:
        p.design_audio_filter("peak", 12000, 7000, 20)
    assert e.value.code == -1

"""The AGC profile's host side (phantomsdr_amd/csrc/agcplan.h, postplan.h pc_agc_coeff) without a GPU: tests/agc_profile_table.cpp
is compiled with the host C++ compiler and driven by the scripts below.  Its `run` - the sample-by-sample recurrence with
agc_want and one fmaf per gain step - is first pinned to the oracle's AGC bit for bit; after that it stands in where the oracle
has no counterpart (manual gain, cap).  The symbols of the feature are checked in the built library and in _lib.py."""
import ctypes
import math
import os

import numpy as np
import pytest

import agc_profile_model as M
from conftest import ROOT

INF_BITS = 0x7F800000


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("agc_profile")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


def bits(v):
    return int(np.float32(v).view(np.uint32))


def noise(seed=3, T=4 * M.L):
    """noise whose level rises by 20 dB in the run (three look-aheads in: the gain has a look-ahead's time to climb before the
    window reaches the rise): release and attack both act"""
    x = np.random.default_rng(seed).standard_normal(T).astype(np.float32) * np.float32(0.003)
    x[3 * T // 4:] *= np.float32(10)
    return x


# (attack_ms, release_ms, desired): ms values exactly representable in f32
ORACLE_PROFILES = [(5.0, 100.0, 0.2), (50.0, 300.0, 0.2), (50.0, 2000.0, 0.2), (50.0, 300.0, 0.05), (5.0, 100.0, 0.5)]


def test_model_equals_the_oracle_bit_for_bit(exe, tmp):
    silence = np.zeros(2 * M.L, np.float32)
    jobs, want = [], []
    for att, rel, desired in ORACLE_PROFILES:
        p = M.profile(desired=desired, attack_ms=att, release_ms=rel)
        for x in (noise(), silence):
            jobs.append((x, [(x.size, 0, p)]))
            want.append(M.oracle_agc(x, p))
    for (x, segs), (y, g), w in zip(jobs, M.model_runs(exe, tmp, jobs), want):
        assert np.array_equal(y.view(np.uint32), w.view(np.uint32)), segs
        assert np.all(y[: M.L - 1] == 0)
        if x.any():
            d = np.diff(g[M.L - 1:])
            assert np.count_nonzero(y) > M.L and (d > 0).sum() > 100 and (d < 0).sum() > 100, "the gain did not both rise and fall: attack or release never acted"
        else:  # digital silence: the gain climbs towards desired / 1e-10
            assert g[-1] > 1e3
    # a slot without a profile runs the context's numbers: the reference profile's bits
    x = noise(seed=4)
    a, b = M.model_runs(exe, tmp, [(x, [(x.size, 0, None)]), (x, [(x.size, 0, M.REFERENCE)])], tag="none")
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_coefficients_are_post_plans(exe):
    for rate in (8000, 12000, 48000, 192000):
        plan = M.fields(M.script(exe, f"plan {rate} 360\n"))
        assert plan["verdict"] == "0" and plan["att_faster"] == "1"
        for ms, key in ((50.0, "attack"), (300.0, "release")):
            got = int(M.fields(M.script(exe, f"coeff {ms!r} {rate}\n"))["bits"])
            # the expression itself, in numpy's f32 and Python's double exp
            arg = np.float32(-1.0) / (np.float32(ms) * np.float32(0.001) * np.float32(rate))
            assert got == int(plan[key]) == bits(np.float32(1 - math.exp(float(arg)))), (rate, ms)
        assert int(plan["desired"]) == bits(0.2)


GOOD = "0.2 50 300 0 0 0"
# (what, arguments behind `set`, verdict) - in the order the header states
REFUSALS = [
    ("unknown id", "2 12000 " + GOOD, "BAD_ID"), ("id below 0", "-1 12000 " + GOOD, "BAD_ID"), ("id past the slots", "4 12000 " + GOOD, "BAD_ID"),
    ("unknown id, null", "3 12000 null", "BAD_ID"),
    ("NaN desired", "0 12000 nan 50 300 0 0 0", "NONFINITE"), ("infinite attack", "0 12000 0.2 inf 300 0 0 0", "NONFINITE"),
    ("NaN release", "0 12000 0.2 50 nan 0 0 0", "NONFINITE"), ("infinite cap", "0 12000 0.2 50 300 inf 0 0", "NONFINITE"),
    ("NaN manual gain", "0 12000 0.2 50 300 0 1 nan", "NONFINITE"), ("manual gain beyond f32", "0 12000 0.2 50 300 0 1 1e39", "NONFINITE"),
    ("non-finite comes before the ranges", "0 12000 7 50 nan 0 0 0", "NONFINITE"),
    ("desired 0", "0 12000 0 50 300 0 0 0", "BAD_DESIRED"), ("desired above 1", "0 12000 1.0000001 50 300 0 0 0", "BAD_DESIRED"), ("desired below 0", "0 12000 -0.2 50 300 0 0 0", "BAD_DESIRED"),
    ("desired before time", "0 12000 2 0 300 0 0 0", "BAD_DESIRED"),
    ("attack 0", "0 12000 0.2 0 300 0 0 0", "BAD_TIME"), ("release above 10 s", "0 12000 0.2 50 10000.001 0 0 0", "BAD_TIME"), ("attack below 0", "0 12000 0.2 -5 300 0 0 0", "BAD_TIME"),
    ("time before cap", "0 12000 0.2 50 0 -1 0 0", "BAD_TIME"),
    ("cap below 0", "0 12000 0.2 50 300 -1 0 0", "BAD_CAP"), ("cap before manual", "0 12000 0.2 50 300 -1 2 0", "BAD_CAP"),
    ("manual 2", "0 12000 0.2 50 300 0 2 0", "BAD_MANUAL"), ("manual -1", "0 12000 0.2 50 300 0 -1 0", "BAD_MANUAL"),
    ("manual gain below 0", "0 12000 0.2 50 300 0 1 -0.5", "BAD_MANUAL_GAIN"),
    ("no audio rate", "0 0 " + GOOD, "NO_RATE"), ("negative audio rate", "0 -12000 " + GOOD, "NO_RATE"),
    ("attack slower than release", "0 12000 0.2 300 50 0 0 0", "ATTACK_SLOWER"), ("attack slower, manual", "0 12000 0.2 100 99 0 1 3", "ATTACK_SLOWER"),
]


def test_every_refusal_leaves_the_setting_alone(exe):
    setup = "set 0 12000 0.5 5 100 40 0 0\n"
    text = setup + "".join(f"set {args}\nset 0 12000 0.5 5 100 40 0 0\n" for _, args, _ in REFUSALS)
    out = M.script(exe, text).strip().split("\n")
    first = M.fields(out[0])
    assert first["verdict"] == "OK"
    e = first["entry"].split(":")
    assert int(e[0]) == bits(0.5) and int(e[3]) == bits(40.0) and e[5:] == ["1", "0"]
    for k, (what, args, verdict) in enumerate(REFUSALS):
        got, again = M.fields(out[1 + 2 * k]), M.fields(out[2 + 2 * k])
        assert got["verdict"] == verdict, (what, got)
        if not args.startswith(("2 ", "-1 ", "4 ", "3 ")):
            assert got["entry"] == first["entry"], f"{what}: the refused call changed the setting"
        assert again == first
    # accepted: the limits themselves, a manual gain that is ignored while manual = 0, equal times, and null
    ok = ["0 12000 1 10000 10000 0 0 0", "0 12000 1e-3 1e-3 1e-3 1e30 1 0", "0 12000 0.2 50 300 0 0 nan", "0 12000 0.2 50 50 0 0 -3", "1 12000 null", "0 12000 null"]
    out = M.script(exe, "".join(f"set {a}\n" for a in ok)).strip().split("\n")
    assert [M.fields(ln)["verdict"] for ln in out] == ["OK"] * len(ok)
    none = M.fields(out[-1])["entry"].split(":")
    assert none[5] == "0" and int(none[3]) == INF_BITS, "null leaves a slot without a profile"


def test_presets_pass_validation_and_the_plan_lists_them(exe):
    want = {0: (0.2, 50.0, 300.0), 1: (0.2, 5.0, 100.0), 2: (0.2, 50.0, 2000.0)}
    for kind, (d, a, r) in want.items():
        f = M.fields(M.script(exe, f"preset {kind}\n"))
        assert f["ok"] == "1" and f["check"] == "OK"
        assert (float(f["desired"]), float(f["attack_ms"]), float(f["release_ms"]), float(f["max_gain"]), int(f["manual"])) == (d, a, r, 0.0, 0)
    assert M.fields(M.script(exe, "preset 3\n"))["ok"] == "0" and M.fields(M.script(exe, "preset -1\n"))["ok"] == "0"
    out = M.script(exe, "batch 1\nset 1 12000 0.2 5 100 0 0 0\nbatch 2\nset 1 12000 null\nbatch 3\n").strip().split("\n")
    assert M.fields(out[0]) == {"any": "0", "on": "0000"} and M.fields(out[2]) == {"any": "1", "on": "0100"} and M.fields(out[4]) == {"any": "0", "on": "0000"}


def test_manual_gain_is_reached_and_held(exe, tmp):
    """In manual mode the gain glides from where the AGC left it to manual_gain and stays.  HOW CLOSE it comes is the arithmetic
    of the unchanged gain step g <- fmaf(c, w - g, g): the step moves g only while |c (w - g)| is at least half a unit in the
    last place of g, so the gain comes to rest within 1 / (2 c) units of manual_gain - EXACTLY on it for a coefficient above
    0.5 (time constants of 0.05 ms at 12 kHz: c = 0.811), within 600 units for the 100 ms release (c = 1 / 1200.5) and within 30
    for the 5 ms attack.  Measured with this program: 0 units for the fast profile, 600 (from below, release) and 30 (from
    above, attack) for 5 / 100 ms.  Once at rest it does not move again, whatever the signal."""
    T = 14 * M.L
    x = noise(seed=6, T=T)
    t0 = 2 * M.L
    fast, slow = dict(attack_ms=0.05, release_ms=0.05), dict(attack_ms=5.0, release_ms=100.0)
    jobs, meta = [], []
    for times in (fast, slow):
        for mg in (3.0, 0.37, 250.0, 0.0, 1e-3):
            jobs.append((x, [(t0, 0, M.profile(attack_ms=5.0, release_ms=100.0)), (T - t0, 0, M.profile(manual=1, manual_gain=mg, **times))]))
            meta.append((times, np.float32(mg)))
    worst = {}
    for (times, mg), (y, g) in zip(meta, M.model_runs(exe, tmp, jobs, tag="manual")):
        before = g[t0 - 1]
        assert before != mg, "the AGC left the gain on the manual value already"
        coef = {k: np.float32(1 - math.exp(float(np.float32(-1.0) / (np.float32(times[k]) * np.float32(0.001) * np.float32(M.RATE))))) for k in times}
        c = coef["attack_ms"] if mg < before else coef["release_ms"]
        # the glide: monotone towards the manual value, never past it
        seg = g[t0:]
        assert np.all(np.diff(seg) <= 0) if mg < before else np.all(np.diff(seg) >= 0), (times, mg)
        assert np.all(seg >= mg) if mg < before else np.all(seg <= mg), "the gain went past the manual value"
        assert abs(float(seg[0]) - float(before)) <= abs(float(mg) - float(before)) * float(c) * 1.001 + 1e-30, "no glide: the first step is more than the coefficient's share"
        # at rest: the last look-ahead's worth of samples has one gain, within 1 / (2 c) units of the manual value
        rest = seg[-M.L:]
        assert np.all(rest == rest[0]), (times, mg, "still moving")
        ulp = float(np.spacing(np.float32(max(abs(float(mg)), abs(float(rest[0]))))))
        units = abs(float(rest[0]) - float(mg)) / ulp if ulp else 0.0
        bound = 0.0 if c > 0.5 else 1.0 / (2.0 * float(c))
        assert units <= bound, (times, mg, units, bound)
        worst[(times["release_ms"], mg < before)] = max(worst.get((times["release_ms"], mg < before), 0.0), units)
        if c > 0.5:
            hit = np.flatnonzero(seg == mg)
            assert hit.size and hit[0] < 256 and np.all(seg[hit[0]:] == mg), "fast profile: the gain must sit on the manual value exactly"
            k = t0 + hit[0]
            assert np.array_equal(y[k:], x[k - (M.L - 1): T - (M.L - 1)] * mg), "the delayed sample times the held gain"
    print("units from the manual value at rest:", worst)


def test_cap_holds_the_gain_on_silence(exe, tmp):
    """On digital silence the wanted gain is desired / 1e-10; a cap replaces it, and the gain climbs to the cap and no further -
    onto it exactly for a release coefficient above 0.5, to rest within 1 / (2 c) units below it otherwise (see the manual test)."""
    silence = np.zeros(12 * M.L, np.float32)
    cap = np.float32(50.0)
    runs = M.model_runs(exe, tmp, [(silence, [(silence.size, 0, M.profile(attack_ms=5.0, release_ms=100.0))]),
                                   (silence, [(silence.size, 0, M.profile(attack_ms=5.0, release_ms=100.0, max_gain=50.0))]),
                                   (silence, [(silence.size, 0, M.profile(attack_ms=0.05, release_ms=0.05, max_gain=50.0))])], tag="cap")
    (_, g0), (_, g1), (_, g2) = runs
    assert g0[-1] > 1e4 * cap, "the uncapped gain did not climb past the cap"
    assert g1.max() <= cap and np.all(np.diff(g1) >= 0) and np.all(g1[-M.L:] == g1[-1])
    assert (float(cap) - float(g1[-1])) / float(np.spacing(cap)) <= 1200.5 / 2, "at rest further below the cap than the step's rounding allows"
    assert g2.max() == cap and np.all(g2[M.L + 256:] == cap), "release coefficient 0.811: the gain sits on the cap exactly"


SYMBOLS = ("psdr_client_set_agc_profile", "psdr_agc_preset", "psdr_read_agc_gain")


def test_symbols_exist_in_the_library_and_in_the_binding():
    from phantomsdr_amd import _lib
    names = {s[0] for s in _lib.SYMBOLS}
    so = ctypes.CDLL(os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so"))
    for name in SYMBOLS:
        assert name in names, f"{name} is not bound in _lib.py"
        assert hasattr(so, name), f"{name} is not exported by the library"
    import phantomsdr_amd as P
    assert callable(P.agc_preset) and hasattr(P.AudioClient, "set_agc_profile") and hasattr(P.AudioClient, "read_agc_gain")
    assert P.agc_preset("fast") == dict(desired=0.2, attack_ms=5.0, release_ms=100.0, max_gain=0.0, manual=False, manual_gain=0.0)
    assert ctypes.sizeof(_lib.psdr_agc_profile) == 48
    with pytest.raises(P.PsdrError):
        P.agc_preset(7)

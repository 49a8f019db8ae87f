"""The squelch's host side (phantomsdr_amd/csrc/squelchplan.h) without a GPU: tests/squelch_plan_table.cpp is compiled with
the host C++ compiler - the header is plain C++17, and its step function is the text k_squelch runs - and driven by the scripts
below.  The model every flag is held against is tests/squelch_model.py, written from the words of include/psdr.h."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import squelch_model as M
from conftest import ROOT
from test_demod_plan import client, kind, ring_bytes

OK = "OK"


def build(tmp, name, extra=()):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(ROOT, "phantomsdr_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "squelch_plan_table.cpp"), "-o", exe])
    return exe


def bits(v):
    return int(np.float32(v).view(np.uint32))


# ---- the step function: random sequences with NaN, +-Inf and exact threshold hits, attack 1..5, hang 0..5, every split
def step_cases():
    rng = np.random.default_rng(20261019)
    special = [np.nan, np.inf, -np.inf, 0.0, -1.0]
    cases = []
    for k in range(2400):
        n = int(rng.integers(1, 10))
        db_open = float(rng.uniform(-40, 10))
        db_close = db_open - float(rng.choice([0.0, 0.5, 3.0, 20.0]))
        t_open, t_close = M.threshold(db_open), M.threshold(db_close)
        near = [t_open, t_close, np.nextafter(t_open, np.float32(0)), np.nextafter(t_close, np.float32(0)), np.nextafter(t_open, np.float32(np.inf))]
        pw = np.empty(n, np.float32)
        for f in range(n):
            u = rng.random()
            if u < 0.15:
                pw[f] = special[int(rng.integers(len(special)))]
            elif u < 0.45:
                pw[f] = near[int(rng.integers(len(near)))]  # exact hits and their neighbours
            else:
                pw[f] = np.float32(10.0 ** (rng.uniform(db_close - 10, db_open + 10) / 10))
        cases.append((t_open, t_close, int(rng.integers(1, 6)), int(rng.integers(0, 6)), pw))
    return cases


def long_cases():
    """batches longer than a chunk of 64 frames, transitions on the seams"""
    rng = np.random.default_rng(7)
    cases = []
    for lens in ([130], [63, 67], [64, 64, 2], [1, 128, 1], [65, 65]):
        n = sum(lens)
        t_open, t_close = M.threshold(-10.0), M.threshold(-13.0)
        pw = np.where(rng.random(n) < 0.5, np.float32(1.0), np.float32(0.001)).astype(np.float32)
        pw[60:64], pw[64:68], pw[124:128], pw[128:] = 0.001, 1.0, 1.0, 0.001  # closed up to frame 63, open from 64 (attack 1); open up to 127
        pw[rng.integers(0, n, 4)] = np.nan
        for attack, hang in ((1, 0), (2, 1), (5, 5)):
            cases.append((t_open, t_close, attack, hang, pw, lens))
    return cases


STEP_CASES, LONG_CASES = step_cases(), long_cases()
DB_GRID = [-300.0, -299.99, -150.0, -100.0, -37.5, -10.0, -3.0, -0.1, 0.0, 0.1, 3.0, 10.0, 12.34, 100.0, 150.0, 299.99, 300.0] + [x / 4 for x in range(-400, 401, 7)]


def step_input():
    lines = ["db %r" % db for db in DB_GRID]
    for t_open, t_close, attack, hang, pw in STEP_CASES:
        lines.append("steps %d %d %d %d %d %s" % (bits(t_open), bits(t_close), attack, hang, len(pw), " ".join(str(bits(v)) for v in pw)))
    for t_open, t_close, attack, hang, pw, lens in LONG_CASES:
        lines.append("run %d %d %d %d %d %d %s %s" % (bits(t_open), bits(t_close), attack, hang, len(pw), len(lens), " ".join(map(str, lens)),
                                                      " ".join(str(bits(v)) for v in pw)))
    return "\n".join(lines) + "\n"


# ---- the plan scripts
def squelch(i, on, open_db=-20.0, close_db=-23.0, attack=2, hang=3):
    return "squelch %d %d %r %r %d %d" % (i, on, open_db, close_db, attack, hang)


PLAN = ["case plan", "post off",
        *client(0, "USB"), *client(1, "AM"), *client(2, "IQ"), *client(3, "SAM"), *client(5, "TUSB"),
        squelch(1, 1), squelch(2, 1, -5.0, -5.0, 1, 0), squelch(5, 1), "pause 5", "batch",  # 0: 1 and 2 listed and fresh; 5 paused
        "batch",  # 1: nobody fresh
        squelch(1, 1, -30.0, -31.0, 4, 5), "batch",  # 2: a parameter change does NOT reset
        squelch(1, 0), "batch",  # 3: off
        squelch(1, 1), "resume 5", "batch",  # 4: off then on between batches: fresh again; 5 switched on while paused: fresh now
        "post on", "batch",  # 5: the chain on: the other audio clients as copy entries
        "remove 1", "add 1", kind(1, "AM"), "window 1 10 15.25 20", "batch",  # 6: a fresh slot: squelch off
        squelch(1, 1), "batch",  # 7: ... and on: fresh
        squelch(1, 0), squelch(2, 0), squelch(5, 0), "batch",  # 8: no squelch client
        squelch(0, 1), "remove 2", "remove 5", "remove 3", "remove 1", "batch",  # 9: the chain on, one squelch client alone
        ]
# the ring: the same script with and without squelch
RING = ["size 12 360 5", "post on", *client(0, "USB"), *client(1, "IQ"), *client(2, "TUSB"), *client(3, "SAMU"), *client(7, "FM"), *client(8, "TIQ"), "SQ 0", "SQ 1", "SQ 2",
        "SQ 8", "batch", "pause 2", "SQ 7", "batch", "post off", "resume 2", "batch", "notch-free", "batch"]


def ring_script(with_squelch):
    out = ["case ring_%d" % with_squelch]
    for ln in RING:
        if ln.startswith("SQ "):
            if with_squelch:
                out.append(squelch(int(ln.split()[1]), 1))
        elif ln != "notch-free":
            out.append(ln)
    return out


REFUSALS = [("unknown id", "squelch 4 1 -20.0 -23.0 2 3", "BAD_ID"), ("id below 0", "squelch -1 1 -20.0 -23.0 2 3", "BAD_ID"), ("id past the slots", "squelch 8 1 -20.0 -23.0 2 3", "BAD_ID"),
            ("unknown id, off", "squelch 4 0 0.0 0.0 1 0", "BAD_ID"),
            ("NaN open", "squelch 0 1 nan -23.0 2 3", "BAD_DB"), ("NaN close", "squelch 0 1 -20.0 nan 2 3", "BAD_DB"), ("Inf open", "squelch 0 1 inf -23.0 2 3", "BAD_DB"),
            ("-Inf close", "squelch 0 1 -20.0 -inf 2 3", "BAD_DB"), ("open above 300", "squelch 0 1 300.001 -23.0 2 3", "BAD_DB"), ("close below -300", "squelch 0 1 -20.0 -300.001 2 3", "BAD_DB"),
            ("close above open", "squelch 0 1 -20.0 -19.999 2 3", "CLOSE_ABOVE_OPEN"),
            ("attack 0", "squelch 0 1 -20.0 -23.0 0 3", "BAD_ATTACK"), ("attack 2^20 + 1", "squelch 0 1 -20.0 -23.0 1048577 3", "BAD_ATTACK"),
            ("hang -1", "squelch 0 1 -20.0 -23.0 2 -1", "BAD_HANG"), ("hang 2^20 + 1", "squelch 0 1 -20.0 -23.0 2 1048577", "BAD_HANG")]
ACCEPTED = ["squelch 0 1 300.0 -300.0 1048576 1048576", "squelch 0 1 -20.0 -20.0 1 0", "squelch 0 0 nan inf -5 -5"]  # the limits themselves; off ignores the rest
VALIDATION = ["case validation", *client(0, "USB"), *client(1, "AM"), squelch(1, 1, -7.0, -9.0, 3, 4), "dump"]
for _, line, _ in REFUSALS:
    VALIDATION += [line, "dump"]
for line in ACCEPTED:
    VALIDATION += [line, "dump"]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("squelch_plan")


@pytest.fixture(scope="module")
def exe(tmp):
    return build(tmp, "squelch_plan_table")


def run(exe, text, timeout=120):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def fields(ln):
    return dict(kv.split("=", 1) for kv in ln.split()[1:])


@pytest.fixture(scope="module")
def step_out(exe):
    return run(exe, step_input())


def test_db_conversion_is_numpys(step_out):
    got = [fields(ln) for ln in step_out.splitlines() if ln.startswith("db ")]
    assert len(got) == len(DB_GRID) and -300.0 in DB_GRID and 300.0 in DB_GRID
    for db, g in zip(DB_GRID, got):
        assert int(g["bits"]) == bits(np.float32(10.0 ** (db / 10))), db
    assert bits(M.threshold(-300.0)) == bits(np.float32(1e-30)) and np.isfinite(M.threshold(300.0))  # normal f32 numbers at both ends


def test_step_function_against_the_model_under_every_split(step_out):
    lines = [fields(ln) for ln in step_out.splitlines() if ln.startswith("st ")]
    at = 0
    seen = dict(nan=0, inf=0, hit=0, opened=0, closed=0, splits=0)
    for t_open, t_close, attack, hang, pw in STEP_CASES:
        flags, (o, c) = M.run(pw, t_open, t_close, attack, hang)
        want = "".join(map(str, flags))
        nsplit = 1 << (len(pw) - 1)
        for k in range(nsplit):
            g = lines[at + k]
            assert int(g["mask"]) == k
            assert (g["flags"], int(g["open"]), int(g["cnt"])) == (want, o, c), (attack, hang, pw, k)
            assert (g["frame_flags"], int(g["frame_open"]), int(g["frame_cnt"])) == (want, o, c)
        at += nsplit
        seen["splits"] += nsplit
        seen["nan"] += int(np.isnan(pw).any())
        seen["inf"] += int(np.isinf(pw).any())
        seen["hit"] += int(((pw == t_open) | (pw == t_close)).any())
        seen["opened"] += int(flags.any())
        seen["closed"] += int((np.diff(flags) < 0).any())
    assert all(v > 100 for v in seen.values()), seen  # (the sequences reach all of it)
    for t_open, t_close, attack, hang, pw, lens in LONG_CASES:
        flags, (o, c) = M.run(pw, t_open, t_close, attack, hang)
        g = lines[at]
        at += 1
        assert (g["flags"], int(g["open"]), int(g["cnt"])) == ("".join(map(str, flags)), o, c), (attack, hang, lens)
        assert g["frame_flags"] == g["flags"]
        if attack == 1 and hang == 0 and not np.isnan(pw[56:70]).any() and not np.isnan(pw[120:132]).any():
            assert (flags[63], flags[64], flags[127], flags[128]) == (0, 1, 1, 0)  # transitions on the chunk seams
    assert at == len(lines)


def test_nan_and_inf_by_hand():
    t = M.threshold(0.0)
    assert list(M.run([np.nan, 2, np.nan, np.nan, 2], t, t, 1, 1)[0]) == [0, 1, 1, 0, 1]  # never opens; counts as below
    assert list(M.run([np.inf, -np.inf, np.inf], t, t, 1, 0)[0]) == [1, 0, 1]
    assert list(M.run([1, 1, 0.5, 1, 1], t, t, 2, 0)[0]) == [0, 1, 0, 0, 1]  # an exact hit is above; the attack's last frame is heard
    assert list(M.run([1, 0, 0, 0, 1], t, t, 1, 2)[0]) == [1, 1, 1, 0, 1]  # the frame that exhausts the hang is not


def parse_batches(out, case):
    """[(lines of the demodulation plan, sq fields)] of a case"""
    res, cur, on = [], None, False
    for ln in out.splitlines():
        if ln.startswith("case "):
            on = fields(ln)["name"] == case
        elif not on:
            continue
        elif ln.startswith("batch "):
            cur = [ln]
        elif ln.startswith("sq "):
            res.append((cur, fields(ln)))
            cur = None
        elif cur is not None:
            cur.append(ln)
    return res


def entries(sq):
    return [tuple(int(v) for v in e.split(":")) for e in sq["list"].split(",")] if sq["list"] else []


def zero(sq):
    return [int(v) for v in sq["zero"].split(",")] if sq["zero"] else []


def test_plan_who_is_listed_and_who_starts_from_zero(exe):
    b = [sq for _, sq in parse_batches(run(exe, "\n".join(PLAN) + "\n"), "plan")]
    T = lambda db: bits(M.threshold(db))  # noqa: E731
    std = (2, 3, 0, T(-20.0), T(-23.0))
    e1, e2, e5 = (1,) + std, (2, 1, 0, 0, T(-5.0), T(-5.0)), (5,) + std
    # 0: the paused client is not listed and its start is still to come; an IQ client is gated like any other
    assert entries(b[0]) == [e1, e2] and zero(b[0]) == [1, 2] and (b[0]["lo"], b[0]["n"], b[0]["ncopy"]) == ("1", "2", "0")
    assert entries(b[1]) == [e1, e2] and zero(b[1]) == []
    assert entries(b[2]) == [(1, 4, 5, 0, T(-30.0), T(-31.0)), e2] and zero(b[2]) == []  # a parameter change does NOT reset
    assert entries(b[3]) == [e2] and zero(b[3]) == [] and (b[3]["lo"], b[3]["n"]) == ("2", "1")
    assert entries(b[4]) == [e1, e2, e5] and zero(b[4]) == [1, 5] and (b[4]["lo"], b[4]["n"]) == ("1", "5")  # off then on; on while paused
    # 5, the chain on: the audio clients without squelch (0 USB, 3 SAM) as copy entries behind; the IQ client has no stream
    assert entries(b[5]) == [e1, e2, e5, (0, 0, 0, 0, 0, 0), (3, 0, 0, 0, 0, 0)] and (b[5]["nsq"], b[5]["ncopy"]) == ("3", "2") and zero(b[5]) == []
    assert [e[0] for e in entries(b[6])] == [2, 5, 0, 1, 3] and zero(b[6]) == []  # a fresh slot comes without squelch
    assert [e[0] for e in entries(b[7])] == [1, 2, 5, 0, 3] and zero(b[7]) == [1]  # ... and starts from zero when it is switched on
    assert b[8]["any"] == "0" and entries(b[8]) == [] and (b[8]["lo"], b[8]["n"]) == ("0", "0")  # nothing to upload, zero or launch
    assert entries(b[9]) == [(0,) + std] and zero(b[9]) == [0] and (b[9]["lo"], b[9]["n"], b[9]["ncopy"]) == ("0", "1", "0")


def test_validation_refuses_and_changes_nothing(exe):
    out = run(exe, "\n".join(VALIDATION) + "\n").splitlines()
    sets = [i for i, ln in enumerate(out) if ln.startswith("set ")]
    dumps = [[ln for ln in out[i + 1:i + 9]] for i in sets]
    assert all(len(d) == 8 and all(ln.startswith("sqs ") for ln in d) for d in dumps)
    assert fields(out[sets[0]])["verdict"] == OK
    base = dumps[0]
    assert fields(base[1]) == dict(slot="1", active="1", on="1", topen=str(bits(M.threshold(-7.0))), tclose=str(bits(M.threshold(-9.0))), attack="3", hang="4", b_on="0", fresh="1")
    assert fields(base[0])["on"] == "0" and (fields(base[0])["attack"], fields(base[0])["hang"]) == ("1", "0")  # the defaults
    for k, (what, _, verdict) in enumerate(REFUSALS, 1):
        assert fields(out[sets[k]])["verdict"] == verdict, what
        assert dumps[k] == base, what  # nothing changed
    a = len(REFUSALS) + 1
    assert [fields(out[sets[a + k]])["verdict"] for k in range(3)] == [OK] * 3
    lim = fields(dumps[a][0])
    assert (lim["on"], lim["attack"], lim["hang"], lim["fresh"]) == ("1", "1048576", "1048576", "1") and int(lim["topen"]) == bits(np.float32(1e30))
    off = fields(dumps[a + 2][0])
    assert off["on"] == "0" and dumps[a + 2][1] == base[1]  # on = 0 ignores the other arguments


def test_the_client_ring_does_not_know_the_squelch(exe):
    a = parse_batches(run(exe, "\n".join(ring_script(1)) + "\n"), "ring_1")
    b = parse_batches(run(exe, "\n".join(ring_script(0)) + "\n"), "ring_0")
    assert len(a) == len(b) == 4
    for (pa, sa), (pb, sb) in zip(a, b):
        assert pa == pb  # the printed plan: lists, offsets, copies, what starts from zero, the slots before and after
        assert "ring_bytes=%d" % ring_bytes(12) in pa[1 + 12]
        assert sb["any"] == "0"
    assert [sq["nsq"] for _, sq in a] == ["4", "4", "5", "5"] and [sq["ncopy"] for _, sq in a] == ["2", "1", "0", "0"]


def test_sanitizers(tmp, exe):
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    # is there a sanitizer runtime at all?  Asked of an empty program, before the table program is built: a failure of THAT build
    # (an error or a warning that shows only under these flags) fails the test
    probe = tmp / "sanitizer_probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17", *flags, str(probe), "-o", str(tmp / "sanitizer_probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime to link against")
    san = build(tmp, "squelch_plan_table_san", flags)
    text = step_input() + "\n".join(PLAN + VALIDATION + ring_script(1)) + "\n"
    r = subprocess.run([san], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == run(exe, text)


def test_abi_symbols_resolve():
    so = os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so")
    lib = ctypes.CDLL(so)
    for name in ("psdr_client_set_squelch", "psdr_read_squelch", "psdr_fetched_squelch"):
        assert hasattr(lib, name), name
    from phantomsdr_amd import _lib
    declared = {s[0] for s in _lib.SYMBOLS}
    assert {"psdr_client_set_squelch", "psdr_read_squelch", "psdr_fetched_squelch"} <= declared
    with open(os.path.join(ROOT, "include", "psdr.h")) as f:
        hdr = f.read()
    assert "PSDR_OPT_SQUELCH" in hdr and "#define PSDR_OPT_SQUELCH" not in hdr and "#define PSDR_ABI_VERSION 3" in hdr

"""The impulse blanker's host side (phantomsdr_amd/csrc/blankerplan.h) without a GPU: tests/blanker_plan_table.cpp is compiled
with the host C++ compiler - the header is plain C++17, and its power, maximum and exceed functions are the text the kernels of
blanker.h run - and driven by the scripts below.  The model everything is held against is tests/nb_model.py, written from the
words of include/psdr.h; the last tests check that the streams of tests/test_gpu_blanker.py ask something of the blanker."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nb_model as M
from conftest import ROOT

CALLS = ("psdr_ring_set_blanker", "psdr_ring_read_blanker", "psdr_ring_read")
FORMATS = ("u8", "s8", "u16", "s16", "f32", "f64")


def build(tmp, name, extra=()):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(ROOT, "phantomsdr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "blanker_plan_table.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("blanker_plan")


@pytest.fixture(scope="module")
def exe(tmp):
    return build(tmp, "blanker_plan_table")


def run(exe, text, timeout=120):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def fields(ln):
    return dict(kv.split("=", 1) for kv in ln.split()[1:])


def bits(v):
    return int(np.float32(v).view(np.uint32))


def test_header_declares_and_library_exports_the_three_calls():
    with open(os.path.join(ROOT, "include", "psdr.h")) as f:
        hdr = f.read()
    assert re.search(r"int psdr_ring_set_blanker\(psdr_ctx \*ctx, int on, double threshold_db, int guard\);", hdr)
    assert re.search(r"int psdr_ring_read_blanker\(psdr_ctx \*ctx, uint64_t half_index, uint32_t \*blanked, float \*ref_level\);", hdr)
    assert re.search(r"int psdr_ring_read\(psdr_ctx \*ctx, uint64_t half_index, void \*host_half\);", hdr)
    assert "#define PSDR_ABI_VERSION 3" in hdr  # additions only
    lib = ctypes.CDLL(os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so"))
    for name in CALLS + ("psdr_debug_blanker_ptrs",):
        assert hasattr(lib, name), name
    from phantomsdr_amd import _lib
    assert set(CALLS) <= {s[0] for s in _lib.SYMBOLS}


# ---- arguments
REFUSED = [("1 -0.001 0", "BAD_DB"), ("1 90.001 0", "BAD_DB"), ("1 nan 0", "BAD_DB"), ("1 inf 0", "BAD_DB"), ("1 -inf 0", "BAD_DB"),
           ("1 10.0 -1", "BAD_GUARD"), ("1 10.0 256", "BAD_GUARD"), ("1 nan 999", "BAD_DB")]
ACCEPTED = ["1 0.0 0", "1 90.0 255", "1 12.5 7", "0 nan -5", "0 1e9 1000"]  # the limits themselves; off ignores both
DB_GRID = [0.0, 0.1, 3.0, 6.0, 10.0, 12.0, 12.34, 20.0, 45.0, 89.99, 90.0] + [x / 8 for x in range(0, 721, 7)]


def test_argument_checks_and_the_factor(exe):
    out = run(exe, "".join("check %s\n" % a for a, _ in REFUSED) + "".join("check %s\n" % a for a in ACCEPTED) + "".join("db %r\n" % d for d in DB_GRID)).splitlines()
    got = [fields(ln)["verdict"] for ln in out if ln.startswith("check ")]
    assert got == [v for _, v in REFUSED] + ["OK"] * len(ACCEPTED)
    dbs = [fields(ln) for ln in out if ln.startswith("db ")]
    assert len(dbs) == len(DB_GRID)
    for d, g in zip(DB_GRID, dbs):
        assert int(g["bits"]) == bits(M.factor(d)), d
    assert M.factor(0.0) == 1.0 and np.isfinite(M.factor(90.0))


# ---- the plan
def plans(exe, script):
    return [fields(ln) for ln in run(exe, "\n".join(script) + "\n").splitlines() if ln.startswith("plan ")]


def model_plan(calls, nhalves):
    """what the words of the header say about a sequence of calls: [(first_new, nnew, own, mirror)] and the final next"""
    nxt, fresh, out = 0, True, []
    for c in calls:
        if c == "on":
            fresh = True
            continue
        first, n = c
        own = fresh or first > nxt
        if own:
            nxt = first
        fresh = False
        new = list(range(max(first, nxt), first + n + 1))
        mirror = [j for j, h in enumerate(new) if h % nhalves == 0]
        out.append((new[0] if new else nxt, len(new), int(own), mirror[-1] if mirror else -1))
        nxt = max(nxt, first + n + 1)
    return out, nxt


def check_plan(exe, calls, nhalves=M.NHALVES, rcap=M.MAX_BATCH + 2):
    script = ["reset"] + ["on" if c == "on" else "plan %d %d %d %d" % (c[0], c[1], nhalves, rcap) for c in calls]
    got = plans(exe, script)
    want, nxt = model_plan(calls, nhalves)
    assert len(got) == len(want)
    pos = {}  # half -> ring position of its level
    for g, (first_new, nnew, own, mirror) in zip(got, want):
        assert (int(g["nnew"]), int(g["own"]), int(g["mirror"])) == (nnew, own, mirror), (g, calls)
        if nnew:
            assert int(g["first_new"]) == first_new and int(g["slot0"]) == first_new % nhalves
            prev = [int(v) for v in g["prev"].split(",")]
            for j in range(nnew):
                h = first_new + j
                pos[h] = (int(g["r0"]) + j) % rcap
                # the threshold's level: the half's own, or that of the half before - still where that half's call put it
                assert prev[j] == (pos[h] if (j == 0 and own) else pos[h - 1]), (g, h)
            live = [pos[first_new + j] for j in range(nnew)] + ([] if own else [pos[first_new - 1]])
            assert len(set(live)) == len(live)  # no level of the call overwrites one the call still reads
    assert int(got[-1]["next"]) == nxt
    return got


def test_plan_splits_rereads_jumps_mirror_and_ring_end(exe):
    a = check_plan(exe, M.SPLIT_A)
    b = check_plan(exe, M.SPLIT_B)
    assert sum(int(g["nnew"]) for g in a) == sum(int(g["nnew"]) for g in b) == M.STREAM_HALVES  # every half once, whatever the split
    assert [int(g["own"]) for g in a] == [1] + [0] * (len(a) - 1) and [int(g["own"]) for g in b] == [1] + [0] * (len(b) - 1)
    # 4+4: the first call blanks 5 halves, the others 4; the call that ends at the ring's end blanks the slot-0 half as its last
    assert [int(g["nnew"]) for g in a] == [5, 4, 4, 4, 4, 3] and [int(g["mirror"]) for g in a] == [0, 3, -1, 3, -1, -1]
    # a call that re-reads old halves blanks nothing and moves nothing; one that overlaps blanks only what is new
    g = check_plan(exe, [(0, 4), (0, 4), (2, 2), (2, 4), (1, 1)])
    assert [int(x["nnew"]) for x in g] == [5, 0, 0, 2, 0] and [int(x["next"]) for x in g] == [5, 5, 5, 7, 7]
    # a jump ahead restarts the reference; the half behind `next` exactly does not
    g = check_plan(exe, M.JUMP)
    assert [(int(x["first_new"]), int(x["nnew"]), int(x["own"])) for x in g] == [(0, 5, 1), (12, 5, 1), (17, 4, 0)]
    g = check_plan(exe, [(0, 4), (5, 2), (9, 1)])
    assert [(int(x["first_new"]), int(x["own"])) for x in g] == [(0, 1), (5, 0), (9, 1)]
    # switched on again: afresh, also for halves below the old `next`
    g = check_plan(exe, [(0, 4), "on", (4, 4), "on", (0, 2)])
    assert [(int(x["first_new"]), int(x["nnew"]), int(x["own"])) for x in g] == [(0, 5, 1), (4, 5, 1), (0, 3, 1)]
    # the end of the ring: a call from the last slot reads the mirror alone; a whole batch of max_batch + 1 new halves
    g = check_plan(exe, [(7, 1), (8, 4)])
    assert [(int(x["slot0"]), int(x["nnew"]), int(x["mirror"])) for x in g] == [(7, 2, 1), (1, 4, -1)]
    g = check_plan(exe, [(4, 4)], nhalves=8, rcap=6)
    assert (int(g[0]["nnew"]), int(g[0]["mirror"])) == (5, 4)
    check_plan(exe, [(f, 3) for f in range(0, 300, 3)], nhalves=9, rcap=5)  # the ring of levels wraps many times


# ---- power, maximum, exceed
def chunk_cases():
    rng = np.random.default_rng(20261019)
    cases = []
    edge = {"u8": [0, 255, 128, 127], "s8": [-128, 127, 0, -1], "u16": [0, 65535, 32768, 32767], "s16": [-32768, 32767, 0, -1]}
    fl = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-30, 3e38, 1e20, -1e20, 1.5, 2.0 ** -140, 16777217.0]
    for fmt in FORMATS:
        dt = M.DTYPE[fmt]
        n = 16 // np.dtype(dt).itemsize
        for k in range(60):
            if fmt in edge:
                info = np.iinfo(dt)
                c = rng.integers(info.min, info.max + 1, n).astype(dt)
                if k < 8:
                    c[:] = edge[fmt][k % 4]  # the flipped extremes in BOTH components: s16 at -32768 twice is 2^31
                elif k < 30:
                    c[rng.integers(0, n, 3)] = rng.choice(edge[fmt], 3).astype(dt)
            else:
                c = (rng.standard_normal(n) * 10.0 ** rng.uniform(-20, 20)).astype(dt)
                if k < 40:
                    c[rng.integers(0, n, 1)] = rng.choice(fl)
            for is_real in (False, True):
                cases.append((fmt, is_real, c))
    return cases


CHUNKS = chunk_cases()


def test_power_functions_against_the_model_on_all_formats(exe):
    text = "".join("chunk %d %d %s\n" % (M.FMT_ID[f], r, " ".join(str(int(w)) for w in c.view(np.uint32))) for f, r, c in CHUNKS)
    out = [fields(ln) for ln in run(exe, text).splitlines() if ln.startswith("chunk ")]
    assert len(out) == len(CHUNKS)
    seen = dict(nan=0, inf=0, two31=0)
    for (fmt, is_real, c), g in zip(CHUNKS, out):
        P = M.power(c, fmt, is_real)
        want = [bits(p) for p in P]
        assert int(g["n"]) == len(P) and int(g["sb"]) == c.itemsize * (1 if is_real else 2)
        assert [int(v) for v in g["p"].split(",")] == want, (fmt, is_real, c)
        assert [int(v) for v in g["s"].split(",")] == want, (fmt, is_real, c)  # sample by sample: the marking kernel's way
        assert int(g["max"]) == bits(M.maximum(P)) == bits(M.block_maxima(np.resize(P, M.BLOCK))[0])
        assert int(g["zero"]) == int(np.full(4 // min(4, c.itemsize), M.zero_code(fmt)).view(np.uint32)[0]) if fmt in M.OFFSET else int(g["zero"]) == 0
        seen["nan"] += int(np.isnan(P).any())
        seen["inf"] += int(np.isinf(P).any())
        seen["two31"] += int((P == np.float32(2.0 ** 31)).any())
    assert all(v > 0 for v in seen.values()), seen
    assert bits(M.power(np.array([-32768, -32768], np.int16), "s16", False)[0]) == bits(2.0 ** 31)
    assert M.power(np.array([0, 0], np.uint16), "u16", False)[0] == 2.0 ** 31 and M.power(np.array([255], np.uint8), "u8", True)[0] == 127.0 ** 2


def test_comparisons_nan_inf_and_the_threshold_that_blanks_nothing(exe):
    vals = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), 3.4028235e38, 1e-45]
    text, want = "", []
    for p in vals:
        for t in vals:
            for m in (0.0, 1.0, np.inf):
                text += "cmp %d %d %d\n" % (bits(p), bits(t), bits(m))
                with np.errstate(invalid="ignore"):
                    want.append((int(np.float32(p) > np.float32(t)), int(np.float32(t) > 0 and np.isfinite(np.float32(t))),
                                 bits(np.float32(p) if np.float32(p) > np.float32(m) else np.float32(m))))
    out = [fields(ln) for ln in run(exe, text).splitlines()]
    assert [(int(g["exceed"]), int(g["valid"]), int(g["max"])) for g in out] == want
    # by hand: a NaN never exceeds and is never a maximum; T = 0 and T = Inf blank nothing
    raw = np.array([1.0, np.nan, 5.0, 0.0] * 64, np.float32)
    assert M.block_maxima(M.power(raw, "f32", True))[0] == 25.0
    assert M.blank(raw, "f32", True, np.float32(0.0), 3)[1] == 0 and M.blank(raw, "f32", True, np.float32(np.inf), 3)[1] == 0
    out, n = M.blank(raw, "f32", True, np.float32(24.0), 1)
    assert n == 64 * 3 and out[5] == 0 and out[2] == 0 and out[1] == 0 and out[0] == 1.0 and out[4] == 1.0  # a NaN inside a guard is zeroed like any sample
    assert np.isnan(M.blank(raw, "f32", True, np.float32(24.0), 0)[0][1])  # ... and never on its own account


def test_sanitizers(tmp, exe):
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    probe = tmp / "sanitizer_probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17", *flags, str(probe), "-o", str(tmp / "sanitizer_probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime to link against")
    san = build(tmp, "blanker_plan_table_san", flags)
    text = "".join("chunk %d %d %s\n" % (M.FMT_ID[f], r, " ".join(str(int(w)) for w in c.view(np.uint32))) for f, r, c in CHUNKS)
    text += "reset\n" + "".join("plan %d %d 8 6\n" % c for c in M.SPLIT_B + M.JUMP) + "check 1 nan 3\ndb 90.0\n"
    r = subprocess.run([san], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == run(exe, text)


# ---- the GPU test's streams ask something of the blanker
GPU_CASES = [(f, False) for f in FORMATS] + [("s16", True), ("f32", True)]


@pytest.mark.parametrize("fmt,is_real", GPU_CASES)
@pytest.mark.parametrize("guard", [0, 7, 255])
def test_fixture_blanks_every_planted_impulse_and_nothing_else(fmt, is_real, guard):
    hs = M.shape(is_real) // 2
    for calls in (M.SPLIT_A, M.JUMP):
        halves, pl = M.fixture(fmt, is_real, guard)
        raw = [h.copy() for h in halves]
        nb = M.Blanker(fmt, is_real, M.THRESHOLD_DB, guard)
        seen = {}
        for first, n in calls:
            seen.update(nb.process(halves, first, n))
        assert len(seen) == (M.STREAM_HALVES if calls is M.SPLIT_A else 14)
        assert any(h in seen for h, _, _ in pl)
        for h, (count, R) in seen.items():
            want = M.expected_hits(hs, pl, h, guard)
            zeroed = (halves[h].reshape(hs, -1) == M.zero_code(fmt)).all(axis=1) & ~(raw[h].reshape(hs, -1) == M.zero_code(fmt)).all(axis=1)
            assert count == int(want.sum()), (h, count)  # every planted impulse with its full guard, nothing in a half without one
            assert not (zeroed & ~want).any() and R > 0 and np.isfinite(R)
            keep = ~want
            assert np.array_equal(halves[h].reshape(hs, -1)[keep].view(np.uint8), raw[h].reshape(hs, -1)[keep].view(np.uint8))
    # at 90 dB the plain noise is left alone
    halves, _ = M.fixture(fmt, is_real, guard, planted=False)
    nb = M.Blanker(fmt, is_real, 90.0, guard)
    assert all(c == 0 for first, n in M.SPLIT_A for c, _ in nb.process(halves, first, n).values())

"""The audio blanker's host side (phantomsdr_amd/csrc/anbplan.h) without a GPU: tests/anb_plan_table.cpp is compiled with the host
C++ compiler - the header is plain C++17, and its detector and gap repair are the text k_audio_nb runs - and driven by the scripts
below.  tests/anb_model.py holds an independent float64 model of the rule.  The measured figures go to
build/records/anb_host.jsonl."""
import ctypes
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import anb_model as M
from conftest import ROOT
from helpers import CLIENT_KINDS
from test_demod_plan import client, kind

NAMES = list(CLIENT_KINDS)
AUDIO_KINDS = [k for k in NAMES if CLIENT_KINDS[k][0] != "IQ"]
NORMAL = (4.5, 7)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("anb_host")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


def run(exe, text, timeout=120):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def fields(ln):
    return dict(kv.split("=", 1) for kv in ln.split()[1:])


def record(name, **figures):
    d = os.path.join(ROOT, "build", "records")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "anb_host.jsonl"), "a") as f:
        f.write(json.dumps(dict(test=name, **figures)) + "\n")


def batches_of(split, F):
    out, left, k = [], F, 0
    while left > 0:
        out.append(min(split[k % len(split)], left))
        left -= out[-1]
        k += 1
    return out


def bits(v):
    return int(np.float32(v).view(np.uint32))


@functools.lru_cache(maxsize=None)
def coloured(n, seed=20261020):
    """low-pass-coloured noise plus a tone, rms about 1"""
    w = np.random.default_rng(seed).standard_normal(n + 16)
    x = np.convolve(w, np.ones(6) / np.sqrt(6.0), mode="full")[8:8 + n] + 0.7 * np.cos(2 * np.pi * 0.043 * np.arange(n) + 0.4)
    return (x / np.sqrt(np.mean(x ** 2))).astype(np.float32)


def spiked(n, centres, amp=25.0, seed=20261020):
    x = coloured(n, seed).copy()
    for k, c in enumerate(centres):
        x[c] += amp if k % 2 == 0 else -amp
    return x


def one(exe, tmp, x, h, frames=None, par=NORMAL, flags=None, tag="one"):
    F = len(x) // h
    fl = np.zeros(F, np.int32) if flags is None else flags
    return M.run_streams(exe, tmp, [(par[0], par[1], x, fl, h, frames or [F])], tag)[0]


# ---- batches, delay, contraction ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", (4, 6, 180))
def test_any_split_into_batches_gives_the_same_bits(exe, tmp, h):
    F = 700 if h < 180 else 41
    x = spiked(h * F, [0, 255, 300, 511, 513, 769, 1000, 1290, 1300, 2047, 2049][:11 if h * F > 2100 else 9])
    flags = np.zeros(F, np.int32)
    splits = [(F,), (1,), (1, 3, 70), (2,), (71, 3, 1)]
    res = M.run_streams(exe, tmp, [(4.5, 7, x, flags, h, batches_of(s, F)) for s in splits], "split%d_" % h)
    rows0, st0, tr0 = res[0]
    assert len(tr0["order"]) == M.blocks_done(h * F) and int(st0[-1]["pos"]) == h * F and len(tr0["centres"]) >= 9
    assert not rows0[:M.D].view(np.uint32).any(), "the first D outputs are +0.0"
    assert rows0[M.D:].any()
    for s, (rows, st, tr) in zip(splits[1:], res[1:]):
        assert rows.tobytes() == rows0.tobytes(), s
        assert tr["centres"].tobytes() == tr0["centres"].tobytes() and tr["m"].tobytes() == tr0["m"].tobytes(), s
        assert (int(st[-1]["impulses"]), int(st[-1]["samples"])) == (int(st0[-1]["impulses"]), int(st0[-1]["samples"])) == (len(tr0["centres"]), int(st0[-1]["samples"]))
        cur = int(st[-1]["cur"]) & 1
        assert st[-1]["hist"][cur].tobytes() == st0[-1]["hist"][int(st0[-1]["cur"]) & 1].tobytes(), s


def test_contraction_cannot_change_a_bit(exe, tmp):
    """the table program built to fuse whatever may be fused (-mfma -ffp-contract=fast, -O2) against one that may fuse nothing"""
    if " fma " not in open("/proc/cpuinfo").read():
        pytest.skip("this CPU has no FMA instruction to contract into")
    fast = M.build_table(tmp, ROOT, ("-O2", "-mfma", "-ffp-contract=fast"), "anb_plan_table_fast")
    off = M.build_table(tmp, ROOT, ("-O2", "-ffp-contract=off"), "anb_plan_table_off")
    x = spiked(180 * 30, [100, 255, 600, 1023, 1026, 3000])
    jobs = [(t, w, x, np.zeros(30, np.int32), 180, [30]) for t, w in ((2.0, 15), (4.5, 7), (3.5, 11))]
    for (ra, sa, ta), (rb, sb, tb), (rc, _, _) in zip(M.run_streams(fast, tmp, jobs, "fast"), M.run_streams(off, tmp, jobs, "off"), M.run_streams(exe, tmp, jobs, "o1")):
        assert ra.tobytes() == rb.tobytes() == rc.tobytes() and sa.tobytes() == sb.tobytes() and ta["m"].tobytes() == tb["m"].tobytes()
        assert len(ta["centres"]) >= 6


def test_no_detection_is_the_input_delayed_bit_for_bit(exe, tmp):
    x = coloured(180 * 20)
    rows, st, tr = one(exe, tmp, x, 180, par=(12.0, 3))
    assert len(tr["centres"]) == 0 and int(st[-1]["impulses"]) == 0
    assert rows[M.D:].tobytes() == x[:-M.D].tobytes() and not rows[:M.D].view(np.uint32).any()


# ---- the float64 model ------------------------------------------------------------------------------------------------------------
MODEL_INPUTS = {
    "spikes": lambda: (spiked(180 * 30, [0, 255, 300, 511, 513, 1000, 1004, 3000, 4095, 4100]), NORMAL),
    "noise at 2 sigma": lambda: (coloured(180 * 12, 7), (2.0, 15)),
    "strong": lambda: (spiked(180 * 20, [37, 700, 1500, 2303, 2306], 40.0, 11), (3.5, 11)),
}
MARGIN = 1e-3   # the float64 model's |m| / T stays this far off 1 on every input (asserted): f32 moves the ratio by about 1e-6


def test_the_float64_model_finds_the_same_centres_and_the_same_repairs(exe, tmp):
    """Tolerance: the repaired samples of the f32 header against the float64 model, relative to the input's rms (1).  The largest
    difference over all inputs is measured and recorded; the bound asserted is 2e-4: 15 steps of a 10-tap recursion amplify the
    f32 rounding of a[] (about 1e-6 relative, Levinson-Durbin over sums of 256 terms) and of the seeds by the predictor's gain, a
    few tens; the measured value is recorded beside it and lies more than a decade below the bound."""
    worst = 0.0
    for name, make in MODEL_INPUTS.items():
        x, par = make()
        rows, st, tr = one(exe, tmp, x, 180, par=par, tag="model")
        y, centres, ratio, orders = M.model(x.astype(np.float64), *par)
        off = float(np.abs(ratio[ratio > 0] - 1).min())
        assert off >= MARGIN, (name, off)
        assert tr["centres"].tolist() == centres.tolist(), name
        assert tr["order"].tolist() == orders
        want = M.delayed(y, len(x))
        final = M.D + (M.blocks_done(len(x)) - 1) * M.B - 8  # processed samples behind this still wait for the next block
        err = float(np.abs(rows[:final] - want[:final]).max())
        pl = (par[1] - 1) // 2
        gap = np.zeros(len(x), bool)
        for c in centres:
            gap[max(c - pl, 0):c + pl + 1] = True
        through = ~M.delayed(gap, len(x))[:final]
        assert rows[:final][through].tobytes() == M.delayed(x, len(x))[:final][through].tobytes(), (name, "a sample outside every gap passes through")
        print(f"{name}: centres {len(centres)} nearest |m|/T to 1: {off:.2e}; repaired samples max abs diff {err:.3e}")
        record("model", input=name, centres=len(centres), nearest_ratio_margin=off, repaired_max_abs_diff=err, bound=2e-4)
        worst = max(worst, err)
        assert len(centres) >= 5
    assert worst <= 2e-4, worst


# ---- crafted inputs -------------------------------------------------------------------------------------------------------------
def gaps_of(tr, width):
    pl = (width - 1) // 2
    return [(int(c) - pl, int(c) + pl) for c in tr["centres"]]


def test_gaps_across_block_and_batch_boundaries_and_overlapping_gaps(exe, tmp):
    h, F = 4, 600
    n = h * F
    # 254: reaches forward into block 1; 513: reaches back into block 1; 1000 and 1004: overlapping, the later wins; 1198..1202
    # straddles the batch boundary at 1200
    x = spiked(n, [254, 513, 1000, 1004, 1200])
    rows, st, tr = one(exe, tmp, x, h, frames=[300, 300])
    g = gaps_of(tr, 7)
    c = tr["centres"].tolist()
    assert {254, 513, 1200} <= set(c)
    assert any(lo // 256 < hi // 256 and ce // 256 == lo // 256 for (lo, hi), ce in zip(g, c)), "forward across a block boundary"
    assert any(lo // 256 < hi // 256 and ce // 256 == hi // 256 for (lo, hi), ce in zip(g, c)), "backward across a block boundary"
    assert any(lo < 1200 <= hi for lo, hi in g), "across the batch boundary"
    unsplit, _, _ = one(exe, tmp, x, h)
    assert rows.tobytes() == unsplit.tobytes()
    # the overlap: the model applies gaps in the order of the centres, so the later centre's values stand
    y, centres, _, _ = M.model(x.astype(np.float64), *NORMAL)
    pairs = [(a, b) for a, b in zip(c, c[1:]) if b - a <= 6]
    assert pairs, c
    assert np.abs(rows[M.D:] - y[:n - M.D])[:M.blocks_done(n) * 256 - 264].max() <= 2e-4


def test_centres_at_the_first_and_the_last_processed_sample(exe, tmp):
    h = 4
    n = 256 * 5 + 24          # exactly five blocks are complete
    n += (-n) % h
    assert M.blocks_done(n) == 5
    x = spiked(n, [0, 5 * 256 - 1])
    rows, st, tr = one(exe, tmp, x, h)
    assert tr["centres"][0] == 0 and tr["centres"][-1] == 5 * 256 - 1
    assert int(st[-1]["samples"]) == 7 * len(tr["centres"]) - 3  # the three samples in front of the stream do not count
    more = np.concatenate([x, coloured(1200, 3)])
    rows2, _, tr2 = one(exe, tmp, more, h)
    y, centres, _, _ = M.model(more.astype(np.float64), *NORMAL)
    assert 1279 in centres.tolist() and np.abs(rows2[M.D:M.D + 1290] - y[:1290]).max() <= 2e-4


def test_the_cap_of_16_impulses_per_block(exe, tmp):
    h = 4
    c = [256 + 8 + 12 * k for k in range(20)]
    x = spiked(256 * 8, c, 60.0)
    rows, st, tr = one(exe, tmp, x, h, par=(2.0, 3))
    in1 = [v for v in tr["centres"].tolist() if 256 <= v < 512]
    assert len(in1) == 16 and in1 == sorted(in1)
    tail = slice(M.D + in1[-1] + 2, M.D + 512 - 1)
    assert rows[tail].tobytes() == x[in1[-1] + 2:511].tobytes(), "behind the 16th gap the block passes through"


def test_an_all_zero_block_and_a_block_with_a_non_finite_r0(exe, tmp):
    h = 4
    x = coloured(256 * 8).copy()
    x[512:768] = 0
    x[1024:1280] *= np.float32(3e19)   # squares overflow: R[0] = +Inf
    x[1700] += 30
    rows, st, tr = one(exe, tmp, x, h)
    assert tr["order"][2] == -1 and tr["order"][4] == -1 and tr["order"][1] >= 1
    assert not [c for c in tr["centres"].tolist() if 512 <= c < 768 or 1024 <= c < 1280]
    assert 1700 in tr["centres"].tolist()
    assert np.isfinite(rows[:M.D + 1000]).all()
    assert rows[M.D + 520:M.D + 760].tobytes() == x[520:760].tobytes()


def test_levinson_stops_early_on_a_pure_tone(exe, tmp):
    """A pure tone's autocorrelation R[i] = cos(w i) is singular from order 2 on: the error of order 2 is zero but for rounding, so
    anb_levinson keeps the filter of the order where its error stops being positive and finite, and the higher coefficients are 0.
    (Over a block of a stream - each product with both factors inside the block - a tone's R is never singular: the edges keep
    every order's error positive, asserted below, and the block is handled like any other.)"""
    stopped = 0
    for w in (0.3, 0.785398, 1.0, 2.0, 2.5):
        R = np.cos(w * np.arange(M.P + 1)).astype(np.float32)
        f = fields(run(exe, "levinson " + " ".join("%.9g" % v for v in R) + "\n").splitlines()[0])
        order, a = int(f["order"]), [float(v) for v in f["a"].split(",")]
        assert 1 <= order <= M.P and a[0] == 1.0 and all(v == 0.0 for v in a[order + 1:]) and all(np.isfinite(a))
        if order < M.P:
            stopped += 1
    assert stopped >= 3, stopped
    f = fields(run(exe, "levinson 1 0 0 0 0 0 0 0 0 0 nan\n").splitlines()[0])
    assert int(f["order"]) == 9  # a value that is not finite ends the recursion, the filter before it stands
    x = np.cos(2 * np.pi * 0.125 * np.arange(256 * 6)).astype(np.float32)
    rows, st, tr = one(exe, tmp, x, 4)
    assert (tr["order"] == M.P).all() and np.isfinite(rows).all() and np.isfinite(tr["level"]).all()


def test_a_flagged_frame_enters_as_zeros_and_keeps_its_row(exe, tmp):
    for h in (4, 6, 180):
        F = 700 if h < 180 else 30
        x = spiked(h * F, [300, 1000, 1500]).copy()
        flags = np.zeros(F, np.int32)
        bad = [F // 3, F // 3 + 1, F - 2]
        flags[bad] = 1
        for f in bad:
            x[f * h] = np.nan
            x[f * h + 1:(f + 1) * h].view(np.uint32)[:] = 0x7FC01234
        clean = np.where(np.repeat(flags, h) != 0, np.float32(0), x)
        jobs = [(4.5, 7, x, flags, h, batches_of(s, F)) for s in ((F,), (1,), (3, 70))] + [(4.5, 7, clean, np.zeros(F, np.int32), h, [F])]
        res = M.run_streams(exe, tmp, jobs, "flag")
        keep = np.repeat(flags, h) == 0
        for rows, st, tr in res[:3]:
            assert rows[~keep].tobytes() == x[~keep].tobytes()  # NaN bits included
            assert rows[keep].tobytes() == res[3][0][keep].tobytes() and np.isfinite(rows[keep]).all()
            assert tr["centres"].tobytes() == res[3][2]["centres"].tobytes()


# ---- repair quality -------------------------------------------------------------------------------------------------------------
def test_repair_brings_the_gaps_closer_to_the_clean_signal(exe, tmp):
    """Spikes of 25 x rms on low-pass-coloured noise plus a tone.  Over the gaps' samples the rms error against the clean signal,
    unrepaired over repaired: the factor is measured on the float64 model and recorded; asserted of the header's run: half of it."""
    n = 180 * 60
    centres = list(range(400, n - 800, 487))
    clean = coloured(n)
    x = spiked(n, centres)
    rows, st, tr = one(exe, tmp, x, 180)
    y, found, _, _ = M.model(x.astype(np.float64), *NORMAL)
    assert set(centres) <= set(found.tolist())
    gap = np.zeros(n, bool)
    for c in found:
        gap[c - 3:c + 4] = True
    final = (M.blocks_done(n) - 1) * 256 - 8
    gap[final:] = False
    rms = lambda v: float(np.sqrt(np.mean(np.square(v, dtype=np.float64))))  # noqa: E731
    before = rms(x[gap].astype(np.float64) - clean[gap])
    model_factor = before / rms(y[gap] - clean[gap])
    got = rows[M.D:].astype(np.float64)[:n - M.D]
    factor = before / rms(got[gap[:n - M.D]] - clean[:n - M.D][gap[:n - M.D]])
    print(f"gap error: unrepaired {before:.3f}, model factor {model_factor:.2f}, header factor {factor:.2f}")
    record("repair_quality", spikes=len(centres), unrepaired_rms=before, model_factor=model_factor, header_factor=factor, asserted=0.5 * model_factor)
    assert model_factor > 2 and factor >= 0.5 * model_factor


# ---- refusals, presets ----------------------------------------------------------------------------------------------------------
REFUSALS = [
    ("id below 0", "anb -1 1 4.5 7", "BAD_ID"), ("id past the slots", "anb 8 1 4.5 7", "BAD_ID"), ("id past the slots, off", "anb 9 0 0 0", "BAD_ID"),
    ("no client", "anb 4 1 4.5 7", "INACTIVE"), ("no client, off", "anb 4 0 0 0", "INACTIVE"),
    ("IQ client", "anb 2 1 4.5 7", "IQ"),
    ("NaN threshold", "anb 0 1 nan 7", "NONFINITE"), ("Inf threshold", "anb 0 1 inf 7", "NONFINITE"), ("-Inf threshold", "anb 0 1 -inf 7", "NONFINITE"),
    ("threshold below 2", "anb 0 1 1.9 7", "BAD_THRESHOLD"), ("threshold above 12", "anb 0 1 12.5 7", "BAD_THRESHOLD"),
    ("even width", "anb 0 1 4.5 6", "BAD_WIDTH"), ("width below 3", "anb 0 1 4.5 1", "BAD_WIDTH"), ("width above 15", "anb 0 1 4.5 17", "BAD_WIDTH"),
    ("negative width", "anb 0 1 4.5 -3", "BAD_WIDTH"),
    # the precedence: id, client, IQ, non-finite, threshold, width
    ("id before everything", "anb 8 1 nan 4", "BAD_ID"), ("client before IQ and numbers", "anb 4 1 nan 4", "INACTIVE"), ("IQ before the numbers", "anb 2 1 nan 4", "IQ"),
    ("non-finite before width", "anb 0 1 nan 4", "NONFINITE"), ("threshold before width", "anb 0 1 99 4", "BAD_THRESHOLD"),
]
ACCEPTED = ["anb 0 1 2 3", "anb 0 1 12 15", "anb 2 0 nan 4", "anb 0 0 99 4"]


def test_refusals_in_order_and_nothing_changes(exe):
    lines = ["case validation", *client(0, "USB"), *client(1, "AM"), *client(2, "IQ"), "anb 1 1 4.5 7", "dump"]
    for _, line, _ in REFUSALS:
        lines += [line, "dump"]
    for line in ACCEPTED:
        lines += [line, "dump"]
    out = run(exe, "\n".join(lines) + "\n").splitlines()
    sets = [i for i, ln in enumerate(out) if ln.startswith("set ")]
    verdicts = [fields(out[i])["verdict"] for i in sets]
    dumps = [out[i + 1:i + 9] for i in sets]
    base = dumps[0]
    f1 = fields(base[1])
    assert verdicts[0] == "OK" and (f1["on"], f1["fresh"], f1["width"]) == ("1", "1", "7") and int(f1["threshold"]) == bits(4.5)
    assert {v for _, _, v in REFUSALS} == {"BAD_ID", "INACTIVE", "IQ", "NONFINITE", "BAD_THRESHOLD", "BAD_WIDTH"}
    for k, (what, _, verdict) in enumerate(REFUSALS, 1):
        assert verdicts[k] == verdict, what
        assert dumps[k] == base, what
    a = len(REFUSALS) + 1
    assert verdicts[a:] == ["OK"] * len(ACCEPTED)
    d = [fields(x[0]) for x in dumps[a:]]
    assert (d[0]["on"], int(d[0]["threshold"]), d[0]["width"]) == ("1", bits(2.0), "3")  # the limits themselves pass
    assert (d[1]["on"], int(d[1]["threshold"]), d[1]["width"]) == ("1", bits(12.0), "15")
    assert d[3]["on"] == "0" and d[3]["width"] == "15"  # off ignores the numbers


def test_presets(exe):
    out = [fields(ln) for ln in run(exe, "".join("preset %d\n" % k for k in (0, 1, 2, 3, 4, -1))).splitlines()]
    assert [(o["ok"], float(o["threshold"]), int(o["width"])) for o in out[1:4]] == [("1", 6.0, 5), ("1", 4.5, 7), ("1", 3.5, 11)]
    assert [o["ok"] for o in out] == ["0", "1", "1", "1", "0", "0"]


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def entries(p):
    return [tuple(int(v) for v in e.split(":")) for e in p["list"].split(",")] if p["list"] else []


def zero(p):
    return [int(v) for v in p["zero"].split(",")] if p["zero"] else []


def test_plan_who_is_listed_and_whose_state_is_fresh(exe):
    """tests/test_nr_host.py's cases, for the blanker"""
    P = len(NAMES)  # the paused client's slot
    lines = ["case plan", "size 16 360 5"]
    for i, k in enumerate(NAMES):
        lines += client(i, k) + (["anb %d 1 4.5 7" % i] if CLIENT_KINDS[k][0] != "IQ" else [])
    lines += client(P, "USB") + ["anb %d 1 6 5" % P, "pause %d" % P, "batch",  # 0
                                 "batch",  # 1: nobody fresh
                                 "anb 0 1 3.5 11", "resume %d" % P, "batch",  # 2: new numbers: fresh; switched on while paused: fresh now
                                 kind(NAMES.index("AM"), "FM"), "window 1 30 35.5 40", "window 3 10 15.75 20", "window 4 10 16.25 20", "batch",  # 3: mode; retune; mid inside its bin; floor(mid)
                                 kind(0, "IQ"), "batch", kind(0, "USB"), "batch",  # 4, 5: USB -> IQ -> USB: not listed, then the state stood still
                                 "anb 6 0 0 0", "remove 3", "add 3", kind(3, "FM"), "window 3 10 15.25 20", "batch",  # 6: off; a fresh slot comes without
                                 "anb 6 1 4.5 7", "batch",  # 7: off and on again: fresh
                                 ]
    for i in range(P + 1):
        lines.append("anb %d 0 0 0" % i)
    lines += ["batch"]  # 8: nobody
    b = [fields(ln) for ln in run(exe, "\n".join(lines) + "\n").splitlines() if ln.startswith("anbp ")]
    audio = [NAMES.index(k) for k in AUDIO_KINDS]
    am = NAMES.index("AM")
    assert len(audio) == 9 and [e[0] for e in entries(b[0])] == audio and zero(b[0]) == audio  # IQ, TIQ and the paused one are not listed
    assert all(e[1:] == (bits(4.5), 7) for e in entries(b[0]))
    assert [e[0] for e in entries(b[1])] == audio and zero(b[1]) == []
    assert [e[0] for e in entries(b[2])] == audio + [P] and zero(b[2]) == [0, P] and entries(b[2])[0][1:] == (bits(3.5), 11)
    assert zero(b[3]) == sorted([am, 1, 4]) and 3 not in zero(b[3])
    assert 0 not in [e[0] for e in entries(b[4])] and zero(b[4]) == []
    assert 0 in [e[0] for e in entries(b[5])] and zero(b[5]) == []
    assert [e[0] for e in entries(b[6])] == [i for i in audio + [P] if i not in (3, 6)] and zero(b[6]) == []
    assert zero(b[7]) == [6]
    assert b[8]["any"] == "0" and entries(b[8]) == [] and zero(b[8]) == []


def test_plan_of_a_context_without_such_clients(exe):
    lines = ["case none", *client(0, "USB"), *client(1, "AM"), "batch", "batch"]
    b = [fields(ln) for ln in run(exe, "\n".join(lines) + "\n").splitlines() if ln.startswith("anbp ")]
    assert len(b) == 2 and all(x["have"] == "0" and x["any"] == "0" and x["list"] == "" for x in b)


def test_the_demodulation_plan_does_not_know_the_blanker(exe):
    def script(with_nb):
        out = ["case ring", "size 12 360 5", "post on"]
        for i, k in ((0, "USB"), (1, "IQ"), (2, "TUSB"), (3, "SAMU"), (7, "FM"), (8, "TIQ")):
            out += client(i, k) + (["anb %d 1 4.5 7" % i] if with_nb else [])
        return out + ["batch", "pause 2", "batch", "post off", "resume 2", "batch"]
    plan = lambda text: [ln for ln in text.splitlines() if not ln.startswith(("anbp ", "set "))]  # noqa: E731
    assert plan(run(exe, "\n".join(script(True)) + "\n")) == plan(run(exe, "\n".join(script(False)) + "\n"))


def test_sanitizers(tmp, exe):
    """the table program as a stand-alone program under AddressSanitizer and UBSan: ragged batches at every h, a centre at the
    stream's first sample, a flagged frame, the validation script"""
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    probe = tmp / "sanitizer_probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17", *flags, str(probe), "-o", str(tmp / "sanitizer_probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime to link against")
    san = M.build_table(tmp, ROOT, flags, "anb_plan_table_san")
    jobs = []
    for h, F in ((4, 1), (4, 70), (4, 71), (4, 400), (6, 43), (6, 300), (180, 1), (180, 2), (180, 9)):
        fl = np.zeros(F, np.int32)
        fl[F // 2] = F > 4
        x = spiked(h * F, [c for c in (0, 255, 300, 511, 1000) if c < h * F])
        for s in ((F,), (1,), (3, 70, 1)):
            jobs.append((2.0, 15, x, fl, h, batches_of(s, F)))
    for (ra, sa, ta), (rb, sb, tb) in zip(M.run_streams(san, tmp, jobs, "san"), M.run_streams(exe, tmp, jobs, "ref")):
        assert ra.tobytes() == rb.tobytes() and sa.tobytes() == sb.tobytes() and ta["centres"].tobytes() == tb["centres"].tobytes()
    text = "\n".join(["case v", *client(0, "USB"), *client(2, "IQ")] + [line for _, line, _ in REFUSALS] + ["batch", "anb 0 1 4.5 7", "batch", "dump"]) + "\n"
    r = subprocess.run([san], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == run(exe, text)


def test_abi_symbols_and_constants():
    lib = ctypes.CDLL(os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so"))
    names = ("psdr_client_set_audio_blanker", "psdr_audio_blanker_preset", "psdr_read_audio_blanker")
    for name in names:
        assert hasattr(lib, name), name
    import phantomsdr_amd as p
    from phantomsdr_amd import _lib
    assert set(names) <= {s[0] for s in _lib.SYMBOLS}
    hdr = open(os.path.join(ROOT, "include", "psdr.h")).read()
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(PSDR_ANB_[A-Z]+|PSDR_OPT_AUDIO_BLANKER)\s+(\d+)", hdr))
    assert defs == {"PSDR_ANB_LIGHT": p.ANB_LIGHT, "PSDR_ANB_NORMAL": p.ANB_NORMAL, "PSDR_ANB_STRONG": p.ANB_STRONG, "PSDR_OPT_AUDIO_BLANKER": p.Context.OPT_AUDIO_BLANKER}
    assert "#define PSDR_ABI_VERSION 3" in hdr and p.Context.OPT_AUDIO_BLANKER == 10
    # the preset helper needs no context (and no device)
    assert [p.audio_blanker_preset(k) for k in ("light", "normal", "strong")] == [(6.0, 5), (4.5, 7), (3.5, 11)]
    with pytest.raises(p.PsdrError) as e:
        p.audio_blanker_preset(0)
    assert e.value.code == -1 and "unknown kind 0" in str(e.value)

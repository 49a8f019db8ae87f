"""The forward path's planners (phantomsdr_amd/csrc/forwardplan.h) without a GPU and without the library:
tests/forward_plan_table.cpp is compiled with the host C++ compiler - the header is plain C++17 - and runs the script below.
Three planners: the chain segments of the fused real second pass (which batches hand off, the table k_fft_pass2_real walks,
what the seam buffers must hold), the pyramid levels above the tile (which kernel takes which level from which scratch buffer)
and the waterfall batch (who is sent what, where, and what becomes of the detectors' carry).  Every expectation here is
written from the rules, and the whole output is held against the hash of what the same code printed
while it still sat in forward.hip, between the launches."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import create_plan_table as CT
import forward_plan_table as T
from conftest import ROOT

# ---- segments
GS = (8, 16, 32, 64, 128)          # tiles of a frame: production has 64 and 128, 16 is the smallest that can hand off, 8 never does
CUS = (1, 64, 256, 304)
ENVS = (0, 1, 3, 4, 64, 1000)      # PSDR_SEG_LEN
CAPS = (1, 2, 16, 255, 256, 257, 512, 640)
# the batch sizes whose tables are printed whole: the edges of the rule (one frame per work-group and one more, for every
# num_cus), the seventeen of HANDOFF below, the bench's, the largest
NF_DUMP = tuple(sorted({1, 2, 3, 7, 16, 17, 63, 64, 65, 96, 128, 160, 192, 255, 256, 257, 288, 304, 305, 320, 384, 511, 512, 513, 600, 640, 1024}))
NF_DUMP_ENV = (1, 2, 3, 5, 8, 33, 64)
# (G, nframes) -> hand-off at 256 CUs: the truth table of the plan's rule, by hand
HANDOFF = {(64, 512): True, (128, 512): True, (64, 640): True, (16, 600): True, (64, 513): True, (64, 511): True, (64, 256): False, (64, 1): False,
           (128, 7): False, (64, 320): True, (64, 160): False, (128, 160): False, (64, 128): False, (64, 192): False, (64, 96): False, (64, 384): True,
           (64, 257): True}

# ---- tails: the nine shapes psdr_create accepts that differ here, as it resolves them (createplan.h: test_shapes_are_what_create_plans) -
# name: R, LT, log2M2, real_fused, RecMap mapped / l2gpt / pair, groups per output row when the column tail takes them (else 0)
SHAPES = {
    "iq12": (1 << 12, 4, 6, 0, 1, 2, 0, 0),         # 64 x 64, tiles of 64 rows: four groups per tile
    "iq16": (1 << 16, 4, 8, 0, 1, 2, 0, 0),         # 256 x 256
    "iq20": (1 << 20, 4, 10, 0, 1, 0, 0, 64),       # 1024 x 1024, tiles of 16 rows
    "iq21": (1 << 21, 4, 10, 0, 1, 0, 0, 128),      # 2048 x 1024
    "iq22": (1 << 22, 3, 11, 0, 1, 0, 0, 0),        # 2048 x 2048, tiles of 8 rows: 2048-point rows of an IQ pass have no column tail
    "real13": (1 << 12, 8, 6, 0, 0, 0, 0, 0),       # three-pass: k_untangle_real leaves level-major sums of level 8
    "real20": (1 << 19, 8, 9, 0, 0, 0, 0, 0),       # three-pass (1024 x 512)
    "real21": (1 << 20, 3, 10, 1, 2, 0, 0, 128),    # fused, octets
    "real22": (1 << 21, 2, 11, 1, 2, 0, 1, 256),    # fused, 1024 x 2048: quartets side by side
    "real22-2048x1024": (1 << 21, 3, 10, 1, 2, 0, 0, 256),  # fused, PSDR_REAL_SPLIT=2048x1024: octets
}


# the config each row of SHAPES names: (fft_size, is_real, PSDR_REAL_SPLIT=2048x1024)
SHAPE_CONFIGS = {"iq12": (1 << 12, 0, 0), "iq16": (1 << 16, 0, 0), "iq20": (1 << 20, 0, 0), "iq21": (1 << 21, 0, 0), "iq22": (1 << 22, 0, 0), "real13": (1 << 13, 1, 0),
                 "real20": (1 << 20, 1, 0), "real21": (1 << 21, 1, 0), "real22": (1 << 22, 1, 0), "real22-2048x1024": (1 << 22, 1, 1)}


def test_shapes_are_what_create_plans():
    """the hand table above against shape_plan (createplan.h) for the config each row names: the facts tails_plan is handed at create"""
    assert set(SHAPE_CONFIGS) == set(SHAPES)
    script = "".join("%s\n%s\n" % (CT.env(split=split), CT.cfg(N, r, levels=3)) for N, r, split in SHAPE_CONFIGS.values())
    out = CT.blocks(CT.run(CT.program(), script))
    for (name, (R, LT, l2m2, fused, mapped, l2gpt, pair, ng)), b in zip(SHAPES.items(), out):
        t = b["tail"][0]
        assert tuple(int(t[k]) for k in ("R", "LT", "l2M2", "M2", "fused", "mapped", "l2gpt", "pair")) == (R, LT, l2m2, 1 << l2m2, fused, mapped, l2gpt, pair), name
        assert ((R >> LT) >> l2m2 if ng else 0) == ng, name  # groups per output row, where the column tail takes them


def tail_levels(R, LT):
    return sorted({1, LT + 1, LT + 2, R.bit_length()})  # downsample_levels: nothing above the tile, one level, two, the maximum


# ---- waterfall: a 2^16-point IQ context (levels 0..4 in tiled records of 16 channels) with three slots, the middle one inactive
WF_R, WF_LEVELS, WF_TLT, WF_CH = 1 << 16, 17, 4, 16
SAMPLE, PEAK, MEAN = 0, 1, 2
SKIPS = (1, 3, 6, 700)
BATCHES = (1, 5, 512)
# (level, l, r): below tiled_lt with whole dwords per record, below it without (16 >> 3 = 2 values per record: vec = 0) and with an
# odd window, AT tiled_lt, above it (level-major, whole dwords), and the two top levels of 2 and 1 values (vec = 0)
WINDOWS = {"low": (1, 0, 1024), "low_odd": (3, 3, 1000), "at": (4, 16, 4096), "above": (6, 1, 1023), "top2": (15, 0, 2), "top1": (16, 0, 1)}


def wf_script():
    """[(line, (first, nframes) or None)]: runs of calls that continue, break, lose every detector and regain one, and hold no sent frame
    for several calls - for every skip_num and batch size"""
    out = []
    for skip in SKIPS:
        for nf in BATCHES:
            out.append("wfreset 3")
            out.append("wffacts %d %d %d %d %d" % (WF_R, WF_LEVELS, WF_TLT, WF_CH, skip))

            def slot(i, active, win, det):
                out.append("wfslot %d %d %d %d %d %d" % ((i, active) + WINDOWS[win] + (det,)))
            slot(0, 1, "low", SAMPLE), slot(1, 0, "at", PEAK), slot(2, 1, "above", PEAK)
            first = 0
            for k in range(4):  # a run that continues
                out.append("wfbatch %d %d" % (first, nf))
                first += nf
            slot(0, 1, "low_odd", MEAN), slot(2, 1, "top2", PEAK)
            out.append("wfbatch %d %d" % (first, nf))  # ... with other windows and detectors
            first += nf + 2                            # a gap: the run breaks
            for k in range(3):
                out.append("wfbatch %d %d" % (first, nf))
                first += nf
            slot(0, 1, "at", SAMPLE), slot(2, 1, "top1", SAMPLE)  # every detector gone
            for k in range(2):
                out.append("wfbatch %d %d" % (first, nf))
                first += nf
            slot(2, 1, "above", MEAN)  # one regained: a new run
            for k in range(3):
                out.append("wfbatch %d %d" % (first, nf))
                first += nf
            slot(0, 0, "low", SAMPLE)  # only the detector client left
            out.append("wfbatch %d %d" % (first, nf))
            out.append("wfbatch %d %d" % (first, nf))  # the same frames again: no continuation
            first = 700 * 3 + 1  # right behind a sent frame of every skip_num: calls without a sent frame accumulate
            for k in range(6):
                out.append("wfbatch %d %d" % (first, nf))
                first += nf
            slot(2, 0, "above", MEAN)  # nobody left
            out.append("wfbatch %d %d" % (first, nf))
    return out


def script():
    lines = []
    for G in GS:
        for cus in CUS:
            for env in ENVS:
                lines.append("seg %d %d %d 1 640" % (G, cus, env))
                lines.append("seg %d %d %d 1024 1024" % (G, cus, env))
                lines += ["cap %d %d %d %d" % (G, cus, env, m) for m in CAPS]
    for G in GS:
        for cus in CUS:
            lines += ["segtab %d %d 0 %d" % (G, cus, nf) for nf in NF_DUMP]
        for env in ENVS[1:]:
            lines += ["segtab %d 256 %d %d" % (G, env, nf) for nf in NF_DUMP_ENV]
    for name, (R, LT, l2m2, fused, mapped, l2gpt, pair, _) in SHAPES.items():
        for levels in tail_levels(R, LT):
            lines.append("tails %d %d %d %d %d %d %d %d %d" % (R, levels, LT, l2m2, 1 << l2m2, fused, mapped, l2gpt, pair))
    lines += wf_script()
    # the carry's layout: the shapes' record buffers (q_len with every level, q_stride rounded to 128, two bytes per bin of
    # records), one without tiled records, one whose records are no whole 16-byte pieces
    for R, tlt in ((1 << 12, 4), (1 << 16, 4), (1 << 20, 4), (1 << 22, 3), (1 << 20, 3), (1 << 21, 2), (1 << 19, -1)):
        for levels in (1, max(tlt, 0) + 1, max(tlt, 0) + 2, R.bit_length()):
            q_len = sum(R >> i for i in range(levels))
            lines.append("wflayout %d %d %d %d %d %d" % (tlt, levels, R, q_len, (q_len + 127) & ~127, 2 * R if tlt >= 0 else 0))
    lines.append("wflayout 4 3 1000 1750 1792 2000")
    lines.append("wflayout 4 3 1000 1750 1792 2008")
    lines.append("wflayout 4 3 1000 1750 1744 2000")
    return "\n".join(lines) + "\n"


INPUT = script()


@pytest.fixture(scope="module")
def stdout():
    return T.run(T.program(), INPUT)


@pytest.fixture(scope="module")
def segs(stdout):
    """{(G, cus, env, nf): fields} of the `seg` lines"""
    res = {}
    for ln in stdout.splitlines():
        if ln.startswith("seg "):
            f = {k: (v if k == "fnv" else int(v)) for k, v in T.fields(ln).items()}
            res[(f["G"], f["cus"], f["env"], f["nf"])] = f
    return res


def test_trace_is_what_the_enqueue_path_computed_before_the_planners_moved(stdout):
    """recorded before any code moved: the parent's real_seg_len / seg_plan_lens / seg_plan_counts / seg_plan, the loop of its
    enqueue_tails and the host part of its psdr_waterfall_batch, compiled verbatim in front of a stand-in for the context,
    printed this script (tests/golden/forward_plan_trace.json): a mismatch is a change of behaviour"""
    with open(os.path.join(ROOT, "tests", "golden", "forward_plan_trace.json")) as f:
        golden = json.load(f)
    assert hashlib.sha256(INPUT.encode()).hexdigest() == golden["input_sha256"], "the script changed: the trace was recorded for another"
    assert hashlib.sha256(stdout.encode()).hexdigest() == golden["output_sha256"]


# ---- segments
def test_every_batch_size_gets_a_table_that_keeps_the_invariants(segs):
    """the program checks every table of the grid itself (seg_invariants: the same rules as check_table below, which runs on the
    tables printed whole); here: the grid is complete, and the counts and lengths fit together"""
    assert len(segs) == len(GS) * len(CUS) * len(ENVS) * 641
    for (G, cus, env, nf), f in segs.items():
        assert f["inv"] == 1, f
        ln = f["len"]
        assert 1 <= ln <= G and ln & (ln - 1) == 0
        if env > 0:
            assert not f["handoff"] and ln == min(1 << (env.bit_length() - 1), G) and f["count"] == nf * (G // ln)
        elif f["handoff"]:
            assert f["count"] == nf * (G.bit_length() + 1)  # log2 G + 2 segments a frame
        else:
            assert f["count"] == nf * (G // ln)
        assert f["handoff"] == (env == 0 and G >= 16 and nf > cus)  # more than one frame per work-group
    # PSDR_SEG_LEN set: the number of CUs plays no part
    for G in GS:
        for env in ENVS[1:]:
            for nf in (1, 7, 256, 640, 1024):
                assert len({segs[(G, cus, env, nf)]["fnv"] for cus in CUS}) == 1


def test_hand_off_truth_table(segs):
    for (G, nf), want in HANDOFF.items():
        assert bool(segs[(G, 256, 0, nf)]["handoff"]) == want, (G, nf)
    assert not any(segs[(8, cus, 0, nf)]["handoff"] for cus in CUS for nf in (1, 2, 305, 640, 1024))  # G = 8: G/8 ... has no tile to give


def test_seg_cap_is_the_largest_count(stdout, segs):
    caps = [T.fields(ln) for ln in stdout.splitlines() if ln.startswith("cap ")]
    assert len(caps) == len(GS) * len(CUS) * len(ENVS) * len(CAPS)
    for c in caps:
        G, cus, env, maxb, cap = (int(c[k]) for k in ("G", "cus", "env", "maxb", "cap"))
        counts = [segs[(G, cus, env, nf)]["count"] for nf in range(1, maxb + 1)]
        assert cap == int(c["brute"]) == max(counts) and all(n <= cap for n in counts)


def check_table(G, nframes, tab, handoff):
    """the invariants of tests/test_real_fused_model.py test_segment_plan_partitions_frames_and_orders_the_hand_offs, on arrays"""
    f, g0, ln, above, mem = tab.T
    assert (ln >= 1).all() and (g0 - ln + 1 >= 0).all() and (g0 < G).all() and (f >= 0).all() and (f < nframes).all()
    cover = np.zeros((nframes, G + 1), np.int64)
    np.add.at(cover, (f, g0 - ln + 1), 1)
    np.add.at(cover, (f, g0 + 1), -1)
    assert (np.cumsum(cover, axis=1)[:, :G] == 1).all()  # every tile of every frame in exactly one segment
    nseam = int((mem == 0).sum())
    assert not mem[:nseam].any() and mem[nseam:].all()   # the segments without a carry-in first
    fa, ga, la = tab[above, 0], tab[above, 1], tab[above, 2]
    assert (fa == f).all()
    top = g0 == G - 1
    assert ((ga - la + 1)[top] == 0).all() and not mem[top].any()  # the top segment: row M1/2 from the segment that holds tile 0
    assert ((ga - la + 1)[~top] == g0[~top] + 1).all()             # the segment above ends one tile above this one's first
    sg = np.arange(len(tab))
    assert (above[mem == 1] == sg[mem == 1] - nframes).all()       # the same frame one level up, nframes entries earlier
    if handoff:
        lens = [G // 4] * 3 + [G >> k for k in range(3, G.bit_length())] + [1]
        assert nseam == nframes and ln.max() == G // 4 and ln[-1] == 1
        assert len(tab) == nframes * (4 + int(np.log2(G // 8)) + 1) == nframes * len(lens)
        assert (ln.reshape(len(lens), nframes) == np.array(lens)[:, None]).all() and (f.reshape(len(lens), nframes) == np.arange(nframes)).all()
    else:
        assert nseam == len(tab) and len(set(ln.tolist())) == 1


def test_printed_tables_partition_frames_and_order_the_hand_offs(stdout, segs):
    tabs = T.tables(stdout)
    assert len(tabs) == len(GS) * (len(CUS) * len(NF_DUMP) + (len(ENVS) - 1) * len(NF_DUMP_ENV))
    seen = set()
    for f, tab in tabs:
        G, cus, env, nf, handoff = (int(f[k]) for k in ("G", "cus", "env", "nf", "handoff"))
        check_table(G, nf, tab, bool(handoff))
        s = segs[(G, cus, env, nf)]
        assert (s["handoff"], s["count"]) == (handoff, len(tab)) and (handoff or set(tab[:, 2].tolist()) == {s["len"]})
        seen.add((G, nf, bool(handoff)) if cus == 256 and env == 0 else None)
    assert {(G, nf, h) for (G, nf), h in HANDOFF.items()} <= seen  # the truth table's seventeen among them


# ---- tails
def tail_lines(stdout):
    return [T.fields(ln) for ln in stdout.splitlines() if ln.startswith("tails ")]


def test_tail_steps_produce_every_level_once_from_alternating_buffers(stdout):
    got = tail_lines(stdout)
    want = [(name, levels) for name, v in SHAPES.items() for levels in tail_levels(v[0], v[1])]
    assert len(got) == len(want)
    kinds = {}
    for (name, levels), g in zip(want, got):
        R, LT, l2m2, fused, mapped, l2gpt, pair, ng = SHAPES[name]
        assert (int(g["R"]), int(g["levels"]), int(g["LT"])) == (R, levels, LT)
        steps = [s.split(":") for s in g["steps"].split(",")] if g["steps"] else []
        assert len(steps) == int(g["n"]) <= 4
        produced, buf = [], 0
        for i, (kind, lvl_in, len_in, src, dst, mp) in enumerate(steps):
            lvl_in, len_in, src, dst, mp = int(lvl_in), int(len_in), int(src), int(dst), int(mp)
            assert len_in == R >> lvl_in and lvl_in + 1 < levels and len_in >= 2
            assert (src, dst) == (buf, buf ^ 1)           # buffers alternate, from pass 2's
            buf = dst
            assert mp == int(i == 0 and mapped != 0)      # only the first consumer of pass 2's sums finds them in RecMap order
            span = 7 if kind == "GENERIC" else ng.bit_length() - 1
            assert kind == "GENERIC" or (i == 0 and ng and len_in >> l2m2 == ng)  # the column tail: first, the levels inside a row
            produced += list(range(lvl_in + 1, min(lvl_in + span, levels - 1) + 1))
            kinds.setdefault(name, set()).add(kind)
        assert produced == list(range(LT + 1, levels))    # levels LT + 1 ... levels - 1, each exactly once
    col = {name: sorted(k - {"GENERIC"}) for name, k in kinds.items()}
    assert col == {"iq12": [], "iq16": [], "iq20": ["COL_64"], "iq21": ["COL_128"], "iq22": [], "real13": [], "real20": [], "real21": ["COL_128"],
                   "real22": ["COL_256_PAIRED"], "real22-2048x1024": ["COL_256"]}


# ---- waterfall
def test_waterfall_calls_against_the_rules(stdout):
    calls = [ln for ln in INPUT.splitlines() if ln.split()[0] in ("wfreset", "wffacts", "wfslot", "wfbatch")]
    got = iter([T.fields(ln) for ln in stdout.splitlines() if ln.startswith("wf ")])
    slots, skip = [], 1
    run, nxt, carry = False, 0, 0
    seen = dict(cont=0, broke=0, accumulate=0, dropped=0, novec=0, early=0, gather_only=0, hold_only=0)
    for ln in calls:
        op, *a = ln.split()
        a = [int(v) for v in a]
        if op == "wfreset":
            slots = [dict(active=0, level=0, l=0, r=0, det=SAMPLE) for _ in range(a[0])]
            run, nxt, carry = False, 0, 0
        elif op == "wffacts":
            assert a[:4] == [WF_R, WF_LEVELS, WF_TLT, WF_CH]
            skip = a[4]
        elif op == "wfslot":
            slots[a[0]] = dict(active=a[1], level=a[2], l=a[3], r=a[4], det=a[5])
        else:
            first, nf = a
            g = next(got)
            sent = [f for f in range(nf) if (first + f) % skip == 0]
            assert [int(v) for v in g["sent"].split(",") if v] == sent and int(g["nsent"]) == len(sent)
            total, maxid = 0, -1
            clients, snap = g["clients"].split(","), g["slots"].split(",")
            for i, s in enumerate(slots):
                qoff = sum(WF_R >> t for t in range(s["level"]))
                vec = int((WF_CH >> s["level"]) >= 4) if s["level"] <= WF_TLT else int((WF_R >> s["level"]) % 4 == 0 and qoff % 4 == 0)
                assert [int(v) for v in clients[i].split(":")] == [s["active"], s["level"], s["l"], s["r"], qoff, total, s["det"], vec]
                assert [int(v) for v in snap[i].split(":")] == [total, len(sent) if s["active"] else 0, s["level"], s["l"], s["r"], s["det"]]
                seen["novec"] += int(s["active"] and not vec)
                if s["active"]:
                    total = (total + len(sent) * (s["r"] - s["l"]) + 15) & ~15
                    maxid = i
            hold = any(s["active"] and s["det"] != SAMPLE for s in slots)
            any_sample = any(s["active"] and s["det"] == SAMPLE for s in slots)
            gather = maxid >= 0 and len(sent) > 0 and total > 0
            assert (int(g["total"]), int(g["maxid"]), int(g["gather"]), int(g["hold"]), int(g["any_sample"])) == (total, maxid, int(gather), int(hold), int(any_sample))
            # the carry: frames of the run since its last sent frame
            cont = hold and run and first == nxt
            seen["cont"] += int(cont)
            seen["broke"] += int(hold and run and first != nxt)
            seen["dropped"] += int(run and not hold)
            seen["early"] += int(not gather and not hold)
            seen["gather_only"] += int(gather and not hold)
            seen["hold_only"] += int(hold and not gather)
            if not cont:
                carry = 0
            assert int(g["carry_in"]) == carry
            assert int(g["f0"]) == (sent[-1] + 1 if sent else 0) and int(g["accumulate"]) == int(not sent and carry > 0)
            seen["accumulate"] += int(g["accumulate"])
            if hold:
                carry = (nf - 1 - sent[-1]) if sent else carry + nf
                run, nxt = True, first + nf
            else:
                run, carry = False, 0
            assert (int(g["run"]), int(g["next"]), int(g["carry_n"])) == (int(run), nxt, carry), (ln, g)
    assert next(got, None) is None
    assert all(v > 0 for v in seen.values()), seen


def test_carry_layout(stdout):
    got = [T.fields(ln) for ln in stdout.splitlines() if ln.startswith("wflayout ")]
    args = [[int(v) for v in ln.split()[1:]] for ln in INPUT.splitlines() if ln.startswith("wflayout ")]
    assert len(got) == len(args)
    for (tlt, levels, R, q_len, q_stride, qt_stride), g in zip(args, got):
        q_up = sum(R >> t for t in range(min(tlt + 1, levels)))
        lenA, qB0, lenB = (int(g[k]) for k in ("lenA", "qB0", "lenB"))
        assert lenA == (qt_stride if tlt >= 0 else 0) and qB0 == q_up // 16 * 16
        assert lenB == max((q_len + 15) // 16 * 16 - qB0, 0)  # the levels above the records, widened to whole 16-byte pieces
        assert int(g["ok"]) == int(lenA % 16 == 0 and (q_len + 15) // 16 * 16 <= q_stride)
    assert [int(g["ok"]) for g in got[-3:]] == [1, 0, 0] and all(int(g["ok"]) for g in got[:-3])


def test_sanitizers(tmp_path, stdout):
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    probe = tmp_path / "sanitizer_probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17", *flags, str(probe), "-o", str(tmp_path / "sanitizer_probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime to link against")
    san = T.build(tmp_path, "forward_plan_table_san", flags)
    assert T.run(san, INPUT, timeout=600) == stdout

"""The multi-GPU group's planner (phantomsdr_amd/csrc/groupplan.h) without a GPU and without the library: tests/group_plan_table.cpp
is compiled with the host C++ compiler - the header is plain C++17 - and runs the scripts below.  What it plans: the argument
rules of psdr_group_create, the layout (transport, buffers per rank, bands), a client's rank, and the ordered operations of a step
with their streams and events.  Placement is held against the Python twin (phantomsdr_amd/distributed.py); the layout rules are
written from DESIGN.md section 6 and include/psdr.h; the operation lists from the order group.hip has always issued them in; and
a happens-before checker walks five consecutive steps of every accepted combination up to 16 ranks - the part of the group no
one-GPU box can run."""
import itertools
import re
import subprocess

import numpy as np
import pytest

import group_plan_table as T
from phantomsdr_amd import distributed as D

CLIENTS, RAW, BAND = 0, 1, 2  # PSDR_SHARD_*
F, MB, AFS = 3, 4, 248        # frames of a step, max_batch, audio_fft_size (the halo)
GC_TIMED = 16


def facts(n, shard, force=0, peer=0, serial=0, twice=-1, R=1 << 16, is_real=0, lay=0, mb=MB, hb=None, ss=None, afs=AFS):
    return "facts %d %d %d %d %d %d %d %d %d %d %d %d %d" % (n, shard, force, peer, serial, twice, R, is_real, lay, mb, 2 * R if hb is None else hb,
                                                          R if ss is None else ss, afs)


def run(lines):
    out = T.run(T.program(), "\n".join(lines) + "\n").splitlines()
    assert len(out) == sum(1 for ln in lines if not ln.startswith("facts"))
    return out


def region_stride(n, R=1 << 20, halo=AFS):
    """a banded 2^20-point root: columns of 1024 bins, 1024 / n of them per band and the halo's behind them"""
    return 1024 * (R // 1024 // n + (halo + 1023) // 1024)


# ---- the argument rules ------------------------------------------------------------------------------------------------------
def test_create_argument_rules_in_the_order_they_are_answered():
    INVALID = -1
    cases = [  # (facts, rule, what the message names) - rules: 1 count, 2 sharding, 3 exclusive flags, 4 listed twice, 5 band power of two
        (facts(0, CLIENTS), 1, 0), (facts(17, CLIENTS), 1, 17), (facts(-3, BAND), 1, -3),
        (facts(2, 3), 2, 3), (facts(2, -1), 2, -1), (facts(0, 7), 1, 0),
        (facts(1, CLIENTS, force=1, peer=1), 3, 0), (facts(2, 5, force=1, peer=1), 2, 5),
        (facts(2, CLIENTS, twice=0), 4, 0), (facts(3, RAW, force=1, twice=5), 4, 5), (facts(2, CLIENTS, force=1, peer=1, twice=0), 3, 0),
        (facts(3, BAND), 5, 3), (facts(6, BAND, peer=1, twice=0), 5, 6), (facts(12, BAND), 5, 12), (facts(3, BAND, twice=1), 4, 1),
    ]
    ok = [facts(1, CLIENTS), facts(16, RAW), facts(3, CLIENTS), facts(5, RAW, peer=1, twice=0), facts(8, BAND, peer=1, twice=0), facts(1, BAND, force=1),
          facts(16, BAND), facts(1, BAND, peer=1), facts(4, BAND, serial=1)]
    out = run([ln for c in cases for ln in (c[0], "check")] + [ln for f in ok for ln in (f, "check")])
    for (f, what, arg), ln in zip(cases, out):
        got = T.fields(ln)
        assert (int(got["code"]), int(got["what"]), int(got["arg"])) == (INVALID, what, arg), (f, ln)
    for f, ln in zip(ok, out[len(cases):]):
        assert ln == "check code=0 what=0 arg=0", (f, ln)


# ---- placement against the Python twin ---------------------------------------------------------------------------------------
def test_band_placement_is_band_of():
    lines, want = [], []
    for n in (1, 2, 4, 8, 16):
        for R in (1 << 15, 1 << 16, 1 << 20):
            lines.append(facts(n, BAND, peer=1, R=R))
            rng = np.random.default_rng(n * 131 + R)
            ls = {0, R - 1} | {e + d for e in range(0, R + 1, R // n) for d in (-1, 0, 1)} | {int(v) for v in rng.integers(0, R, 300)}
            for l in sorted(ls):
                lines.append("place %d 0" % l)
                # outside [0, R) the Python function is not defined: the C rule clamps l at 0 and the band at n - 1
                want.append(0 if l < 0 else n - 1 if l >= R else D.band_of(l, R, n))
            for l, band in ((-1, 0), (-R, 0), (-(1 << 31), 0), (R, n - 1), (R + R // n, n - 1), ((1 << 31) - 1, n - 1)):
                lines.append("place %d 5" % l)
                want.append(band)
    assert [int(T.fields(ln)["rank"]) for ln in run(lines)] == want


def test_round_robin_placement_is_assign_clients():
    for shard in (CLIENTS, RAW):
        for n in (1, 2, 3, 5, 8, 16):
            count = 3 * n + 2
            out = run([facts(n, shard, peer=1)] + ["place %d %d" % (1000 * i, i) for i in range(count)])
            got = [[i for i in range(count) if int(T.fields(out[i])["rank"]) == r] for r in range(n)]
            assert got == D.assign_clients(count, n)


def test_packed_band_bounds_are_band_bounds():
    for n in (1, 2, 4, 8, 16):
        for R in (1 << 15, 1 << 16, 1 << 20):
            for halo in (0, 248, 720):
                f = T.fields(run([facts(n, BAND, peer=1, R=R, afs=halo), "layout"])[0])
                first, bins = [int(v) for v in f["first"].split(",")], [int(v) for v in f["bins"].split(",")]
                assert list(zip(first, bins)) == [D.band_bounds(g, R, n, halo) for g in range(n)], (n, R, halo)
                assert int(f["stride"]) == bins[0] and int(f["halo"]) == halo


# ---- every combination group_check accepts -----------------------------------------------------------------------------------
class Combo:
    def __init__(self, n, shard, transport, serial, banded_shape=False, from_ring=False):
        self.n, self.shard, self.transport, self.serial, self.from_ring = n, shard, transport, serial, from_ring
        self.R = 1 << 20 if banded_shape else 1 << 16
        self.lay = 1 if banded_shape else 0
        self.hb, self.ss = 2 * self.R, self.R
        if banded_shape and shard == BAND and n > 1:  # the root of a banded group keeps its frames one region stride apart
            self.ss = region_stride(n)
        # written from the rules (psdr.h), not from the planner's answer
        self.rccl = transport in ("rccl", "forced")
        self.peer = transport == "peer" and n > 1
        self.self_loop = transport == "forced"
        self.banded = shard == BAND and self.lay == 1 and n > 1
        self.overlap = (not serial) and (self.rccl or self.peer) and (shard == CLIENTS or self.banded)
        self.stride = region_stride(n) if self.banded else min((self.R + n - 1) // n + 1 + AFS, self.R)

    def lines(self, steps):
        f = facts(self.n, self.shard, force=int(self.transport == "forced"), peer=int(self.transport == "peer"), serial=int(self.serial), R=self.R,
                  lay=self.lay, hb=self.hb, ss=self.ss, twice=0 if self.transport == "peer" and self.n > 1 else -1)
        return [f, "layout %d" % self.stride if self.banded else "layout"] + ["step %d %d" % (int(self.from_ring), F)] * steps

    def link_bytes(self):
        if not (self.rccl or self.peer):
            return 0
        return {RAW: (F + 1) * self.hb, CLIENTS: F * self.ss * 8, BAND: F * self.stride * 8}[self.shard]

    def __repr__(self):
        return "n=%d shard=%d %s serial=%d R=2^%d ring=%d" % (self.n, self.shard, self.transport, self.serial, self.R.bit_length() - 1, self.from_ring)


def combos(ns=(1, 2, 4, 8, 16)):
    for n, shard, serial in itertools.product(ns, (CLIENTS, RAW, BAND), (False, True)):
        for transport in (("none", "forced", "peer") if n == 1 else ("rccl", "peer")):
            for banded_shape in ((False, True) if shard != RAW else (False,)):
                for from_ring in ((False, True) if shard == RAW else (False,)):
                    yield Combo(n, shard, transport, serial, banded_shape, from_ring)


STEPS = 5


@pytest.fixture(scope="module")
def planned():
    """[(combo, layout fields, [step fields])] of five consecutive steps of every combination"""
    cs = list(combos())
    out = run([ln for c in cs for ln in c.lines(STEPS)])
    return [(c, T.fields(out[i * (STEPS + 1)]), [T.fields(ln) for ln in out[i * (STEPS + 1) + 1:(i + 1) * (STEPS + 1)]]) for i, c in enumerate(cs)]


def test_layout_rules(planned):
    assert len(planned) > 100
    for c, lay, steps in planned:
        flag = lambda k: bool(int(lay[k]))
        assert (flag("comm_on"), flag("peer_copy"), flag("self_loop")) == (c.rccl, c.peer, c.self_loop), c
        assert flag("overlap") == c.overlap and flag("banded") == c.banded, c
        rbuf = [int(v) for v in lay["rbuf"].split(",")]
        want = {RAW: (MB + 1) * c.hb, CLIENTS: 0, BAND: MB * c.stride * 8}[c.shard]
        # raw and band: every rank >= 1 receives into a buffer of its own (clients: into its spectrum buffer); the root only its
        # own band on the self-loop - its raw broadcast is in place
        assert rbuf[1:] == [want] * (c.n - 1), c
        assert rbuf[0] == (want if c.shard == BAND and c.self_loop else 0), c
        packed = c.shard == BAND and not c.banded
        assert lay["sbuf"] == "".join(str(int(packed and (b >= 1 or c.self_loop))) for b in range(c.n)), c
        if c.shard == BAND:
            assert int(lay["stride"]) == c.stride and int(lay["halo"]) == AFS
        for s in steps:
            assert int(s["link_bytes"]) == c.link_bytes(), c
            assert int(s["n"]) < 160
            ops = s["ops"].split(";")
            timed = [op for op in ops if "/" in op and int(op.split("/")[1]) & GC_TIMED]
            assert len(timed) == (1 if c.rccl or c.peer else 0) and int(s["stats"]) == (2 if c.peer else 1 if c.rccl else 0), c
            if not (c.rccl or c.peer):  # one rank, nothing forced: no mode issues an exchange
                assert not [op for op in ops if re.match(r"WAIT|RECORD|GROUP|BCAST|SEND|RECV|PULL|PACK", op)], (c, ops)
                # (raw from the ring still waits for the ring's copies: that is the ingest's order, not an exchange)
                assert ops == ["RING_WAIT(ST0,%d)" % (F + 1)] * c.from_ring + ["TRANSFORM(0)", "DEMOD_OWN(0)", "WATERFALL(0)"], (c, ops)


# ---- the operation lists ------------------------------------------------------------------------------------------------------
def expected_steps(c, steps):
    """the lists of `steps` consecutive steps, in the order the group has always issued them (issue order of group.hip before the
    planner existed); without the commit marks"""
    n, res = c.n, []
    cur, copies, xp = 0, False, [False, False]
    st = lambda r: "ST%d" % r

    def pull(ops, nbytes, closing):
        ops.append("RECORD(EV_X,ST0)")
        for r in range(1, n):
            ops.extend(["WAIT(%s,EV_X)" % st(r), "RECORD(EV_T0[%d],%s)" % (r, st(r)), "PULL(%d,%s,%d)" % (r, st(r), nbytes), "RECORD(EV_T1[%d],%s)" % (r, st(r)),
                        "RECORD(%s,%s)" % (closing % r, st(r))])

    def bracket(ops, inner, s):
        if c.overlap:
            ops.extend(["RECORD(EV_X,ST0)", "WAIT(XS,EV_X)", "RECORD(EV0,XS)", "GROUP_START"] + inner + ["GROUP_END", "RECORD(EV1,XS)", "RECORD(EV_XDONE[%d],XS)" % s])
        else:
            ops.extend(["RECORD(EV0,ST0)", "GROUP_START"] + inner + ["GROUP_END", "RECORD(EV1,ST0)"])

    for _ in range(steps):
        ops = []
        s = cur ^ 1 if c.overlap else cur
        xstream = "XS" if c.overlap else "ST0"
        if c.overlap:
            if xp[s]:
                ops.extend(["WAIT(ST0,EV_XDONE[%d])" % s] if c.rccl else ["WAIT(ST0,EV_PULL[%d][%d])" % (s, r) for r in range(1, n)])
                xp[s] = False
        elif copies:
            ops.extend("WAIT(ST0,EV_RANK[%d])" % r for r in range(1, n))
            copies = False
        if c.shard == RAW:
            nbytes = (F + 1) * c.hb
            if c.from_ring:
                ops.append("RING_WAIT(ST0,%d)" % (F + 1))
            if c.rccl:
                bracket(ops, ["BCAST_RAW(%d,%s,%d)" % (r, st(r), nbytes) for r in range(n)], s)
            elif c.peer:
                pull(ops, nbytes, "EV_RANK[%d]")
                ops.extend("WAIT(ST0,EV_RANK[%d])" % r for r in range(1, n))
            ops.extend("TRANSFORM(%d)" % r for r in range(n))
            ops.extend("DEMOD_OWN(%d)" % r for r in range(n))
        elif c.shard == CLIENTS:
            count = F * c.ss * 2
            ops.append("TRANSFORM(0)")
            if c.rccl:
                bracket(ops, ["BCAST_SPEC(%d,%s,%d)" % (r, xstream if r == 0 else st(r), count) for r in range(n)], s)
            elif c.peer:
                pull(ops, count * 4, "EV_PULL[%d]" % s + "[%d]" if c.overlap else "EV_RANK[%d]")
            ops.append("DEMOD_OWN(0)")
            ops.extend("DEMOD_FROM_SPEC(%d)" % r for r in range(1, n))
        else:
            count = F * c.stride * 2
            ops.append("TRANSFORM(0)")
            if not c.banded:
                ops.extend("PACK(%d)" % b for b in range(1, n))
            if c.self_loop:
                ops.append("PACK(0)")
            if c.rccl:
                bracket(ops, [op for b in range(0 if c.self_loop else 1, n) for op in ("SEND_BAND(%d,%s,%d)" % (b, xstream, count), "RECV_BAND(%d,%s,%d)" % (b, st(b), count))], s)
            elif c.peer:
                pull(ops, count * 4, "EV_PULL[%d]" % s + "[%d]" if c.overlap else "EV_RANK[%d]")
            ops.append("DEMOD_FROM_BAND(0)" if c.self_loop else "DEMOD_OWN(0)")
            ops.extend(("DEMOD_FROM_BAND_REGION(%d)" if c.banded else "DEMOD_FROM_BAND(%d)") % b for b in range(1, n))
        ops.append("WATERFALL(0)")
        if c.overlap:
            xp[s], cur = True, s
        elif c.peer and c.shard != RAW:
            copies = True
        res.append(ops)
    return res


def bare(ops):
    return [op.split("/")[0] for op in ops.split(";")]


def test_operation_lists_of_three_steps():
    cs = [Combo(n, shard, transport, serial, banded_shape=shard == BAND and n > 1 and not serial)
          for shard in (CLIENTS, RAW, BAND) for n, transport in ((1, "forced"), (4, "rccl"), (4, "peer")) for serial in (True, False)]
    cs += [Combo(4, BAND, "rccl", False), Combo(4, BAND, "peer", True, banded_shape=True), Combo(4, RAW, "peer", False, from_ring=True)]
    out = run([ln for c in cs for ln in c.lines(3)])
    for i, c in enumerate(cs):
        got = [bare(T.fields(ln)["ops"]) for ln in out[4 * i + 1:4 * i + 4]]
        assert got == expected_steps(c, 3), c


def test_two_lists_spelled_out():
    """one rank with RCCL forced, spectrum broadcast, overlapped: the third step waits for the first one's exchange; and four ranks,
    packed bands pulled by the peers, serial: the second step waits for the first one's copies"""
    c = Combo(1, CLIENTS, "forced", False)
    out = [T.fields(ln) for ln in run(c.lines(3))[1:]]
    count = F * (1 << 16) * 2
    body = ["TRANSFORM(0)", "RECORD(EV_X,ST0)", "WAIT(XS,EV_X)", "RECORD(EV0,XS)", "GROUP_START", "BCAST_SPEC(0,XS,%d)" % count, "GROUP_END", "RECORD(EV1,XS)"]
    tail = ["DEMOD_OWN(0)", "WATERFALL(0)"]
    assert out[0]["ops"].split(";") == body + ["RECORD(EV_XDONE[1],XS)/24"] + tail and (out[0]["set"], out[0]["after"]) == ("1", "1:0:0:1")
    assert out[1]["ops"].split(";") == body + ["RECORD(EV_XDONE[0],XS)/24"] + tail and (out[1]["set"], out[1]["after"]) == ("0", "0:0:1:1")
    assert out[2]["ops"].split(";") == ["WAIT(ST0,EV_XDONE[1])/4"] + body + ["RECORD(EV_XDONE[1],XS)/24"] + tail and out[2]["after"] == "1:0:1:1"
    c = Combo(4, BAND, "peer", True)
    out = [T.fields(ln) for ln in run(c.lines(2))[1:]]
    nbytes = F * c.stride * 8
    assert c.stride == (1 << 14) + 1 + AFS
    body = ["TRANSFORM(0)", "PACK(1)", "PACK(2)", "PACK(3)", "RECORD(EV_X,ST0)"]
    for r in (1, 2, 3):
        body += ["WAIT(ST%d,EV_X)" % r, "RECORD(EV_T0[%d],ST%d)" % (r, r), "PULL(%d,ST%d,%d)" % (r, r, nbytes), "RECORD(EV_T1[%d],ST%d)" % (r, r),
                 "RECORD(EV_RANK[%d],ST%d)" % (r, r) + ("/18" if r == 3 else "")]
    body += ["DEMOD_OWN(0)", "DEMOD_FROM_BAND(1)", "DEMOD_FROM_BAND(2)", "DEMOD_FROM_BAND(3)", "WATERFALL(0)"]
    assert out[0]["ops"].split(";") == body and out[0]["after"] == "0:1:0:0"
    assert out[1]["ops"].split(";") == ["WAIT(ST0,EV_RANK[1])", "WAIT(ST0,EV_RANK[2])", "WAIT(ST0,EV_RANK[3])/1"] + body and out[1]["after"] == "0:1:0:0"


# ---- ordering, mechanically -----------------------------------------------------------------------------------------------------
OP = re.compile(r"(\w+?)(?:\((.*)\))?$")


class Node:
    def __init__(self, step, text):
        self.step, self.text = step, text
        kind, args = OP.match(text).groups()
        a = args.split(",") if args else []
        self.kind, self.stream, self.event, self.rank, self.band = kind, None, None, None, None
        if kind == "WAIT":
            self.stream, self.event = a
        elif kind == "RECORD":
            self.event, self.stream = a
        elif kind == "RING_WAIT":
            self.stream = a[0]
        elif kind in ("BCAST_RAW", "BCAST_SPEC", "RECV_BAND", "PULL"):
            self.rank, self.stream = int(a[0]), a[1]
        elif kind == "SEND_BAND":
            self.band, self.stream, self.rank = int(a[0]), a[1], 0
        elif kind == "PACK":
            self.band, self.stream, self.rank = int(a[0]), "ST0", 0
        elif not kind.startswith("GROUP"):  # TRANSFORM, DEMOD_*, WATERFALL: on the rank's own stream
            self.rank, self.stream = int(a[0]), "ST" + a[0]


def check_order(c, steps):
    """steps: [[operation text]] of consecutive steps.  Raises AssertionError where the order of section 6 does not follow from
    program order per stream, WAIT behind the latest earlier RECORD of its event, and peer side behind root side of a collective."""
    if c.shard == RAW:  # the raw halves are ready on the root's stream when the step begins (the caller's order, or the ring's events)
        steps = [["SOURCE(0)"] + ops for ops in steps]
    nodes = [Node(k, op) for k, ops in enumerate(steps) for op in ops]
    anc, last_on, last_rec, root_side = [], {}, {}, {}
    for i, v in enumerate(nodes):  # host order is a topological order: every edge points forward
        pred = []
        if v.stream is not None:
            if v.stream in last_on:
                pred.append(last_on[v.stream])
            last_on[v.stream] = i
        if v.kind == "WAIT":
            assert v.event in last_rec, "(d) %s in step %d: no RECORD of its event before it (%r)" % (v.text, v.step, c)
            pred.append(last_rec[v.event])
        if v.kind == "RECORD":
            last_rec[v.event] = i
        if v.kind in ("BCAST_RAW", "BCAST_SPEC") and v.rank == 0 or v.kind == "SEND_BAND":
            root_side[(v.step, v.band)] = i
        if v.kind in ("BCAST_RAW", "BCAST_SPEC") and v.rank > 0 or v.kind == "RECV_BAND":
            pred.append(root_side[(v.step, v.rank if v.kind == "RECV_BAND" else None)])
        m = 0
        for p in pred:
            m |= anc[p] | (1 << p)
        anc.append(m)
    hb = lambda a, b: bool(anc[b] >> a & 1)
    find = lambda step, kind, **kw: [i for i, v in enumerate(nodes) if v.step == step and v.kind == kind and all(getattr(v, k) == w for k, w in kw.items())]
    one = lambda step, kind, **kw: (lambda r: r[0] if len(r) == 1 else pytest.fail("%s of step %d: %d found (%r)" % (kind, step, len(r), c)))(find(step, kind, **kw))
    packed = c.shard == BAND and not c.banded
    alternate = 2 if c.overlap else 1
    for k in range(len(steps)):
        t0 = one(k, "TRANSFORM", rank=0)
        # who reads the root's data of step k: its side of a collective, and the peers' copies
        readers = [i for i, v in enumerate(nodes) if v.step == k and (v.kind in ("BCAST_RAW", "BCAST_SPEC") and v.rank == 0 or v.kind in ("SEND_BAND", "PULL"))]
        if c.rccl or c.peer:
            assert readers, (c, k)
        for i in readers:
            v = nodes[i]
            band = v.band if v.kind == "SEND_BAND" else v.rank
            if c.shard == RAW:  # the caller's halves: the root's transform - and what the caller orders behind it - after every reader
                assert hb(one(k, "SOURCE"), i), "(a) raw: %s of step %d is not behind what the root's stream held at the step's start (%r)" % (v.text, k, c)
                assert hb(i, t0), "(b) raw: %s of step %d is not before the root's transform (%r)" % (v.text, k, c)
                continue
            assert hb(t0, i), "(a) %s of step %d is not behind the root's transform (%r)" % (v.text, k, c)
            if packed:
                assert hb(one(k, "PACK", band=band), i), "(a) %s of step %d is not behind its PACK (%r)" % (v.text, k, c)
                if k + 1 < len(steps):
                    assert hb(i, one(k + 1, "PACK", band=band)), "(b) %s of step %d is not before the next PACK of its buffer (%r)" % (v.text, k, c)
            if k + alternate < len(steps):
                assert hb(i, one(k + alternate, "TRANSFORM", rank=0)), "(b) %s of step %d is not before the transform of step %d (%r)" % (v.text, k, k + alternate, c)
        # who writes into rank r's receive / spectrum buffer, and who reads it there
        for i, v in enumerate(nodes):
            if v.step != k or not (v.kind in ("BCAST_RAW", "BCAST_SPEC") and v.rank > 0 or v.kind in ("RECV_BAND", "PULL")):
                continue
            demod = [j for j, w in enumerate(nodes) if w.step == k and w.kind.startswith("DEMOD") and w.rank == v.rank]
            assert len(demod) == 1, (c, k, v.text)
            use = [one(k, "TRANSFORM", rank=v.rank)] if c.shard == RAW else []  # raw: the rank's transform reads the buffer, then its demodulation
            for j in use + demod:
                assert hb(i, j), "(c) %s of step %d is not before %s (%r)" % (v.text, k, nodes[j].text, c)
                if k + 1 < len(steps):
                    nxt = [x for x, w in enumerate(nodes) if w.step == k + 1 and w.kind == v.kind and w.rank == v.rank]
                    assert len(nxt) == 1 and hb(j, nxt[0]), "(c) %s of step %d is not before the write of step %d (%r)" % (nodes[j].text, k, k + 1, c)
    return len(nodes)


def test_order_of_five_steps_for_every_combination_up_to_16_ranks(planned):
    for c, lay, steps in planned:
        ops = [bare(s["ops"]) for s in steps]
        assert ops == expected_steps(c, STEPS), c
        check_order(c, ops)


@pytest.mark.parametrize("c", [Combo(4, CLIENTS, "peer", False), Combo(4, CLIENTS, "rccl", False), Combo(4, BAND, "peer", True), Combo(4, RAW, "peer", False),
                               Combo(2, BAND, "peer", False, banded_shape=True), Combo(1, CLIENTS, "forced", False)], ids=repr)
def test_the_checker_misses_no_removed_wait(c):
    """on copies of the lists: every WAIT of five steps is load-bearing - without any one of them the checker objects"""
    steps = [bare(T.fields(ln)["ops"]) for ln in run(c.lines(STEPS))[1:]]
    check_order(c, steps)
    waits = [(k, i) for k, ops in enumerate(steps) for i, op in enumerate(ops) if op.startswith("WAIT(")]
    assert len(waits) >= 3
    for k, i in waits:
        cut = [list(ops) for ops in steps]
        del cut[k][i]
        with pytest.raises(AssertionError):
            check_order(c, cut)


# ---- optional sanitiser pass ----------------------------------------------------------------------------------------------------
def test_sanitizers(tmp_path):
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    probe = tmp_path / "sanitizer_probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17", *flags, str(probe), "-o", str(tmp_path / "sanitizer_probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime to link against")
    text = "\n".join(ln for c in combos() for ln in c.lines(STEPS)) + "\n" + "\n".join([facts(16, BAND, peer=1, R=1 << 15), "place -5 0", "place 99999999 0"]) + "\n"
    san = T.build(tmp_path, "group_plan_table_san", flags)
    assert T.run(san, text, timeout=600) == T.run(T.program(), text)

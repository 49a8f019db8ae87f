"""The cases of tests/test_gpu_post_chain_forms.py - one per form the post chain's plan (phantomsdr_amd/csrc/postplan.h
pc_resolve) can take without a tuning knob - shared with the host-side checks of the same cases
(tests/test_post_chain_forms_cover.py: which plan each case resolves to, what the cases cover of a sweep of rates, frame sizes
and slot counts, and whether each case's input drives the chain far enough).

A case is (rate, n, slots, max_batch, batches, AGC option, pcm16, occupied slots, late slot) and the plan it must resolve to,
written out as literals: a change in pc_resolve cannot move a case onto another form unnoticed.  AGC option 2: the form
changes with every batch (PSDR_OPT_POST_CHAIN_AGC set to batch & 1).

Signal: one s16 stream of stationary noise and carriers (helpers.synth_stream) through a 2^12-point IQ context; client k
of a case sits on CENTRES[k], USB / LSB / AM / FM in turn.  Cases of at most 64 slots add their clients to slots 0, 1, 2, ...;
larger ones fill every slot, remove all but `occupied` (the holes are part of the test) and add one client two batches
late into `late`, a high slot, through the holes below it.

Stream length: a client's stream runs at least L + D + 4 h samples past its start (L = rate / 5: the AGC puts out zeros
until its look-ahead is full), over at least three batches, one of them shorter than max_batch, and where h is not whole
16-sample chunks one batch ends inside a chunk.  rules() checks all of that for every case, without a GPU.

Outside the cases: D >= 1024 with 64 lanes (384 kHz and up: the ring of sums no longer fits in LDS and the plan falls back
to MA_POW2).  No shipped configuration has such a rate, and its look-ahead of 76800 samples does not fit a test of a few
seconds."""
import functools
import os
import subprocess
from collections import namedtuple

import numpy as np

from conftest import ROOT
from helpers import quantize_raw, synth_stream

N, LEVELS = 1 << 12, 3
MODES = ("USB", "LSB", "AM", "FM")
CENTRES = tuple(300 + 230 * k for k in range(15))
SEED = 83

Case = namedtuple("Case", "rate n slots max_batch batches agc pcm16 occupied late plan")
ONE, FIVE = "AGC_ONE_KERNEL", "AGC_FIVE"
SMALL = dict(groups=1, lanes=32, rgroups=2, reserve=8, own=1)
FIRST4 = (0, 1, 2, 3)
# slots 0, 31, 32, 63, 64 (the edges of a work-group of 32 and of 64), 127 | 128, the last slot of a middle group | the first
# of the next, one group with a single client (450 / 1100), 1535 | 1536, the last whole group's last slot, the very last slot
OCC600 = (0, 31, 32, 63, 64, 127, 128, 319, 320, 450, 575, 576, 599)
OCC1600 = (0, 31, 32, 63, 64, 127, 128, 831, 832, 1100, 1535, 1536, 1599)
OCC2000 = (0, 31, 32, 63, 64, 127, 128, 1023, 1024, 1100, 1535, 1536, 1983, 1999)
# 600 / 1600 slots: whole waves (lanes 64), work-groups that own their SIMDs / that do not (more of them than CUs left free)
BIG = dict(lanes=64, own=1, reserve=16, agc=FIVE, gain_lds=0)
KiB = 1024


def _case(rate, n, slots, max_batch, batches, agc=1, pcm16=False, occupied=FIRST4, late=None, plan=None):
    return Case(rate, n, slots, max_batch, tuple(batches), agc, pcm16, tuple(occupied), late, plan)


CASES = {
    # ---- k_pc_ma<., true> (MA_POW2), never launched by another GPU test
    # nsub = 1: k_pc_submax is skipped; D % 4 != 0: the scalar gather / output
    "1000-n248": _case(1000, 248, 4, 4, (4, 3, 4, 2), plan=dict(SMALL, D=2, L=200, ma="MA_POW2", agc=FIVE, rows4=0, nsub=1, direct=0)),
    "1500-n248": _case(1500, 248, 4, 4, (4, 3, 4, 2), plan=dict(SMALL, D=4, L=300, ma="MA_POW2", agc=FIVE, rows4=1, nsub=2, direct=0)),
    "3200-n248": _case(3200, 248, 4, 6, (6, 5, 6, 3), plan=dict(SMALL, D=8, L=640, ma="MA_POW2", agc=ONE, rows4=1, direct=0)),
    "3200-n248-agc0": _case(3200, 248, 4, 6, (6, 5, 6, 3), agc=0, plan=dict(SMALL, D=8, L=640, ma="MA_POW2", agc=FIVE, rows4=1)),
    # ---- the division path (MA_DIV) in front of the one-kernel AGC, a DC delay that is not a whole chunk
    "8000-n248": _case(8000, 248, 4, 9, (9, 7, 9, 4), plan=dict(SMALL, D=20, L=1600, ma="MA_DIV", agc=ONE, rows4=1, direct=0)),
    "8000-n248-agc0": _case(8000, 248, 4, 9, (9, 7, 9, 4), agc=0, plan=dict(SMALL, D=20, L=1600, ma="MA_DIV", agc=FIVE, rows4=1)),
    "8000-n248-agc2": _case(8000, 248, 4, 9, (9, 7, 9, 4), agc=2, plan=dict(SMALL, D=20, L=1600, ma="MA_DIV", rows4=1)),
    "8000-n248-pcm16": _case(8000, 248, 4, 9, (9, 7, 9, 4), pcm16=True, plan=dict(SMALL, D=20, L=1600, ma="MA_DIV", agc=ONE, pcm16=1)),
    "8000-n360": _case(8000, 360, 4, 7, (7, 5, 7, 3), plan=dict(SMALL, D=20, L=1600, h=180, ma="MA_DIV", agc=ONE, rows4=1, direct=0)),
    "8000-n360-agc0": _case(8000, 360, 4, 7, (7, 5, 7, 3), agc=0, plan=dict(SMALL, D=20, L=1600, h=180, ma="MA_DIV", agc=FIVE, rows4=1)),
    # ---- the scalar gather / output with h % 4 == 0 (D = 42)
    "16000-n248": _case(16000, 248, 4, 12, (12, 9, 12, 7), plan=dict(SMALL, D=42, L=3200, ma="MA_DIV", agc=FIVE, rows4=0, direct=0)),
    # ---- the smallest frames: one row group, read from the demodulator's rows (a batch of 5 frames is shorter than the DC
    # delay: not direct); h = 16, the smallest the one-kernel AGC accepts
    "12000-n8": _case(12000, 8, 4, 256, (256, 201, 5, 256, 191), plan=dict(SMALL, D=32, L=2400, h=4, ma="MA2", agc=FIVE, rows4=1, direct=1, agc_ok=0)),
    "12000-n32": _case(12000, 32, 4, 64, (64, 50, 64, 45), plan=dict(SMALL, D=32, L=2400, h=16, ma="MA2_CMW", agc=ONE, rows4=1, direct=1)),
    "12000-n32-agc0": _case(12000, 32, 4, 64, (64, 50, 64, 45), agc=0, plan=dict(SMALL, D=32, L=2400, h=16, ma="MA2", agc=FIVE, direct=0)),
    # ---- whole waves: 64 slots per recurrence work-group, clients in the high slots
    "12000-n360-600": _case(12000, 360, 600, 9, (3, 2, 9, 9, 7), occupied=OCC600, late=598,
                            plan=dict(BIG, D=32, L=2400, ma="MA2", direct=1, rgroups=10, ma_lds=0)),
    "3200-n248-600": _case(3200, 248, 600, 6, (3, 2, 6, 6, 5), occupied=OCC600, late=598, plan=dict(BIG, D=8, L=640, ma="MA_POW2", rgroups=10)),
    "8000-n248-600": _case(8000, 248, 600, 9, (4, 3, 9, 9, 7), occupied=OCC600, late=598, plan=dict(BIG, D=20, L=1600, ma="MA_DIV", rgroups=10)),
    # k_pc_mad's ring [D / 16][4][lanes] with 64 lanes; 192000: 128 KiB of dynamic LDS, the largest request the library makes
    "48000-n248-600": _case(48000, 248, 600, 33, (8, 5, 33, 33, 30), occupied=OCC600, late=598,
                            plan=dict(BIG, D=128, L=9600, ma="MAD", rgroups=10, ma_lds=32 * KiB)),
    "192000-n248-600": _case(192000, 248, 600, 128, (20, 10, 128, 128, 100), occupied=OCC600, late=598,
                             plan=dict(BIG, D=512, L=38400, ma="MAD", rgroups=10, ma_lds=128 * KiB)),
    # ---- more recurrence work-groups than CUs left free: waves that share CUs with the passes (k_pc_ma2<false>,
    # k_pc_mad<false>, k_pc_gain<true, false>)
    "12000-n360-2000": _case(12000, 360, 2000, 9, (3, 2, 9, 9, 7), occupied=OCC2000, late=1998,
                             plan=dict(BIG, D=32, L=2400, ma="MA2", direct=1, rgroups=32, reserve=24, own=0, ma_lds=0)),
    "48000-n248-1600": _case(48000, 248, 1600, 33, (8, 5, 33, 33, 30), occupied=OCC1600, late=1598,
                             plan=dict(BIG, D=128, L=9600, ma="MAD", rgroups=25, reserve=24, own=0, ma_lds=32 * KiB)),
}
LATE_BATCH = 2  # the late client joins in front of this batch


def start_frame(case, slot):
    """the first frame of the client in `slot`"""
    return sum(case.batches[:LATE_BATCH]) if slot == case.late else 0


def slots_of(case):
    """every slot that holds a client at some time, ascending - client k of the case sits in slots_of(case)[k]"""
    return tuple(sorted(case.occupied + ((case.late,) if case.late is not None else ())))


def client_spec(case, k):
    """(mode, l, mid, r) of the case's k-th client"""
    mode, m, w = MODES[k % 4], CENTRES[k], min(100, case.n // 2 - 1)
    l, r = (m, m + w) if mode == "USB" else (m - w, m) if mode == "LSB" else (m - w, m + w)
    return mode, l, float(m), r


def agc_option(case, batch):
    return batch & 1 if case.agc == 2 else case.agc


@functools.lru_cache(maxsize=1)
def _stream():
    longest = max(sum(c.batches) for c in CASES.values())
    return quantize_raw(synth_stream((longest + 1) * (N // 2), False, seed=SEED, fft_size=N), "s16", False)


def raw_stream(case):
    """the case's raw s16 samples: nframes + 1 half frames (every case reads the head of one stream)"""
    return _stream()[:(sum(case.batches) + 1) * (N // 2) * 2]


def rules(case):
    """the stream-length rules as a list of the ones the case breaks"""
    h, L, D = case.n // 2, case.rate // 5, case.rate // 750 * 2
    broken = []
    total = sum(case.batches)
    for slot in slots_of(case):
        have = (total - start_frame(case, slot)) * h
        if have < L + D + 4 * h:
            broken.append(f"slot {slot}: a stream of {have} samples, needs {L + D + 4 * h}")
    if len(case.batches) < 3:
        broken.append("fewer than three batches")
    if not any(b < case.max_batch for b in case.batches) or max(case.batches) > case.max_batch:
        broken.append("no batch is shorter than max_batch (or one is longer)")
    if max(case.batches) != case.max_batch:
        broken.append("no batch is max_batch frames long")
    if h % 16 and not any((b * h) % 16 for b in case.batches):
        broken.append("no batch ends inside a 16-sample chunk")
    if case.slots > 64:
        if case.late is None or case.late < case.slots - 64 or case.late in case.occupied:
            broken.append("no late client in a high slot")
        if len(case.batches) <= LATE_BATCH:
            broken.append("the late client never joins")
        groups = [s >> 6 for s in slots_of(case)]
        if not any(groups.count(g) == 1 for g in set(groups)):
            broken.append("no work-group with exactly one client")
        if not {0, 31, 32, 63, 64, case.slots - 1} <= set(case.occupied):
            broken.append("slots 0, 31, 32, 63, 64 and the last one are not all occupied")
        if max(slots_of(case)) >= case.slots:
            broken.append("a slot past the last")
    elif case.occupied != tuple(range(len(case.occupied))) or case.late is not None:
        broken.append("a small case adds its clients to slots 0, 1, 2, ...")
    if len(slots_of(case)) > len(CENTRES):
        broken.append("more clients than centres")
    return broken


def mismatch(case, k, slot, batch, frame, pos, want, got):
    """the first differing sample of a frame, by where it lies in the client's stream: against the 16-sample chunks, the
    blocks of L samples of the look-ahead and the start of the batch - which names the kernel"""
    i = int(np.nonzero(want != got)[0][0])
    t, L = pos + i, case.rate // 5
    return (f"client {k} ({client_spec(case, k)[0]}) slot {slot} batch {batch} frame {frame} sample {i}: want {int(want[i])}, got {int(got[i])} "
            f"({int(np.count_nonzero(want != got))} of {want.size} samples of the frame differ; stream sample {t} of the client = chunk {t // 16} + {t % 16}, "
            f"look-ahead block {t // L} + {t % L}, sample {frame * (case.n // 2) + i} of the batch's stream)")


# ---- the plans, from the library's own pc_resolve (tests/post_plan_table.cpp, built with the host compiler) ----------------
def build_plan_table(directory):
    exe = os.path.join(str(directory), "post_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "phantomsdr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "post_plan_table.cpp"), "-o", exe])
    return exe


def resolve(exe, points):
    """points: [(rate, n, max_batch, slots, AGC option, pcm16)] -> [plan as a dict of strings]"""
    text = "".join("%d %d %d %d 0 %d %d 0\n" % p for p in points)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(points), r.stdout
    return [dict(kv.split("=", 1) for kv in ln.split()) for ln in out]


def case_points(case):
    """the plan table's rows of a case: one per AGC option it runs with"""
    return [(case.rate, case.n, case.max_batch, case.slots, a, int(case.pcm16)) for a in ((0, 1) if case.agc == 2 else (case.agc,))]


def projection(p):
    """a plan projected onto what decides which code runs: {component: value}"""
    ma, agc, own, lanes = p["ma"], p["agc"], p["own"], p["lanes"]
    return {
        "moving averages (kernel, own where it is a template argument, lanes)": (ma, own if ma in ("MA2", "MAD") else "-", lanes),
        "AGC (pipeline, own of k_pc_gain, lanes)": (agc, own if agc == FIVE else "-", lanes),
        "(moving averages, AGC)": (ma, agc),
        "rows4": p["rows4"],
        "nsub == 1": str(int(p["nsub"] == "1")),
        "direct": p["direct"],
        "h < 16": str(int(int(p["h"]) < 16)),
    }

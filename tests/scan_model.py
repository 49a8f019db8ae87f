"""The band scan's rule (include/psdr.h: psdr_scan_set) in numpy integers, written from the header's words - sort for the quartile,
a walk over the hot bins for the runs - and the driver of tests/scan_plan_table.cpp, the host program that runs the kernels' own
steps (phantomsdr_amd/csrc/scanplan.h).  Shared by tests/test_scan_host.py, tests/test_gpu_band_scan.py
and the mask tests (tests/band_scan_masks.py)."""
import os
import struct
import subprocess

import numpy as np

SEG, RANK, CAP = 256, 63, 8192
SIGNAL = np.dtype([("first", np.uint32), ("end", np.uint32), ("peak_bin", np.uint32), ("peak", np.uint32), ("floor", np.uint32)])


# ---- the model --------------------------------------------------------------------------------------------------------------
def trace(s, frames, fresh, a):
    """s: the trace so far (any integer array, or None with fresh), frames: int8 [F][n] -> int64 [n] after the frames"""
    s = None if s is None else np.asarray(s, np.int64).copy()
    for k, q in enumerate(np.asarray(frames, np.int8)):
        u = (q.astype(np.int64) + 128) << 8
        if fresh and k == 0:
            s = u
        else:
            s = s + ((u - s) >> a)  # numpy's >> of a negative int64 is arithmetic: floor
    assert s.min() >= 0 and s.max() <= 255 * 256
    return s


def quartiles(s):
    return np.sort(np.asarray(s, np.int64).reshape(-1, SEG), axis=1)[:, RANK]


def floors(Q):
    G = len(Q)
    return np.array([min(Q[max(g - 1, 0):min(g + 2, G)]) for g in range(G)], np.int64)


def hot_bins(s, F, threshold):
    s = np.asarray(s, np.int64)
    return s >= np.repeat(np.asarray(F, np.int64), SEG) + (threshold << 8)


def runs(s, threshold, gap):
    """-> (F, every run as a SIGNAL array in ascending order of first - NOT truncated)"""
    s = np.asarray(s, np.int64)
    F = floors(quartiles(s))
    idx = np.flatnonzero(hot_bins(s, F, threshold))
    out = []
    if len(idx):
        cut = np.flatnonzero(np.diff(idx) > gap + 1)  # more than `gap` cold bins between two hot ones: two runs
        firsts = np.concatenate(([idx[0]], idx[cut + 1]))
        lasts = np.concatenate((idx[cut], [idx[-1]]))
        for a, b in zip(firsts, lasts):
            pk = a + int(np.argmax(s[a:b + 1]))  # (argmax: the lowest among equals)
            out.append((a, b + 1, pk, s[pk], F[pk >> 8]))
    return F, np.array(out, SIGNAL)


def listed(all_runs, min_width=1, cap=None):
    """what psdr_read_signals delivers of `all_runs`: (the first `cap` of the kept ones that pass, how many passed, total)"""
    kept = all_runs[:CAP]
    ok = kept[(kept["end"].astype(np.int64) - kept["first"]) >= min_width]
    return (ok if cap is None else ok[:cap]), len(ok), len(all_runs)


# ---- the host program -------------------------------------------------------------------------------------------------------
def build_table(tmp, root, extra=(), name="scan_plan_table"):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(root, "phantomsdr_amd", "csrc"),
                           os.path.join(root, "tests", "scan_plan_table.cpp"), "-o", exe])
    return exe


def run(exe, text, timeout=300):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def fields(ln):
    head, _, text = ln.partition(" text=")
    d = dict(kv.split("=", 1) for kv in head.split()[1:])
    if _:
        d["text"] = text
    return d


def table_trace(exe, tmp, s, frames, fresh, a, tag="t"):
    frames = np.ascontiguousarray(frames, np.int8)
    n = frames.shape[1]
    s = np.zeros(n, np.uint16) if s is None else np.ascontiguousarray(s, np.uint16)
    src, dst = str(tmp / f"{tag}.in"), str(tmp / f"{tag}.out")
    with open(src, "wb") as f:
        f.write(struct.pack("=4i", n, len(frames), int(bool(fresh)), a) + s.tobytes() + frames.tobytes())
    run(exe, f"trace {src} {dst}\n")
    out = np.fromfile(dst, np.uint16)
    os.remove(src), os.remove(dst)
    assert len(out) == n
    return out


def table_eval(exe, tmp, s, threshold, gap, min_width=1, cap=CAP, tag="e"):
    """-> dict(Q, F, total, list (the kept runs), passed, out (the filtered, capped ones))"""
    s = np.ascontiguousarray(s, np.uint16)
    n, G = len(s), len(s) // SEG
    src, dst = str(tmp / f"{tag}.in"), str(tmp / f"{tag}.out")
    with open(src, "wb") as f:
        f.write(struct.pack("=5i", n, threshold, gap, min_width, cap) + s.tobytes())
    run(exe, f"eval {src} {dst}\n")
    raw = open(dst, "rb").read()
    os.remove(src), os.remove(dst)
    Q = np.frombuffer(raw, np.uint32, G, 0)
    F = np.frombuffer(raw, np.uint32, G, 4 * G)
    total, kept = (int(v) for v in np.frombuffer(raw, np.uint32, 2, 8 * G))
    at = 8 * G + 8
    lst = np.frombuffer(raw, SIGNAL, kept, at)
    at += kept * SIGNAL.itemsize
    passed = int(np.frombuffer(raw, np.int32, 1, at)[0])
    out = np.frombuffer(raw, SIGNAL, min(passed, cap), at + 4)
    assert at + 4 + len(out) * SIGNAL.itemsize == len(raw)
    return dict(Q=Q, F=F, total=total, list=lst, passed=passed, out=out)

"""The driver of tests/anb_plan_table.cpp's `run` (the host side of the audio blanker, phantomsdr_amd/csrc/anbplan.h) and an
independent float64 model of the rule, written from the words of include/psdr.h with numpy's own sums, convolutions and variance.
Shared by tests/test_anb_host.py and tests/test_gpu_audio_blanker.py: the table program's anb_stream is the expectation of both."""
import os
import struct
import subprocess

import numpy as np

B, P, E, MAXC, D, H = 256, 10, 24, 16, 536, 824
STATE_BYTES = 6624
STATE_DTYPE = np.dtype([("hist", np.float32, (2, H)), ("pos", np.uint64), ("impulses", np.uint64), ("samples", np.uint64), ("cur", np.uint64)])
assert STATE_DTYPE.itemsize == STATE_BYTES
R0_MIN = 1e-20


def build_table(tmp, root, extra=(), name="anb_plan_table"):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(root, "phantomsdr_amd", "csrc"),
                           "-I" + os.path.join(root, "tests"), os.path.join(root, "tests", "anb_plan_table.cpp"), "-o", exe])
    return exe


def run_streams(exe, tmp, jobs, tag="job"):
    """jobs: [(threshold, width, rows f32 [F * h], flags [F], h, frames)] -> [(rows, states [batches], trace)], one process;
    trace: dict(order [blocks], level [blocks], m [blocks][256], centres [..]) over the blocks in the order they became complete"""
    script = []
    for k, (thr, width, rows, flags, h, frames) in enumerate(jobs):
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1)
        flags = np.ascontiguousarray(flags, np.int32)
        assert sum(frames) == len(flags) and len(rows) == len(flags) * h
        with open(str(tmp / f"{tag}{k}.in"), "wb") as f:
            f.write(struct.pack("=3id", h, len(frames), int(width), float(thr)))
            f.write(np.asarray(frames, np.int32).tobytes() + flags.tobytes() + rows.tobytes())
        script.append("run %s %s" % (tmp / f"{tag}{k}.in", tmp / f"{tag}{k}.out"))
    r = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = []
    for k, (thr, width, rows, flags, h, frames) in enumerate(jobs):
        raw = open(str(tmp / f"{tag}{k}.out"), "rb").read()
        n = len(flags) * h
        got = np.frombuffer(raw, np.float32, n)
        states = np.frombuffer(raw, STATE_DTYPE, len(frames), 4 * n)
        at = 4 * n + STATE_BYTES * len(frames)
        nblk, ncen = (int(v) for v in np.frombuffer(raw, np.int64, 2, at))
        at += 16
        order = np.frombuffer(raw, np.int32, nblk, at)
        level = np.frombuffer(raw, np.float32, nblk, at + 4 * nblk)
        m = np.frombuffer(raw, np.float32, nblk * B, at + 8 * nblk).reshape(nblk, B)
        centres = np.frombuffer(raw, np.int64, ncen, at + 8 * nblk + 4 * nblk * B)
        assert at + 8 * nblk + 4 * nblk * B + 8 * ncen == len(raw)
        out.append((got, states, dict(order=order, level=level, m=m, centres=centres)))
        os.remove(str(tmp / f"{tag}{k}.in")), os.remove(str(tmp / f"{tag}{k}.out"))
    return out


def blocks_done(T):
    return 0 if T < B + E else (T - B - E) // B + 1


def levinson64(R):
    a = np.zeros(P + 1)
    a[0] = 1.0
    err, order = R[0], 0
    for i in range(1, P + 1):
        acc = R[i] + float(np.dot(a[1:i], R[i - 1:0:-1]))
        k = -acc / err
        new = err * (1.0 - k * k)
        if not (new > 0.0 and np.isfinite(new)):
            break
        nxt = a.copy()
        nxt[1:i] = a[1:i] + k * a[i - 1:0:-1]
        nxt[i] = k
        a, err, order = nxt, new, i
    return a, order


def model(x, threshold, width):
    """the rule in float64 over the whole stream x (flagged frames already zero): (processed samples [len(x)] - final for the
    samples of every block but the last complete one's successor -, centres, per block the largest distance-from-1 record:
    ratio [blocks][256] = |m| / T, zeros where the block has no detections by R[0])"""
    x = np.asarray(x, np.float64)
    pl = (width - 1) // 2
    nb = blocks_done(len(x))
    xp = np.concatenate([np.zeros(E), x, np.zeros(E)])  # xp[i + E] = x[i]
    y = x.copy()
    centres, ratio, orders = [], np.zeros((nb, B)), []
    for b in range(nb):
        s = b * B
        blk = x[s:s + B]
        with np.errstate(all="ignore"):
            R = np.array([np.dot(blk[:B - i], blk[i:]) for i in range(P + 1)])
        if not np.isfinite(R[0]) or not R[0] > R0_MIN:
            orders.append(-1)
            continue
        a, order = levinson64(R)
        orders.append(order)
        seg = xp[s + E - P:s + E + B + P]           # x[s - P, s + B + P)
        e = np.convolve(seg, a, mode="valid")       # e[n], n in [s, s + B + P)
        m = np.correlate(e, a, mode="valid")        # m[n] = sum a[j] e[n + j], n in [s, s + B)
        T = threshold * np.sqrt(np.var(m))
        ratio[b] = np.abs(m) / T
        n, found = 0, 0
        while n < B and found < MAXC:
            if abs(m[n]) > T:
                c = s + n
                centres.append(c)
                found += 1
                g0 = c - pl
                f = list(xp[g0 + E - P:g0 + E])     # ... f[i - P .. i - 1]
                for i in range(width):
                    f.append(-sum(a[j] * f[-j] for j in range(1, P + 1)))
                bk = list(xp[g0 + width + E:g0 + width + E + P])  # b[i + 1 .. i + P]
                for i in range(width):
                    bk.insert(0, -sum(a[j] * bk[j - 1] for j in range(1, P + 1)))
                for i in range(width):
                    w = i / (width - 1)
                    if g0 + i >= 0:
                        y[g0 + i] = (1 - w) * f[P + i] + w * bk[i]
                n += pl + 1
            else:
                n += 1
    return y, np.array(centres, np.int64), ratio, orders


def delayed(y, n):
    """the stream's output of length n from processed samples y"""
    out = np.zeros(n, y.dtype)
    if n > D:
        out[D:] = y[:n - D]
    return out

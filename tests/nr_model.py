"""The driver of tests/nr_plan_table.cpp's `run` (the host side of the noise reduction, phantomsdr_amd/csrc/nrplan.h) and a float64
restatement of its windowed transform pair, written from the words of include/psdr.h.  Shared by tests/test_nr_host.py and
tests/test_gpu_noise_reduction.py: the table program's nr_stream is the expectation of both."""
import os
import struct
import subprocess

import numpy as np

M, R, BINS, PAD = 256, 128, 129, 132
STATE_BYTES = 3648
STATE_DTYPE = np.dtype([("tail", np.float32, M), ("ola", np.float32, R), ("pend", np.float32, R), ("Ps", np.float32, PAD), ("N", np.float32, PAD),
                        ("G", np.float32, PAD), ("pos", np.uint64), ("pad", np.uint64)])
assert STATE_DTYPE.itemsize == STATE_BYTES


def build_table(tmp, root, extra=(), name="nr_plan_table"):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(root, "phantomsdr_amd", "csrc"),
                           "-I" + os.path.join(root, "tests"), os.path.join(root, "tests", "nr_plan_table.cpp"), "-o", exe])
    return exe


def run_streams(exe, tmp, jobs, tag="job", rate=12000):
    """jobs: [(depth_db, beta, rows f32 [F * h], flags [F], h, frames)] -> [(rows, states [batches], gains [blocks][129])], one process"""
    script = []
    for k, (depth, beta, rows, flags, h, frames) in enumerate(jobs):
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1)
        flags = np.ascontiguousarray(flags, np.int32)
        assert sum(frames) == len(flags) and len(rows) == len(flags) * h
        with open(str(tmp / f"{tag}{k}.in"), "wb") as f:
            f.write(struct.pack("=3i2d", h, len(frames), rate, float(depth), float(beta)))
            f.write(np.asarray(frames, np.int32).tobytes() + flags.tobytes() + rows.tobytes())
        script.append("run %s %s" % (tmp / f"{tag}{k}.in", tmp / f"{tag}{k}.out"))
    r = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = []
    for k, (depth, beta, rows, flags, h, frames) in enumerate(jobs):
        raw = open(str(tmp / f"{tag}{k}.out"), "rb").read()
        n = len(flags) * h
        got = np.frombuffer(raw, np.float32, n)
        states = np.frombuffer(raw, STATE_DTYPE, len(frames), 4 * n)
        gains = np.frombuffer(raw, np.float32, offset=4 * n + STATE_BYTES * len(frames)).reshape(-1, BINS)
        out.append((got, states, gains))
        os.remove(str(tmp / f"{tag}{k}.in")), os.remove(str(tmp / f"{tag}{k}.out"))
    return out


def tables(exe, tmp):
    """(win f32 [256], tw f32 [256][2]) as the device gets them"""
    path = str(tmp / "nr_tables.bin")
    r = subprocess.run([exe], input="tables %s\n" % path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = np.fromfile(path, np.float32)
    os.remove(path)
    assert len(d) == 3 * M
    return d[:M], d[M:].reshape(M, 2)


def restated_unit_gain(x, win, tw):
    """the transform pair with every gain 1, in float64 arithmetic over the plan's f32 tables: x times the window, a 256-point DFT
    whose matrix is built from the twiddle table, the inverse from its conjugate, the window again, overlap-add at hop 128, the
    result delayed by 256 samples.  What it differs from the delayed input by is the rounding of the tables alone."""
    x = np.asarray(x, np.float64)
    w = win.astype(np.float64)
    W = tw[:, 0].astype(np.float64) + 1j * tw[:, 1].astype(np.float64)
    k = np.arange(M)
    F = W[np.outer(k, k) % M]
    nb = (len(x) - M) // R + 1 if len(x) >= M else 0
    y = np.zeros(len(x) + M)
    for b in range(nb):
        X = F @ (x[b * R:b * R + M] * w)
        y[b * R:b * R + M] += (np.conj(F) @ X).real / M * w
    out = np.zeros(len(x))
    out[M:] = y[:len(x) - M]
    return out

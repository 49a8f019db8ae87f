"""The audio filter's model (include/psdr.h: psdr_client_set_audio_filter), written from the header's words, and the driver of
tests/audio_filter_table.cpp's `run`.  Two evaluations of a cascade, both with the coefficients the device holds (each rounded
once to f32):
  truth()       float64, the difference equation itself: y = b0 x + b1 x[-1] + b2 x[-2] - a1 y[-1] - a2 y[-2]
  sequential()  f32, sample by sample in transposed direct form II with the header's fused operations.  numpy has no fma: each
                fmaf(a, b, c) is a * b + c in float64 rounded to f32 - the product of two f32 numbers is exact in float64, so
                the one difference to a true fmaf is a double rounding in rare halfway cases, which an ERROR measurement against
                truth() does not see
Several streams are evaluated at once: x is [streams][samples].  A flagged frame enters as zeros."""
import os
import struct
import subprocess

import numpy as np

CHUNK, LANES = 16, 64
POLE_MAX = 0.9995
DEEMPHASIS, HIGHPASS, LOWPASS, PEAK = 0, 1, 2, 3


def f32_sections(sections):
    return [tuple(float(np.float32(v)) for v in s) for s in sections]


def masked(x, flags, h):
    x = np.array(x, np.float64, ndmin=2)
    if flags is not None:
        x = x * (np.repeat(np.asarray(flags), h) == 0)
    return x


def truth(sections, x, flags=None, h=1):
    y = masked(x, flags, h)
    for b0, b1, b2, a1, a2 in f32_sections(sections):
        x, y = y, np.zeros_like(y)
        x1 = x2 = y1 = y2 = np.zeros(x.shape[0])
        for i in range(x.shape[1]):
            v = b0 * x[:, i] + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
            y[:, i] = v
            x2, x1, y2, y1 = x1, x[:, i], y1, v
    return y


def _fma(a, b, c):
    return (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def sequential(sections, x, flags=None, h=1):
    y = masked(x, flags, h).astype(np.float32)
    for b0, b1, b2, a1, a2 in f32_sections(sections):
        x, y = y, np.zeros_like(y)
        s1 = s2 = np.zeros(x.shape[0], np.float32)
        for i in range(x.shape[1]):
            v = _fma(b0, x[:, i], s1)
            s1 = _fma(b1, x[:, i], _fma(-a1, v, s2))
            s2 = _fma(b2, x[:, i], (np.float32(-a2) * v).astype(np.float32))
            y[:, i] = v
    return y


def response_db(section, f, rate):
    """|H| in dB at f, float64, from the coefficients as given"""
    b0, b1, b2, a1, a2 = section
    z = np.exp(-2j * np.pi * np.asarray(f, np.float64) / rate)
    return 20 * np.log10(np.abs((b0 + b1 * z + b2 * z * z) / (1 + a1 * z + a2 * z * z)))


def state_matrix(section):
    """A of the f32 recurrence's zero-input step, from the rounded coefficients"""
    _, _, _, a1, a2 = f32_sections([section])[0]
    return np.array([[-a1, 1.0], [-a2, 0.0]])


def pole_section(radius, theta, gain=1.0):
    """a resonator with its pole pair at radius * exp(+-j theta)"""
    return (gain, 0.0, 0.0, -2.0 * radius * np.cos(theta), radius * radius)


def batches_of(split, F):
    """the split's batch lengths over and over until F frames are used up (the last one cut)"""
    out, left, k = [], F, 0
    while left > 0:
        out.append(min(split[k % len(split)], left))
        left -= out[-1]
        k += 1
    return out


def build_table(tmp, root, extra=(), name="audio_filter_table"):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(root, "phantomsdr_amd", "csrc"),
                           "-I" + os.path.join(root, "tests"), os.path.join(root, "tests", "audio_filter_table.cpp"), "-o", exe])
    return exe


def write_run(path, sections, rows, flags, h, frames):
    """the `run` operation's input file: rows f32 [F * h] (any bits), flags [F], frames: the batches' lengths"""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1)
    flags = np.ascontiguousarray(flags, np.int32)
    assert sum(frames) == len(flags) and len(rows) == len(flags) * h
    with open(path, "wb") as f:
        f.write(struct.pack("=3i", len(sections), h, len(frames)))
        f.write(np.asarray(frames, np.int32).tobytes())
        f.write(np.asarray(sections, np.float64).tobytes())
        f.write(flags.tobytes())
        f.write(rows.tobytes())


def run_blocked(exe, tmp, jobs, tag="job"):
    """jobs: [(sections, rows, flags, h, frames)] -> [(rows f32 [F * h], states f32 [batches][4])], one process for all"""
    script = []
    for k, (sections, rows, flags, h, frames) in enumerate(jobs):
        write_run(str(tmp / f"{tag}{k}.in"), sections, rows, flags, h, frames)
        script.append("run %s %s" % (tmp / f"{tag}{k}.in", tmp / f"{tag}{k}.out"))
    r = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = []
    for k, (sections, rows, flags, h, frames) in enumerate(jobs):
        d = np.fromfile(str(tmp / f"{tag}{k}.out"), np.float32)
        n = len(flags) * h
        assert len(d) == n + 4 * len(frames)
        out.append((d[:n], d[n:].reshape(len(frames), 4)))
        os.remove(str(tmp / f"{tag}{k}.in")), os.remove(str(tmp / f"{tag}{k}.out"))
    return out

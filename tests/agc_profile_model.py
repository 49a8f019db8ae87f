"""What the AGC profile tests share (include/psdr.h: psdr_client_set_agc_profile): the one GPU configuration and its input, the
chain assembled from the oracle library's own entry points (its DC blocker, orc_agc_create with a profile's numbers, its int16
conversion), and the driver of tests/agc_profile_table.cpp, the host program over phantomsdr_amd/csrc/agcplan.h whose `run` is
the sample-by-sample recurrence - pinned to the oracle bit for bit by tests/test_agc_profile_host.py, so that it can stand in
where the oracle has no counterpart (cap, manual gain, a profile change in mid-stream)."""
import os
import struct
import subprocess

import numpy as np

from oracle import oracle as O

# the one configuration: the smallest IQ context, 12 kHz audio in frames of 180 samples; L = 2400, D = 32
N, LEVELS, AUDIO_N, RATE = 1 << 12, 3, 360, 12000
H, L, D = AUDIO_N // 2, RATE // 5, RATE // 750 * 2
MAX_CLIENTS, SLOTS, FRAMES = 80, (0, 1, 63, 64, 79), 48
REFERENCE = dict(desired=0.2, attack_ms=50.0, release_ms=300.0, max_gain=0.0, manual=0, manual_gain=0.0)


def profile(**kw):
    return dict(REFERENCE, **kw)


def raw_stream(frames=FRAMES, seed=5):
    """s16 IQ noise whose level rises by 20 dB in the middle of the run: the gain first climbs (release), then falls (attack)"""
    rng = np.random.default_rng(seed)
    ns = (frames + 1) * (N // 2)
    x = rng.standard_normal((ns, 2))
    x[: ns // 2] *= 150.0
    x[ns // 2:] *= 1500.0
    return np.clip(np.round(x), -32768, 32767).astype(np.int16).reshape(-1)


def window(k):
    """client k's USB window"""
    m = 300 + 230 * k
    return m, float(m), m + 100


def build_table(tmp, root):
    exe = str(tmp / "agc_profile_table")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "phantomsdr_amd", "csrc"),
                           os.path.join(root, "tests", "agc_profile_table.cpp"), "-o", exe])
    return exe


def script(exe, text, timeout=300):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def fields(ln):
    return dict(kv.split("=", 1) for kv in ln.split()[1:])


def model_runs(exe, tmp, jobs, rate=RATE, look=L, tag="job"):
    """jobs: [(x f32 [T], segments)] with segments [(count, reset, profile dict or None)] -> [(y f32 [T], g f32 [T])]: the AGC's
    output and the gain behind every sample, from an empty window and gain 0; one process for all jobs"""
    lines = []
    for k, (x, segs) in enumerate(jobs):
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        assert sum(s[0] for s in segs) == x.size
        with open(tmp / f"{tag}{k}.in", "wb") as f:
            f.write(struct.pack("=3ifi", rate, look, len(segs), 0.0, 0))
            for count, reset, p in segs:
                q = p or REFERENCE
                f.write(struct.pack("=9d", count, reset, 1 if p else 0, q["desired"], q["attack_ms"], q["release_ms"], q["max_gain"], q["manual"], q["manual_gain"]))
            f.write(x.tobytes())
        lines.append(f"run {tmp / f'{tag}{k}.in'} {tmp / f'{tag}{k}.out'}")
    script(exe, "\n".join(lines) + "\n")
    out = []
    for k, (x, _) in enumerate(jobs):
        r = np.fromfile(tmp / f"{tag}{k}.out", np.float32)
        T = np.asarray(x).size
        assert r.size == 2 * T
        out.append((r[:T].copy(), r[T:].copy()))
    return out


def dc_block(x, delay=D):
    """the oracle's DC blocker over a whole stream, from zero state"""
    Lb = O.lib()
    a = np.ascontiguousarray(x, np.float32).reshape(-1).copy()
    dc = Lb.orc_dc_create(delay)
    Lb.orc_dc_remove(dc, O._p(a), a.size)
    Lb.orc_dc_destroy(dc)
    return a


def to_int16(y):
    """the oracle's int16 conversion (mult 65536 / 4)"""
    y = np.ascontiguousarray(y, np.float32).reshape(-1)
    pcm = np.zeros(y.size, np.int32)
    O.lib().orc_float_to_int16(O._p(y), O._p(pcm), 16384.0, y.size)
    return pcm


def oracle_agc(x, p, rate=RATE):
    """orc_agc_create with the profile's numbers over a whole stream (manual = 0, no cap: what the oracle has)"""
    assert not p["manual"] and p["max_gain"] == 0
    Lb = O.lib()
    a = np.ascontiguousarray(x, np.float32).reshape(-1).copy()
    agc = Lb.orc_agc_create(p["desired"], p["attack_ms"], p["release_ms"], 200.0, float(rate))
    Lb.orc_agc_process(agc, O._p(a), a.size)
    Lb.orc_agc_destroy(agc)
    return a


def oracle_chain(audio, p):
    """audio rows [F][h] -> PCM [F][h] through the oracle's DC blocker, its AGC built with the profile's numbers and its int16
    conversion: a client's whole stream, nothing dropped"""
    audio = np.asarray(audio, np.float32)
    return to_int16(oracle_agc(dc_block(audio), p)).reshape(audio.shape)

"""The tone decoder's models (include/psdr.h: psdr_client_set_tone_decoder), written from the words of the header:
  records()       a numpy restatement in the rule's own f32 arithmetic - every fmaf exactly, by a float64 sum rounded to odd - that
                  gives a stream's per-frame records bit for bit; the gate is tests/squelch_model.py's state machine;
  windows64()     a float64 evaluation with exact phases (no tables, no recurrence, no f32 sum): the truth the level is measured
                  against and the detector the identification test runs;
  build_table(), run_streams()   the driver of tests/tone_plan_table.cpp's `run` (phantomsdr_amd/csrc/toneplan.h on the host).
Shared by tests/test_tone_host.py and tests/test_gpu_tone_decoder.py."""
import os
import struct
import subprocess

import numpy as np

import squelch_model

HZ = [67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0, 127.3, 131.8,
      136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9, 183.5, 186.2, 189.9, 192.8, 196.6, 199.5,
      203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1]
N, B, TAB, REF_RANK = 50, 256, 4096, 12
REC_DTYPE = np.dtype([("tone", np.int32), ("level", np.float32), ("open", np.int32), ("pad", np.int32)])
STATE_DTYPE = np.dtype([("part", np.float32, B), ("pos", np.uint64), ("open", np.int32), ("cnt", np.int32), ("tone_plus1", np.int32),
                        ("level", np.float32)])
assert REC_DTYPE.itemsize == 16 and STATE_DTYPE.itemsize == 1048
DEFAULTS = dict(want=-1, gate=1, snr_db=22.0, min_level=0.0, attack=2, hang=None)  # hang None: NB


def nb_of(rate):
    return int(np.ceil(2.0 * rate / 1280.0))


def increments(rate):
    return np.array([int(np.floor(f / rate * 4294967296.0 + 0.5)) for f in HZ], np.uint64)


def window(rate):
    """(h f32 [NB], lscale f32)"""
    nb = nb_of(rate)
    h = (0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(nb) + 0.5) / nb)).astype(np.float32)
    s = 0.0
    for v in h:
        s += float(v)
    return h, np.float32(4.0 / ((256.0 * s) * (256.0 * s)))


def fma32(a, b, c):
    """fmaf on f32 arrays, exactly: the product of two f32 is exact in float64; the float64 sum is rounded to odd (its error term
    from the two-sum decides), which makes the final rounding to f32 the rounding of the exact value"""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    si = np.ascontiguousarray(s).view(np.int64)
    need = (err != 0) & ((si & 1) == 0)
    si = np.where(need, si + np.where((err > 0) == (s > 0), 1, -1), si)
    return si.view(np.float64).astype(np.float32)


def cmul32(ar, ai, br, bi):
    return fma32(ar, br, -(ai * bi)), fma32(ar, bi, ai * br)


def correlations(x, rate, first_block=0):
    """C f32 [blocks][50] (re, im) of the whole blocks of the stream x (f32), block 0 being stream block `first_block`"""
    x = np.asarray(x, np.float32)
    nblk = len(x) // B
    xb = x[:nblk * B].reshape(nblk, B)
    inc = increments(rate)
    j = np.arange(TAB)
    coarse = (np.cos(2 * np.pi * j / 4096.0).astype(np.float32), np.sin(2 * np.pi * j / 4096.0).astype(np.float32))
    fine = (np.cos(2 * np.pi * j / 16777216.0).astype(np.float32), np.sin(2 * np.pi * j / 16777216.0).astype(np.float32))
    ang = 2 * np.pi * inc.astype(np.float64) / 4294967296.0
    rr, ri = np.cos(ang).astype(np.float32)[None, :], np.sin(ang).astype(np.float32)[None, :]
    t0 = (np.arange(nblk, dtype=np.uint64) + np.uint64(first_block)) * np.uint64(B)
    phase = ((inc[None, :] * (t0[:, None] & np.uint64(0xFFFFFFFF))) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    wr, wi = cmul32(coarse[0][phase >> 20], coarse[1][phase >> 20], fine[0][(phase >> 8) & 4095], fine[1][(phase >> 8) & 4095])
    cr, ci = np.zeros((nblk, N), np.float32), np.zeros((nblk, N), np.float32)
    for n in range(B):
        xn = xb[:, n:n + 1]
        cr = fma32(xn, wr, cr)
        ci = fma32(-xn, wi, ci)
        wr, wi = cmul32(wr, wi, rr, ri)
    return cr, ci


def decisions(cr, ci, rate, want=-1, snr_db=22.0, min_level=0.0):
    """per block b >= NB - 1 of the correlations: (hit, best, level f32, ratio P_best / ref as float64); block NB - 1 first"""
    h, lscale = window(rate)
    nb = len(h)
    nd = len(cr) - nb + 1
    if nd <= 0:
        return np.zeros(0, bool), np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0)
    sr, si = np.zeros((nd, N), np.float32), np.zeros((nd, N), np.float32)
    for j in range(nb):
        sr, si = fma32(h[j], cr[j:j + nd], sr), fma32(h[j], ci[j:j + nd], si)
    P = fma32(sr, sr, si * si)
    u = np.ascontiguousarray(P).view(np.uint32)
    best = np.argmax(u, axis=1)
    ref = np.sort(u, axis=1)[:, REF_RANK].copy().view(np.float32)
    Pb = P[np.arange(nd), best]
    level = (Pb * lscale).astype(np.float32)
    ratio = np.float32(10.0 ** (snr_db / 10.0))
    fin = np.isfinite(P).all(axis=1)
    hit = fin & (Pb >= ratio * ref) & (level >= np.float32(min_level)) & ((want < 0) | (best == want))
    level = np.where(fin, level, np.float32(0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = Pb.astype(np.float64) / ref.astype(np.float64)
    return hit, best, level, q


def records(rows, flags, h, rate, want=-1, gate=1, snr_db=22.0, min_level=0.0, attack=2, hang=None, prev_drop=None):
    """REC_DTYPE [F] (and drop int32 [F] if prev_drop is given) of the stream rows f32 [F][h] from zero state: the model of the rule.
    It sees the whole stream at once - the rule's records do not depend on the batches."""
    rows = np.asarray(rows, np.float32).reshape(len(flags), h).copy()
    rows[np.asarray(flags) != 0] = 0
    F = len(flags)
    nb = nb_of(rate)
    hang = nb if hang is None else hang
    cr, ci = correlations(rows.reshape(-1), rate)
    hit, best, level, _ = decisions(cr, ci, rate, want, snr_db, min_level)
    gates, _ = squelch_model.run(hit.astype(np.float32), 0.5, 0.5, attack, hang)
    rec = np.zeros(F, REC_DTYPE)
    done = ((np.arange(F) + 1) * h) // B  # blocks complete at the frame's last sample
    for f in range(F):
        d = done[f] - nb  # index of the last decision
        if d < 0:
            rec[f] = (-1, 0.0, 0, 0)
        else:
            rec[f] = (best[d] if hit[d] else -1, level[d], gates[d], 0)
    if prev_drop is None:
        return rec
    drop = ((np.asarray(prev_drop) != 0) | ((gate != 0) & (rec["open"] == 0))).astype(np.int32)
    return rec, drop


def windows64(x, rate):
    """x float64 [cases][NB * 256]: one window each, with exact phases in float64.  (best [cases], P_best / ref [cases],
    level [cases]): the detector's decision and the squared amplitude it measures"""
    x = np.asarray(x, np.float64)
    nb = nb_of(rate)
    assert x.shape[1] == nb * B
    hw = np.repeat(window(rate)[0].astype(np.float64), B)
    inc = increments(rate).astype(np.float64)
    t = np.arange(nb * B, dtype=np.float64)
    ph = 2 * np.pi * np.mod(np.outer(t, inc), 4294967296.0) / 4294967296.0  # (products below 2^53: exact)
    E = np.exp(-1j * ph)
    S = (x * hw[None, :]) @ E
    P = np.abs(S) ** 2
    best = np.argmax(P, axis=1)
    Pb = P[np.arange(len(P)), best]
    ref = np.sort(P, axis=1)[:, REF_RANK]
    level = Pb * 4.0 / (256.0 * window(rate)[0].astype(np.float64).sum()) ** 2
    return best, Pb / ref, level


def tone_inputs(rate, seed=20261021, amp=0.1, sigma=0.1, phases=4):
    """the fixed inputs of the identification check: per tone `phases` windows of the tone at amplitude `amp` and a random phase
    in white noise of standard deviation `sigma`: (x float64 [50 * phases][NB * 256], tone number [50 * phases])"""
    rng = np.random.default_rng(seed + rate)
    n = nb_of(rate) * B
    t = np.arange(n)
    x, k = [], []
    for tone, f in enumerate(HZ):
        for _ in range(phases):
            x.append(amp * np.cos(2 * np.pi * f * t / rate + rng.uniform(0, 2 * np.pi)) + sigma * rng.standard_normal(n))
            k.append(tone)
    return np.array(x), np.array(k)


def noise_inputs(rate, windows=300, seed=20261022, sigma=0.1):
    rng = np.random.default_rng(seed + rate)
    return sigma * rng.standard_normal((windows, nb_of(rate) * B))


# ---- the table program ---------------------------------------------------------------------------------------------------------
def build_table(tmp, root, extra=(), name="tone_plan_table"):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(root, "phantomsdr_amd", "csrc"),
                           "-I" + os.path.join(root, "tests"), os.path.join(root, "tests", "tone_plan_table.cpp"), "-o", exe])
    return exe


def run_script(exe, script, timeout=600):
    r = subprocess.run([exe], input=script, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def run_streams(exe, tmp, jobs, tag="job", rate=12000):
    """jobs: [(cfg dict like DEFAULTS, rows f32 [F * h], flags [F], prev_drop [F] or None, h, frames)] ->
    [(rec REC_DTYPE [F], drop int32 [F], states STATE_DTYPE [batches])], one process"""
    script = []
    for k, (cfg, rows, flags, prev, h, frames) in enumerate(jobs):
        c = dict(DEFAULTS, **cfg)
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1)
        flags = np.ascontiguousarray(flags, np.int32)
        prev = np.zeros(len(flags), np.int32) if prev is None else np.ascontiguousarray(prev, np.int32)
        assert sum(frames) == len(flags) and len(rows) == len(flags) * h
        hang = nb_of(rate) if c["hang"] is None else c["hang"]
        with open(str(tmp / f"{tag}{k}.in"), "wb") as f:
            f.write(struct.pack("=7i2d", h, len(frames), rate, c["want"], c["gate"], c["attack"], hang, float(c["snr_db"]), float(c["min_level"])))
            f.write(np.asarray(frames, np.int32).tobytes() + flags.tobytes() + prev.tobytes() + rows.tobytes())
        script.append("run %s %s" % (tmp / f"{tag}{k}.in", tmp / f"{tag}{k}.out"))
    run_script(exe, "\n".join(script) + "\n")
    out = []
    for k, (cfg, rows, flags, prev, h, frames) in enumerate(jobs):
        raw = open(str(tmp / f"{tag}{k}.out"), "rb").read()
        F = len(flags)
        rec = np.frombuffer(raw, REC_DTYPE, F)
        drop = np.frombuffer(raw, np.int32, F, 16 * F)
        states = np.frombuffer(raw, STATE_DTYPE, len(frames), 20 * F)
        out.append((rec, drop, states))
        os.remove(str(tmp / f"{tag}{k}.in")), os.remove(str(tmp / f"{tag}{k}.out"))
    return out


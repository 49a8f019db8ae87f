"""The CW decoder's models (include/psdr.h: psdr_client_set_cw_decoder), written from the words of the header:
  records()       a numpy restatement in the rule's own f32 arithmetic - every fmaf exactly (tests/tone_model.py's fma32) - that
                  gives a stream's per-frame records and its text bit for bit;
  decode64()      the same rule in float64 with exact phases (no tables, no recurrence, no f32): what the noise test measures with;
  keyed_sine()    the sender: standard timing (dit 1, dah 3, gaps 1 / 3 / 7), 2 ms raised edges;
  build_table(), run_streams()   the driver of tests/cw_plan_table.cpp's `run` (phantomsdr_amd/csrc/cwplan.h on the host).
Shared by tests/test_cw_host.py and the GPU tests."""
import os
import struct
import subprocess

import numpy as np

from tone_model import cmul32, fma32

LANES, RING, LO_RANK, TEXT, TAB = 64, 128, 16, 1024, 4096
F0, DF = 250.0, 25.0
REC_DTYPE = np.dtype([("nchars", np.uint32), ("wpm", np.float32), ("pitch_hz", np.float32), ("level", np.float32), ("key", np.int32),
                      ("pad", np.int32)])
STATE_DTYPE = np.dtype([("part", np.float32, 256), ("cprev", np.float32, (64, 2)), ("A", np.float32, 64), ("ring", np.float32, 128),
                        ("pos", np.uint64), ("nchars", np.uint64), ("hi", np.float32), ("lane", np.int32), ("u", np.int32),
                        ("key", np.int32), ("pend", np.int32), ("run", np.int32), ("code", np.int32), ("sp", np.int32)])
assert REC_DTYPE.itemsize == 24 and STATE_DTYPE.itemsize == 2352
DEFAULTS = dict(pitch_hz=700.0, search_hz=100.0, wpm=20.0, track_speed=1, snr_db=22.0)
MORSE = {"A": ".-", "B": "-...", "C": "-.-.", "D": "-..", "E": ".", "F": "..-.", "G": "--.", "H": "....", "I": "..", "J": ".---", "K": "-.-",
         "L": ".-..", "M": "--", "N": "-.", "O": "---", "P": ".--.", "Q": "--.-", "R": ".-.", "S": "...", "T": "-", "U": "..-", "V": "...-",
         "W": ".--", "X": "-..-", "Y": "-.--", "Z": "--..", "1": ".----", "2": "..---", "3": "...--", "4": "....-", "5": ".....", "6": "-....",
         "7": "--...", "8": "---..", "9": "----.", "0": "-----", ".": ".-.-.-", ",": "--..--", ":": "---...", "?": "..--..", "'": ".----.",
         "-": "-....-", "/": "-..-.", "(": "-.--.", ")": "-.--.-", '"': ".-..-.", "=": "-...-", "+": ".-.-.", "@": ".--.-."}


def code_of(key):
    c = 1
    for ch in key:
        c = (c << 1) | (ch == "-")
    return c


BY_CODE = {code_of(k): ch for ch, k in MORSE.items()}


def hop_of(rate):
    return 32 if rate < 8000 else 64 if rate < 16000 else 128 if rate < 32000 else 256


def u_of(wpm, rate):
    return int(np.floor(19.2 * rate / (hop_of(rate) * wpm) + 0.5))


def lane_hz(k):
    return F0 + DF * np.asarray(k, np.float64)


def nearest(pitch):
    return int(min(max(np.floor((pitch - F0) / DF + 0.5), 0), LANES - 1))


def candidates(pitch, search):
    c = np.abs(lane_hz(np.arange(LANES)) - pitch) <= search
    c[nearest(pitch)] = True
    return c


def increments(rate):
    return np.array([int(np.floor(f / rate * 4294967296.0 + 0.5)) for f in lane_hz(np.arange(LANES))], np.uint64)


# ---- the sender ----------------------------------------------------------------------------------------------------------------
def keying(text):
    """the sent text as (on, dots) runs: standard timing"""
    runs = []
    for wi, word in enumerate(text.split(" ")):
        if wi:
            runs.append((0, 7))
        for ci, ch in enumerate(word):
            if ci:
                runs.append((0, 3))
            for ei, el in enumerate(MORSE[ch]):
                if ei:
                    runs.append((0, 1))
                runs.append((1, 3 if el == "-" else 1))
    return runs


def envelope(text, wpm, rate, lead=1.2037, tail=0.6, edge=0.002):
    """float64 [samples]: 0 / 1 keying of `text` at `wpm` behind `lead` seconds of silence, the edges raised cosines of `edge` seconds
    centred on the nominal instants"""
    dot = 1.2 / wpm
    t, parts = lead, [(0.0, 0)]
    for on, dots in keying(text):
        parts.append((t, on))
        t += dots * dot
    parts.append((t, 0))
    n = int(round((t + tail) * rate))
    env = np.zeros(n)
    at = np.array([int(round(p[0] * rate)) for p in parts] + [n])
    for i, (_, on) in enumerate(parts):
        env[at[i]:at[i + 1]] = on
    m = max(int(round(edge * rate)), 1)
    k = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(m) + 0.5) / m)
    return np.convolve(env, k / k.sum(), mode="same")


def keyed_sine(text, wpm, rate, pitch=700.0, amp=0.5, **kw):
    env = envelope(text, wpm, rate, **kw)
    return amp * env * np.sin(2 * np.pi * pitch * np.arange(len(env)) / rate + 0.4)


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def correlations(x, rate):
    """C f32 (re, im) [hops][64] of the whole hops of the stream x (f32) from position 0"""
    H = hop_of(rate)
    x = np.asarray(x, np.float32)
    nh = len(x) // H
    xb = x[:nh * H].reshape(nh, H)
    inc = increments(rate)
    j = np.arange(TAB)
    coarse = (np.cos(2 * np.pi * j / 4096.0).astype(np.float32), np.sin(2 * np.pi * j / 4096.0).astype(np.float32))
    fine = (np.cos(2 * np.pi * j / 16777216.0).astype(np.float32), np.sin(2 * np.pi * j / 16777216.0).astype(np.float32))
    ang = 2 * np.pi * inc.astype(np.float64) / 4294967296.0
    rr, ri = np.cos(ang).astype(np.float32)[None, :], np.sin(ang).astype(np.float32)[None, :]
    t0 = np.arange(nh, dtype=np.uint64) * np.uint64(H)
    phase = ((inc[None, :] * (t0[:, None] & np.uint64(0xFFFFFFFF))) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    wr, wi = cmul32(coarse[0][phase >> 20], coarse[1][phase >> 20], fine[0][(phase >> 8) & 4095], fine[1][(phase >> 8) & 4095])
    cr, ci = np.zeros((nh, LANES), np.float32), np.zeros((nh, LANES), np.float32)
    for n in range(H):
        xn = xb[:, n:n + 1]
        cr = fma32(xn, wr, cr)
        ci = fma32(-xn, wi, ci)
        wr, wi = cmul32(wr, wi, rr, ri)
    return cr, ci


def energies(cr, ci):
    """E f32 [hops][64] = |C[b] + C[b - 1]|^2, not finite -> 0"""
    pr, pi = np.vstack([np.zeros((1, LANES), np.float32), cr[:-1]]), np.vstack([np.zeros((1, LANES), np.float32), ci[:-1]])
    sr, si = (cr + pr).astype(np.float32), (ci + pi).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        E = fma32(sr, sr, (si * si).astype(np.float32))
    return np.where(np.isfinite(E), E, np.float32(0)).astype(np.float32)


def energies64(x, rate):
    """E float64 [hops][64] with exact phases"""
    H = hop_of(rate)
    x = np.asarray(x, np.float64)
    nh = len(x) // H
    t = np.arange(nh * H, dtype=np.float64)
    C = np.empty((nh, LANES), complex)
    for k, inc in enumerate(increments(rate).astype(np.float64)):
        ph = 2 * np.pi * np.mod(t * inc, 4294967296.0) / 4294967296.0
        C[:, k] = (x[:nh * H] * np.exp(-1j * ph)).reshape(nh, H).sum(axis=1)
    S = C + np.vstack([np.zeros((1, LANES)), C[:-1]])
    return np.abs(S) ** 2


class Key:
    """the keying and timing state machine, integers"""

    def __init__(self, u, track, umin, umax):
        self.u, self.track, self.umin, self.umax = u, track, umin, umax
        self.key = self.pend = self.run = self.code = self.sp = 0

    def step(self, raw):
        out = ""
        if self.run < (1 << 26):
            self.run += 1
        if raw != self.key:
            self.pend += 1
            if self.pend >= max(1, self.u // 64):
                if self.key:
                    self.mark_end(self.run - self.pend)
                self.key, self.run, self.pend = raw, self.pend, 0
        else:
            self.pend = 0
        if not self.key:
            len16 = (self.run - self.pend) * 16
            if self.code and len16 >= 2 * self.u:
                out += "*" if self.code >= 256 else BY_CODE.get(self.code, "*")
                self.code, self.sp = 0, 1
            if self.sp and len16 >= 5 * self.u:
                out += " "
                self.sp = 0
        return out

    def mark_end(self, ln):
        dah = int(ln * 16 >= 2 * self.u)
        if self.code == 0:
            self.code = 1
        self.code = 256 if self.code >= 128 else (self.code << 1) | dah
        if self.track:
            target = (16 * ln) // 3 if dah else 16 * ln
            self.u = min(max(self.u + ((target - self.u) >> 2), self.umin), self.umax)  # (>> on a Python int: floor)


def sequence(E, rate, f32, pitch_hz=700.0, search_hz=100.0, wpm=20.0, track_speed=1, snr_db=22.0):
    """the order-dependent part over the hops' energies E [hops][64]: per hop (nchars, u, lane, hi, key), and the text.  f32: the
    rule's own arithmetic; else float64"""
    ft = np.float32 if f32 else np.float64
    nh = len(E)
    cand = candidates(pitch_hz, search_hz)
    lane = nearest(pitch_hz)
    ratio = ft(np.float32(10.0 ** (snr_db / 10.0)))
    key = Key(u_of(wpm, rate), track_speed, u_of(40.0, rate), u_of(10.0, rate))
    # the followers do not depend on a decision: all hops, lane-parallel
    A = np.zeros((nh, LANES), ft)
    a = np.zeros(LANES, ft)
    for b in range(nh):
        a = fma32((E[b] - a).astype(np.float32), np.float32(0.015625), a) if f32 else a + (E[b] - a) / 64
        A[b] = a
    hi = ft(0)
    ring = np.zeros(RING, ft)
    text, trace = "", []
    for b in range(nh):
        ab = np.where(cand, A[b], ft(-1))
        q = int(np.argmax(ab))  # (the first of the largest)
        if A[b][q] > ft(2) * A[b][lane]:
            lane = q
        e = E[b][lane]
        d = np.float32(fma32(hi, np.float32(-0.0078125), hi).reshape(-1)[0]) if f32 else hi - hi / 128
        hi = e if e > d else d
        ring[b % RING] = e
        full = b + 1 >= RING
        lo = np.sort(ring)[LO_RANK] if full else ft(0)  # (energies are >= +0: the order of the values is the bit patterns')
        present = full and np.isfinite(hi) and hi > 0 and hi >= ft(ratio * lo)
        raw = int(present and e >= ft(ft(0.25) * hi))
        text += key.step(raw)
        trace.append((len(text), key.u, lane, hi, key.key))
    return trace, text


def wpm_of(u, rate):
    return np.float32(19.2 * rate / (float(hop_of(rate)) * u))


def records(rows, flags, h, rate, **cfg):
    """(REC_DTYPE [F], text) of the stream rows f32 [F][h] from zero state: the model of the rule.  It sees the whole stream at once -
    the rule's records do not depend on the batches."""
    flags = np.asarray(flags)
    rows = np.asarray(rows, np.float32).reshape(len(flags), h).copy()
    rows[flags != 0] = 0
    F, H = len(flags), hop_of(rate)
    cr, ci = correlations(rows.reshape(-1), rate)
    trace, text = sequence(energies(cr, ci), rate, True, **cfg)
    lscale = np.float32(1.0 / (float(H) * H))
    rec = np.zeros(F, REC_DTYPE)
    done = ((np.arange(F) + 1) * h) // H
    start = np.float32(lane_hz(nearest(cfg.get("pitch_hz", 700.0))))
    for f in range(F):
        if done[f] == 0:
            rec[f] = (0, 0.0, start, 0.0, 0, 0)
        else:
            n, u, lane, hi, key = trace[done[f] - 1]
            rec[f] = (n & 0xFFFFFFFF, wpm_of(u, rate), np.float32(lane_hz(lane)), np.float32(hi) * lscale, key, 0)
    return rec, text


def decode64(x, rate, **cfg):
    """(trace, text) of the stream x in float64"""
    return sequence(energies64(x, rate), rate, False, **cfg)


# ---- the table program ---------------------------------------------------------------------------------------------------------
def build_table(tmp, root, extra=(), name="cw_plan_table"):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(root, "phantomsdr_amd", "csrc"),
                           "-I" + os.path.join(root, "tests"), os.path.join(root, "tests", "cw_plan_table.cpp"), "-o", exe])
    return exe


def run_script(exe, script, timeout=600):
    r = subprocess.run([exe], input=script, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def text_of(ring, total):
    """the last min(total, 1024) characters of a slot's ring"""
    ring = bytes(ring)
    return "".join(chr(ring[i % TEXT]) for i in range(max(0, total - TEXT), total))


def run_streams(exe, tmp, jobs, tag="job", rate=12000):
    """jobs: [(cfg dict like DEFAULTS, rows f32 [F * h], flags [F], h, frames)] ->
    [(rec REC_DTYPE [F], states STATE_DTYPE [batches], text)], one process"""
    script = []
    for k, (cfg, rows, flags, h, frames) in enumerate(jobs):
        c = dict(DEFAULTS, **cfg)
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1)
        flags = np.ascontiguousarray(flags, np.int32)
        assert sum(frames) == len(flags) and len(rows) == len(flags) * h
        with open(str(tmp / f"{tag}{k}.in"), "wb") as f:
            f.write(struct.pack("=4i4d", h, len(frames), rate, c["track_speed"], c["pitch_hz"], c["search_hz"], c["wpm"], c["snr_db"]))
            f.write(np.asarray(frames, np.int32).tobytes() + flags.tobytes() + rows.tobytes())
        script.append("run %s %s" % (tmp / f"{tag}{k}.in", tmp / f"{tag}{k}.out"))
    run_script(exe, "\n".join(script) + "\n")
    out = []
    for k, (cfg, rows, flags, h, frames) in enumerate(jobs):
        raw = open(str(tmp / f"{tag}{k}.out"), "rb").read()
        F = len(flags)
        rec = np.frombuffer(raw, REC_DTYPE, F)
        states = np.frombuffer(raw, STATE_DTYPE, len(frames), 24 * F)
        ring = raw[24 * F + 2352 * len(frames):]
        assert len(ring) == TEXT
        out.append((rec, states, text_of(ring, int(states[-1]["nchars"]))))
        os.remove(str(tmp / f"{tag}{k}.in")), os.remove(str(tmp / f"{tag}{k}.out"))
    return out

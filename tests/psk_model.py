"""The PSK31 decoder's models (include/psdr.h: psdr_client_set_psk_decoder), written from the words of the header:
  records()       a numpy restatement in the rule's own f32 arithmetic - every fmaf exactly (tests/tone_model.py's fma32) - that
                  gives a stream's per-frame records and its text bit for bit;
  varicode(), bpsk()   the sender: BPSK with symbols +-1 under the pulse (1 + cos(pi t / T)) / 2 over |t| < T, an idle preamble of
                  reversals, the characters with 00 between them, a steady-carrier postamble;
  table()         G3PLX's varicode by character, read from the dump of tests/psk_plan_table.cpp (phantomsdr_amd/csrc/pskplan.h
                  holds the one copy there is);
  build_table(), run_streams()   the driver of tests/psk_plan_table.cpp's `run`.
Shared by tests/test_psk_host.py and the GPU tests."""
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np

from tone_model import cmul32, fma32

LANES, P0, WMAX, BINS, FILL, TEXT, TAB, SR_BITS = 16, 8, 32, 16, 32, 1024, 4096, 12
REC_DTYPE = np.dtype([("nchars", np.uint32), ("errors", np.uint32), ("offset_hz", np.float32), ("level", np.float32), ("quality", np.float32),
                      ("present", np.int32)])
STATE_DTYPE = np.dtype([("part", np.float32, 64), ("ring", np.float32, (32, 16, 2)), ("prev", np.float32, (16, 2)), ("Qre", np.float32, 16),
                        ("G", np.float32, 16), ("pos", np.uint64), ("nchars", np.uint64), ("quality", np.float32),
                        ("level", np.float32), ("errors", np.uint32), ("sr", np.uint32), ("p", np.int32), ("present", np.int32), ("c", np.int32),
                        ("age", np.int32), ("nsp", np.int32), ("pad", np.int32)])
assert REC_DTYPE.itemsize == 24 and STATE_DTYPE.itemsize == 4664
QUALITY_DEFAULT = 0.51  # PSDR_PSK_QUALITY_DEFAULT
DEFAULTS = dict(carrier_hz=1000.0, baud=31.25, search_hz=None, quality=QUALITY_DEFAULT)  # search_hz None: 3 baud / 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hop_of(rate):
    return 8 if rate < 8000 else 16 if rate < 16000 else 32 if rate < 32000 else 64


def wn_of(baud, rate):
    return int(np.floor(rate / (baud * hop_of(rate)) + 0.5))


def u_of(baud, rate):
    return int(np.floor(16.0 * rate / (baud * hop_of(rate)) + 0.5))


def lane_hz(baud):
    """f64 [16]: lane j's offset from the carrier"""
    return (np.arange(LANES, dtype=np.float64) - P0) * baud / 8.0


def candidates(search_hz, baud):
    c = np.abs(lane_hz(baud)) <= search_hz
    c[P0] = True
    return c


def increments(rate, carrier_hz, baud):
    return np.array([int(np.floor(f / rate * 4294967296.0 + 0.5)) for f in carrier_hz + lane_hz(baud)], np.uint64)


def config(**cfg):
    c = dict(DEFAULTS)
    c.update(cfg)
    if c["search_hz"] is None:
        c["search_hz"] = 3.0 * c["baud"] / 8.0
    return c


# ---- the table program ---------------------------------------------------------------------------------------------------------
def build_table(tmp, root=ROOT, extra=(), name="psk_plan_table"):
    exe = os.path.join(str(tmp), name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(root, "phantomsdr_amd", "csrc"),
                           "-I" + os.path.join(root, "tests"), os.path.join(root, "tests", "psk_plan_table.cpp"), "-o", exe])
    return exe


def run_script(exe, script, timeout=600):
    r = subprocess.run([exe], input=script, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def parse_tables(line):
    d = dict(kv.split("=", 1) for kv in line.split()[1:])
    d["varicode"] = [int(v, 16) for v in d["varicode"].split(",")]
    return d


@functools.lru_cache(maxsize=None)
def table():
    """the varicode by character, [128] of int: the code's bits, the first one sent on top.  Read from the table program's dump -
    the program is built for it where nobody has (the GPU tests)"""
    with tempfile.TemporaryDirectory() as tmp:
        t = parse_tables(run_script(build_table(tmp), "tables 12000\n").splitlines()[0])["varicode"]
    assert len(t) == 128
    return tuple(t)


# ---- the sender ----------------------------------------------------------------------------------------------------------------
def varicode(text, preamble=48, postamble=32):
    """the bits of `text` as sent: `preamble` zeros (reversals), per character its code and 00, `postamble` ones (carrier)"""
    t = table()
    bits = [0] * preamble
    for ch in text:
        bits += [int(b) for b in bin(t[ord(ch)])[2:]] + [0, 0]
    return bits + [1] * postamble


def envelope(bits, baud, rate):
    """float64 [samples]: the bits - a 0 turns the symbol over - as symbols +-1 under the pulse (1 + cos(pi t / T)) / 2 over |t| < T,
    one symbol every T = 1 / baud, ramping up into the first symbol and down behind the last"""
    s = np.concatenate([[0.0], np.cumprod(np.where(np.asarray(bits) != 0, 1.0, -1.0)), [0.0]])
    u = np.arange(int(np.floor((len(s) - 1) * rate / baud)), dtype=np.float64) * baud / rate
    k = np.floor(u).astype(np.int64)
    w = 0.5 - 0.5 * np.cos(np.pi * (u - k))  # the next symbol's pulse; this one's is 1 - w
    return s[k] * (1.0 - w) + s[k + 1] * w


def bpsk(bits, baud, rate, carrier=1000.0, amp=0.5, lead=0.0, tail=0.0, phase=0.4):
    """float64 [samples]: `lead` seconds of nothing, envelope(bits) on a carrier, `tail` seconds of nothing"""
    env = envelope(bits, baud, rate)
    n0 = int(round(lead * rate))
    t = (np.arange(len(env)) + n0) / rate
    x = amp * env * np.cos(2 * np.pi * carrier * t + phase)
    return np.concatenate([np.zeros(n0), x, np.zeros(int(round(tail * rate)))])


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def correlations(x, rate, carrier_hz, baud):
    """C f32 (re, im) [hops][16] of the whole hops of the stream x (f32) from position 0"""
    H = hop_of(rate)
    x = np.asarray(x, np.float32)
    nh = len(x) // H
    xb = x[:nh * H].reshape(nh, H)
    inc = increments(rate, carrier_hz, baud)
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


def windows(cr, ci, wn):
    """S f32 (re, im) [hops][16] = the sum of the last wn hops' C, oldest first (hops before the start count as 0)"""
    nh = len(cr)
    pr, pi = np.vstack([np.zeros((wn - 1, LANES), np.float32), cr]), np.vstack([np.zeros((wn - 1, LANES), np.float32), ci])
    sr, si = np.zeros((nh, LANES), np.float32), np.zeros((nh, LANES), np.float32)
    for j in range(wn):
        sr, si = (sr + pr[j:j + nh]).astype(np.float32), (si + pi[j:j + nh]).astype(np.float32)
    return sr, si


def clean(v):
    return np.where(np.isfinite(v), v, np.float32(0)).astype(np.float32)


class Varicode:
    """the shift register: a character ends at 00; more than 12 bits without 00 is an error unless they are ones only"""

    def __init__(self):
        self.by_code = {code: ch for ch, code in enumerate(table())}
        self.sr = self.errors = 0

    def step(self, bit):
        self.sr = self.sr << 1 | bit
        if self.sr & 3 == 0:
            code, self.sr = self.sr >> 2, 0
            if code == 0:
                return ""
            if code not in self.by_code:
                self.errors += 1
                return ""
            return chr(self.by_code[code]) if self.by_code[code] else ""
        if self.sr >> SR_BITS:
            self.errors += self.sr != (1 << (SR_BITS + 1)) - 1
            self.sr = 0
        return ""


def sequence(sr, si, rate, lscale, baud=31.25, search_hz=None, quality=QUALITY_DEFAULT, **_):
    """the order-dependent part over the hops' window sums S f32 [hops][16]: per hop (nchars, errors, p, level, coherence, present),
    and the text"""
    nh, u = len(sr), u_of(baud, rate)
    cand = candidates(search_hz, baud)
    k32, quality = np.float32(0.03125), np.float32(quality)
    E = clean(fma32(sr, sr, (si * si).astype(np.float32)))
    G, Q = np.zeros(BINS, np.float32), np.zeros(LANES, np.float32)
    pr, pi = np.zeros(LANES, np.float32), np.zeros(LANES, np.float32)
    vc = Varicode()
    p, c, age, nsp, present = P0, 0, 0, 0, 0
    coh = lev = np.float32(0)
    text, trace = "", []
    for b in range(nh):
        c = (c + 16) % u
        i = 16 * c // u
        tot = np.float32(0)
        for j in np.flatnonzero(cand):
            tot = np.float32(tot + E[b][j])
        G[i] = fma32(tot - G[i], k32, G[i]).reshape(())
        g = int(np.argmax(G.view(np.uint32)))  # (the first of the largest)
        age = min(age + 16, 65536)
        if (c - g * u // 16) % u < u // 2 and age >= 3 * u // 4:
            age = 0
            ar, ai = sr[b], si[b]
            dre = fma32(ar, pr, (ai * pi).astype(np.float32))
            dim = fma32(ai, pr, -(ar * pi).astype(np.float32))
            pr, pi = ar.copy(), ai.copy()
            q = clean(fma32(dre, dre, -(dim * dim).astype(np.float32)))
            w = clean(fma32(dre, dre, (dim * dim).astype(np.float32)))
            Q = fma32((q - Q).astype(np.float32), k32, Q)
            M = np.where(Q > 0, Q, np.float32(0)).astype(np.float32)
            best = int(np.argmax(np.where(cand, M.view(np.uint32).astype(np.int64), -1)))
            if M[best] > np.float32(2) * M[p] and best != p:
                p, vc.sr = best, 0
            nsp = min(nsp + 1, FILL)
            lev = fma32(E[b][p] - lev, k32, lev).reshape(())
            one = np.float32(q[p]) / np.float32(w[p]) if w[p] != 0 else np.float32(0)
            one = one if np.isfinite(one) else np.float32(0)
            coh = fma32(one - coh, k32, coh).reshape(())
            present = int(nsp >= FILL and coh >= quality)
            if present:
                text += vc.step(int(dre[p] >= 0))
            else:
                vc.sr = 0
        trace.append((len(text), vc.errors, p, np.float32(lev * lscale), coh, present))
    return trace, text


def records(rows, flags, h, rate, **cfg):
    """(REC_DTYPE [F], text) of the stream rows f32 [F][h] from zero state: the model of the rule.  It sees the whole stream at once -
    the rule's records do not depend on the batches.  cfg: fields of DEFAULTS"""
    c = config(**cfg)
    flags = np.asarray(flags)
    rows = np.asarray(rows, np.float32).reshape(len(flags), h).copy()
    rows[flags != 0] = 0
    F, H, wn = len(flags), hop_of(rate), wn_of(c["baud"], rate)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        cr, ci = correlations(rows.reshape(-1), rate, c["carrier_hz"], c["baud"])
        sr, si = windows(cr, ci, wn)
        lscale = np.float32(4.0 / (float(wn * H) * float(wn * H)))
        trace, text = sequence(sr, si, rate, lscale, **c)
        rec = np.zeros(F, REC_DTYPE)
        done = ((np.arange(F) + 1) * h) // H
        df = np.float32(c["baud"] / 8.0)
        for f in range(F):
            if done[f]:
                n, errs, p, level, coh, present = trace[done[f] - 1]
                rec[f] = (n & 0xFFFFFFFF, errs & 0xFFFFFFFF, np.float32(p - P0) * df, level, coh, present)
    return rec, text


# ---- the streams ----------------------------------------------------------------------------------------------------------------
def text_of(ring, total):
    """the last min(total, 1024) characters of a slot's ring"""
    ring = bytes(ring)
    return "".join(chr(ring[i % TEXT]) for i in range(max(0, total - TEXT), total))


def run_streams(exe, tmp, jobs, tag="job", rate=12000):
    """jobs: [(cfg dict like DEFAULTS, rows f32 [F * h], flags [F], h, frames)] ->
    [(rec REC_DTYPE [F], states STATE_DTYPE [batches], text)], one process"""
    script = []
    for k, (cfg, rows, flags, h, frames) in enumerate(jobs):
        c = config(**cfg)
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1)
        flags = np.ascontiguousarray(flags, np.int32)
        assert sum(frames) == len(flags) and len(rows) == len(flags) * h
        with open(str(tmp / f"{tag}{k}.in"), "wb") as f:
            f.write(struct.pack("=4i4d", h, len(frames), rate, 0, c["carrier_hz"], c["baud"], c["search_hz"], c["quality"]))
            f.write(np.asarray(frames, np.int32).tobytes() + flags.tobytes() + rows.tobytes())
        script.append("run %s %s" % (tmp / f"{tag}{k}.in", tmp / f"{tag}{k}.out"))
    run_script(exe, "\n".join(script) + "\n")
    out = []
    for k, (cfg, rows, flags, h, frames) in enumerate(jobs):
        raw = open(str(tmp / f"{tag}{k}.out"), "rb").read()
        F = len(flags)
        rec = np.frombuffer(raw, REC_DTYPE, F)
        states = np.frombuffer(raw, STATE_DTYPE, len(frames), 24 * F)
        ring = raw[24 * F + STATE_DTYPE.itemsize * len(frames):]
        assert len(ring) == TEXT
        out.append((rec, states, text_of(ring, int(states[-1]["nchars"]))))
        os.remove(str(tmp / f"{tag}{k}.in")), os.remove(str(tmp / f"{tag}{k}.out"))
    return out

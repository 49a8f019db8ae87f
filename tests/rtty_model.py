"""The RTTY decoder's models (include/psdr.h: psdr_client_set_rtty_decoder), written from the words of the header:
  records()       a numpy restatement in the rule's own f32 arithmetic - every fmaf exactly (tests/tone_model.py's fma32) - that
                  gives a stream's per-frame records and its text bit for bit;
  baudot(), fsk() the sender, with a code table of its own: phase-continuous FSK, the shift sent again behind every space (so that
                  it is right for either usos), 1, 1.5 or 2 stop bits, idle mark between characters;
  build_table(), run_streams()   the driver of tests/rtty_plan_table.cpp's `run` (phantomsdr_amd/csrc/rttyplan.h on the host).
Shared by tests/test_rtty_host.py and the GPU tests."""
import os
import struct
import subprocess

import numpy as np

from tone_model import cmul32, fma32

LANES, PAIRS, P0, WMAX, FILL, TEXT, TAB = 32, 16, 8, 24, 256, 1024, 4096
DF = 20.0
REC_DTYPE = np.dtype([("nchars", np.uint32), ("errors", np.uint32), ("offset_hz", np.float32), ("level", np.float32), ("quality", np.float32),
                      ("present", np.int32)])
STATE_DTYPE = np.dtype([("part", np.float32, 64), ("ring", np.float32, (24, 32, 2)), ("A", np.float32, 16), ("pos", np.uint64), ("nchars", np.uint64),
                        ("em", np.float32), ("es", np.float32), ("T", np.float32), ("Nn", np.float32), ("errors", np.uint32), ("p", np.int32),
                        ("present", np.int32), ("pad", np.int32), ("busy", np.int32), ("k", np.int32), ("i", np.int32), ("code", np.int32),
                        ("sp", np.int32), ("figs", np.int32)])
assert REC_DTYPE.itemsize == 24 and STATE_DTYPE.itemsize == 6536
SNR_DEFAULT = 7.5  # PSDR_RTTY_SNR_DEFAULT
DEFAULTS = dict(mark_hz=2125.0, shift_hz=170.0, baud=45.45, usos=1, search_hz=60.0, snr_db=SNR_DEFAULT)
# the decoder's table, by code: ITA2 with the US-TTY figures; "" prints nothing
LTRS = ["", "E", "\n", "A", " ", "S", "I", "U", "\r", "D", "R", "J", "N", "F", "C", "K", "T", "Z", "L", "W", "H", "Y", "P", "Q", "O", "B", "G", "", "M", "X",
        "V", ""]
FIGS = ["", "3", "\n", "-", " ", "\x07", "8", "7", "\r", "$", "4", "'", ",", "!", ":", "(", "5", '"', ")", "2", "#", "6", "0", "1", "9", "?", "&", "", ".",
        "/", ";", ""]
CODE_LTRS, CODE_FIGS, CODE_SPACE = 31, 27, 4
# the sender's own table, by character: the five bits in the order they are sent, 1 = mark
SEND_LTRS = {"A": "11000", "B": "10011", "C": "01110", "D": "10010", "E": "10000", "F": "10110", "G": "01011", "H": "00101", "I": "01100",
             "J": "11010", "K": "11110", "L": "01001", "M": "00111", "N": "00110", "O": "00011", "P": "01101", "Q": "11101", "R": "01010",
             "S": "10100", "T": "00001", "U": "11100", "V": "01111", "W": "11001", "X": "10111", "Y": "10101", "Z": "10001"}
SEND_FIGS = {"1": "11101", "2": "11001", "3": "10000", "4": "01010", "5": "00001", "6": "10101", "7": "11100", "8": "01100", "9": "00011",
             "0": "01101", "-": "11000", "\x07": "10100", "$": "10010", "'": "11010", ",": "00110", "!": "10110", ":": "01110", "(": "11110",
             '"': "10001", ")": "01001", "#": "00101", "?": "10011", "&": "01011", ".": "00111", "/": "10111", ";": "01111"}
SEND_BOTH = {" ": "00100", "\r": "00010", "\n": "01000"}
SEND_LTRS_SHIFT, SEND_FIGS_SHIFT = "11111", "11011"


def hop_of(rate):
    return 8 if rate < 8000 else 16 if rate < 16000 else 32 if rate < 32000 else 64


def wn_of(baud, rate):
    return max(2, int(np.floor(rate / (baud * hop_of(rate)) + 0.5)))


def u_of(baud, rate):
    return int(np.floor(16.0 * rate / (baud * hop_of(rate)) + 0.5))


def pair_hz(j):
    return DF * (np.asarray(j, np.float64) - P0)


def lane_hz(mark_hz, shift_hz):
    """f64 [32]: lane 2 j the mark tone of pair j, lane 2 j + 1 its space tone"""
    f = np.empty(LANES)
    f[0::2] = mark_hz + pair_hz(np.arange(PAIRS))
    f[1::2] = mark_hz + shift_hz + pair_hz(np.arange(PAIRS))
    return f


def candidates(search_hz):
    c = np.abs(pair_hz(np.arange(PAIRS))) <= search_hz
    c[P0] = True
    return c


def increments(rate, mark_hz, shift_hz):
    return np.array([int(np.floor(f / rate * 4294967296.0 + 0.5)) for f in lane_hz(mark_hz, shift_hz)], np.uint64)


def default_mark(rate):
    return 2125.0 if 2125.0 + 170.0 + 160.0 < 0.45 * rate else 915.0


# ---- the sender ----------------------------------------------------------------------------------------------------------------
def baudot(text):
    """the codes of `text` as strings of five bits in sending order, shifts included: the sender starts in letters and sends the
    shift of the next character again behind every space"""
    out, figs, again = [], False, False
    for ch in text:
        if ch in SEND_BOTH:
            out.append(SEND_BOTH[ch])
            again |= ch == " "
            continue
        want = ch in SEND_FIGS
        assert want or ch in SEND_LTRS, ch
        if want != figs or again:
            out.append(SEND_FIGS_SHIFT if want else SEND_LTRS_SHIFT)
        figs, again = want, False
        out.append((SEND_FIGS if want else SEND_LTRS)[ch])
    return out


def line_runs(text, baud, stop_bits=1.5, lead=0.8, tail=0.3, idle=None):
    """the line as (mark, seconds) runs: `lead` seconds of mark, per code a start bit, five data bits and the stop bits, idle[i]
    seconds of mark more behind code i (None: none), `tail` seconds of mark"""
    bit = 1.0 / baud
    runs = [(1, lead)]
    for i, code in enumerate(baudot(text)):
        runs.append((0, bit))
        runs += [(int(b), bit) for b in code]
        runs.append((1, stop_bits * bit + (0.0 if idle is None else float(idle[i]))))
    runs.append((1, tail))
    return runs


def fsk(text, baud, rate, mark=2125.0, shift=170.0, stop_bits=1.5, idle=None, amp=0.5, amp_space=None, lead=0.8, tail=0.3):
    """float64 [samples]: phase-continuous FSK of `text`; amp_space: the space tone's amplitude where it differs from the mark's"""
    runs = line_runs(text, baud, stop_bits, lead, tail, idle)
    edges = np.cumsum([0.0] + [r[1] for r in runs])
    n = int(round(edges[-1] * rate))
    at = np.minimum(np.round(edges * rate).astype(np.int64), n)
    mk = np.ones(n, bool)
    for (m, _), a, b in zip(runs, at[:-1], at[1:]):
        mk[a:b] = bool(m)
    f = np.where(mk, mark, mark + shift)
    ph = 2 * np.pi * np.concatenate([[0.0], np.cumsum(f[:-1])]) / rate
    return np.where(mk, amp, amp if amp_space is None else amp_space) * np.sin(ph + 0.4)


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def correlations(x, rate, mark_hz, shift_hz):
    """C f32 (re, im) [hops][32] of the whole hops of the stream x (f32) from position 0"""
    H = hop_of(rate)
    x = np.asarray(x, np.float32)
    nh = len(x) // H
    xb = x[:nh * H].reshape(nh, H)
    inc = increments(rate, mark_hz, shift_hz)
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


def energies(cr, ci, wn):
    """E f32 [hops][32] = |sum of the last wn hops' C, oldest first|^2 (hops before the start count as 0), not finite -> 0"""
    nh = len(cr)
    pr, pi = np.vstack([np.zeros((wn - 1, LANES), np.float32), cr]), np.vstack([np.zeros((wn - 1, LANES), np.float32), ci])
    sr, si = np.zeros((nh, LANES), np.float32), np.zeros((nh, LANES), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(wn):
            sr, si = (sr + pr[j:j + nh]).astype(np.float32), (si + pi[j:j + nh]).astype(np.float32)
        E = fma32(sr, sr, (si * si).astype(np.float32))
    return np.where(np.isfinite(E), E, np.float32(0)).astype(np.float32)


def f1(v):
    return np.float32(np.asarray(v).reshape(-1)[0])


class Framing:
    """the framing machine, integers: sample points u / 2 + i u behind the hop that started the character, in 1/16 hop"""

    def __init__(self, u, usos):
        self.u, self.usos = u, usos
        self.busy = self.k = self.i = self.code = self.sp = self.figs = 0
        self.errors = 0

    def step(self, mark):
        out = ""
        if not self.busy and not mark and not self.sp:
            self.busy, self.k, self.i, self.code = 1, 0, 0, 0
        if self.busy:
            c = self.u // 2 + self.i * self.u
            if 16 * self.k <= c < 16 * (self.k + 1):
                if self.i == 0:
                    if mark:
                        self.busy = 0
                    else:
                        self.i = 1
                elif self.i <= 5:
                    self.code |= mark << (self.i - 1)
                    self.i += 1
                else:
                    if mark:
                        if self.code == CODE_LTRS:
                            self.figs = 0
                        elif self.code == CODE_FIGS:
                            self.figs = 1
                        else:
                            out = (FIGS if self.figs else LTRS)[self.code]
                        if self.code == CODE_SPACE and self.usos:
                            self.figs = 0
                    else:
                        self.errors += 1
                    self.busy = 0
            self.k += 1
        self.sp = int(not mark)
        return out


def sequence(E, rate, baud=45.45, usos=1, search_hz=60.0, snr_db=SNR_DEFAULT, **_):
    """the order-dependent part over the hops' energies E f32 [hops][32]: per hop (nchars, errors, p, em, es, T, Nn, present), and
    the text"""
    nh = len(E)
    cand = candidates(search_hz)
    ratio = np.float32(10.0 ** (snr_db / 10.0))
    fr = Framing(u_of(baud, rate), usos)
    k64, k256, k16 = np.float32(0.015625), np.float32(-0.00390625), np.float32(0.0625)
    # the followers do not depend on a decision: all hops, pair-parallel
    A = np.zeros((nh, PAIRS), np.float32)
    a = np.zeros(PAIRS, np.float32)
    pairsum = (E[:, 0::2] + E[:, 1::2]).astype(np.float32)
    for b in range(nh):
        a = fma32((pairsum[b] - a).astype(np.float32), k64, a)
        A[b] = a
    p = P0
    em = es = T = Nn = np.float32(0)
    text, trace = "", []
    for b in range(nh):
        ab = np.where(cand, A[b].view(np.uint32).astype(np.int64), -1)
        q = int(np.argmax(ab))  # (the first of the largest)
        if A[b][q] > np.float32(2) * A[b][p]:
            p = q
        m, s = E[b][2 * p], E[b][2 * p + 1]
        d = f1(fma32(em, k256, em))
        pm = m if m > d else d
        d = f1(fma32(es, k256, es))
        ps = s if s > d else d
        em, es = max(pm, np.float32(ps * k16)), max(ps, np.float32(pm * k16))
        bit = int(np.float32(m * es) >= np.float32(s * em))
        t, n = (m, s) if m > s else (s, m)
        T = f1(fma32(np.float32(t - T), -k256, T))
        Nn = f1(fma32(np.float32(n - Nn), -k256, Nn))
        present = int(b + 1 >= FILL and np.isfinite(T) and T > 0 and T >= np.float32(ratio * Nn))
        text += fr.step(bit if present else 1)
        trace.append((len(text), fr.errors, p, em, es, T, Nn, present))
    return trace, text


def records(rows, flags, h, rate, **cfg):
    """(REC_DTYPE [F], text) of the stream rows f32 [F][h] from zero state: the model of the rule.  It sees the whole stream at once -
    the rule's records do not depend on the batches.  cfg: fields of DEFAULTS (mark_hz defaults to default_mark(rate))"""
    c = dict(DEFAULTS, mark_hz=default_mark(rate))
    c.update(cfg)
    flags = np.asarray(flags)
    rows = np.asarray(rows, np.float32).reshape(len(flags), h).copy()
    rows[flags != 0] = 0
    F, H, wn = len(flags), hop_of(rate), wn_of(c["baud"], rate)
    cr, ci = correlations(rows.reshape(-1), rate, c["mark_hz"], c["shift_hz"])
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        trace, text = sequence(energies(cr, ci, wn), rate, **c)
        lscale = np.float32(4.0 / (float(wn * H) * float(wn * H)))
        rec = np.zeros(F, REC_DTYPE)
        done = ((np.arange(F) + 1) * h) // H
        for f in range(F):
            if done[f]:
                n, errs, p, em, es, T, Nn, present = trace[done[f] - 1]
                q = np.float32(T) / np.float32(Nn) if Nn != 0 else np.float32(0)
                rec[f] = (n & 0xFFFFFFFF, errs & 0xFFFFFFFF, np.float32(20 * (p - P0)), np.float32(max(em, es) * lscale), q if np.isfinite(q) else 0.0, present)
    return rec, text


# ---- the table program ---------------------------------------------------------------------------------------------------------
def build_table(tmp, root, extra=(), name="rtty_plan_table"):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(root, "phantomsdr_amd", "csrc"),
                           "-I" + os.path.join(root, "tests"), os.path.join(root, "tests", "rtty_plan_table.cpp"), "-o", exe])
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
        c = dict(DEFAULTS, mark_hz=default_mark(rate))
        c.update(cfg)
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1)
        flags = np.ascontiguousarray(flags, np.int32)
        assert sum(frames) == len(flags) and len(rows) == len(flags) * h
        with open(str(tmp / f"{tag}{k}.in"), "wb") as f:
            f.write(struct.pack("=4i5d", h, len(frames), rate, c["usos"], c["mark_hz"], c["shift_hz"], c["baud"], c["search_hz"], c["snr_db"]))
            f.write(np.asarray(frames, np.int32).tobytes() + flags.tobytes() + rows.tobytes())
        script.append("run %s %s" % (tmp / f"{tag}{k}.in", tmp / f"{tag}{k}.out"))
    run_script(exe, "\n".join(script) + "\n")
    out = []
    for k, (cfg, rows, flags, h, frames) in enumerate(jobs):
        raw = open(str(tmp / f"{tag}{k}.out"), "rb").read()
        F = len(flags)
        rec = np.frombuffer(raw, REC_DTYPE, F)
        states = np.frombuffer(raw, STATE_DTYPE, len(frames), 24 * F)
        ring = raw[24 * F + 6536 * len(frames):]
        assert len(ring) == TEXT
        out.append((rec, states, text_of(ring, int(states[-1]["nchars"]))))
        os.remove(str(tmp / f"{tag}{k}.in")), os.remove(str(tmp / f"{tag}{k}.out"))
    return out

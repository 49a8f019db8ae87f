"""The radiofax decoder's models (include/psdr.h: psdr_client_set_fax_decoder), written from the words of the header:
  records()       a numpy restatement in the rule's own f32 arithmetic - every fmaf exactly (tests/tone_model.py's fma32) - that
                  gives a stream's per-frame records, every kept line and its meta bit for bit;
  tx_freq(), audio()   the sender: the instantaneous frequency of a synthetic transmission - silence, start tone, phasing lines,
                  an image, stop tone - at any sample rate, and the audio it makes;
  build_table(), run_streams(), angles()   the driver of tests/fax_plan_table.cpp.
Shared by tests/test_fax_host.py and the GPU tests."""
import math
import os
import struct
import subprocess

import numpy as np

from tone_model import cmul32, fma32

AUTO, FREE = 0, 1
IDLE, PHASING, IMAGE = 0, 1, 2
TAB, RING_MIN, PHASING_MAX, STATE_BYTES = 4096, 64, 80, 3224
TONE_HZ = (300.0, 450.0, 675.0)
HALF_PI = np.float32(1.57079637)
ATAN = [np.float32(c) for c in (0.0028662257, -0.0161657367, 0.0429096138, -0.0752896400, 0.1065626393, -0.1420889944, 0.1999355085, -0.3333314528, 1.0)]
REC_DTYPE = np.dtype([("nlines", np.uint32), ("state", np.int32), ("image", np.uint32), ("ioc", np.int32), ("offset_hz", np.float32), ("tone_quality", np.float32)])
assert REC_DTYPE.itemsize == 24
TONE_RATIO_DEFAULT = 0.22  # PSDR_FAX_TONE_RATIO_DEFAULT
DEFAULTS = dict(mode=AUTO, black_hz=1500.0, white_hz=2300.0, lpm=120.0, width=1024, slant_ppm=0.0, phase_col=0, tone_ratio=TONE_RATIO_DEFAULT, start_blocks=8,
                phase_lines=4, max_lines=0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def config(**cfg):
    c = dict(DEFAULTS)
    assert set(cfg) <= set(c), cfg
    c.update(cfg)
    return c


# ---- the plan's numbers --------------------------------------------------------------------------------------------------------
def hop_of(rate):
    return 8 if rate < 8000 else 16 if rate < 16000 else 32 if rate < 32000 else 64


def k_of(centre, rate):
    return max(2, int(math.floor(rate / (2.0 * centre) + 0.5)))


def d_of(rate):
    return max(1, int(math.floor(rate / 3200.0)))


def nb_of(rate):
    return int(math.floor(rate / (8.0 * hop_of(rate)) + 0.5))


def lq_of(lpm, slant_ppm, rate):
    return int(math.floor(65536.0 * 60.0 * rate / lpm * (1.0 + slant_ppm * 1e-6) + 0.5))


def ring_of(Lq, max_samples):
    return max(RING_MIN, 2 + max_samples * 65536 // Lq + 1)


def increment(hz, rate):
    return int(math.floor(hz / rate * 4294967296.0 + 0.5))


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def twiddles(hz, rate, nh):
    """w f32 (re, im) [nh][H]: per hop the seed at the exact phase of its first sample, then one rotation per sample"""
    H = hop_of(rate)
    inc = increment(hz, rate)
    j = np.arange(TAB)
    coarse = (np.cos(2 * np.pi * j / 4096.0).astype(np.float32), np.sin(2 * np.pi * j / 4096.0).astype(np.float32))
    fine = (np.cos(2 * np.pi * j / 16777216.0).astype(np.float32), np.sin(2 * np.pi * j / 16777216.0).astype(np.float32))
    ang = 2 * np.pi * inc / 4294967296.0
    rr, ri = np.float32(np.cos(ang)), np.float32(np.sin(ang))
    phase = ((np.arange(nh, dtype=np.uint64) * np.uint64(H) & np.uint64(0xFFFFFFFF)) * np.uint64(inc) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    wr, wi = cmul32(coarse[0][phase >> 20], coarse[1][phase >> 20], fine[0][(phase >> 8) & 4095], fine[1][(phase >> 8) & 4095])
    outr, outi = np.empty((nh, H), np.float32), np.empty((nh, H), np.float32)
    for n in range(H):
        outr[:, n], outi[:, n] = wr, wi
        wr, wi = cmul32(wr, wi, rr, ri)
    return outr, outi


def angle(re, im):
    """fax_angle on f32 arrays"""
    re, im = np.asarray(re, np.float32), np.asarray(im, np.float32)
    sat = np.where(im > 0, HALF_PI, np.where(im < 0, -HALF_PI, np.float32(0))).astype(np.float32)
    ok = np.isfinite(re) & np.isfinite(im) & (re > 0)
    swap = np.abs(im) > re
    with np.errstate(all="ignore"):
        q = np.where(swap, re / im, im / re).astype(np.float32)
    q = np.where(ok, np.clip(q, np.float32(-1), np.float32(1)), np.float32(0)).astype(np.float32)
    s = (q * q).astype(np.float32)
    p = fma32(ATAN[0], s, ATAN[1])
    for c in ATAN[2:]:
        p = fma32(p, s, c)
    a = (q * p).astype(np.float32)
    a = np.where(swap, (sat + -a).astype(np.float32), a)
    return np.where(ok, a, sat).astype(np.float32)


def shifted(a, i):
    """a[t - i], 0 before the start"""
    return a if i == 0 else np.concatenate([np.zeros(i, a.dtype), a[:-i]])


def discriminator(x, rate, black_hz, white_hz):
    """v f32 [T] of the stream x (f32) from position 0"""
    x = np.asarray(x, np.float32)
    T, H = len(x), hop_of(rate)
    centre, shift = (black_hz + white_hz) / 2.0, white_hz - black_hz
    K, D = k_of(centre, rate), d_of(rate)
    nh = -(-T // H)
    wr, wi = twiddles(centre, rate, nh)
    wr, wi = wr.reshape(-1)[:T], wi.reshape(-1)[:T]
    zr, zi = (x * wr).astype(np.float32), (-x * wi).astype(np.float32)
    yr, yi = np.zeros(T, np.float32), np.zeros(T, np.float32)
    for i in range(K):
        yr, yi = (yr + shifted(zr, i)).astype(np.float32), (yi + shifted(zi, i)).astype(np.float32)
    dr, di = shifted(yr, D), shifted(yi, D)
    with np.errstate(all="ignore"):
        dre = fma32(yr, dr, (yi * di).astype(np.float32))
        dim = fma32(yi, dr, -(yr * di).astype(np.float32))
    s = np.float32(rate / (2.0 * np.pi * D * shift))
    return np.clip(fma32(angle(dre, dim), s, np.float32(0.5)), np.float32(0), np.float32(1)).astype(np.float32)


def hop_sums(v, rate):
    """per whole hop of v: C f32 (re, im) [hops][3], Q [hops], M [hops]"""
    H = hop_of(rate)
    nh = len(v) // H
    u = (v[:nh * H].reshape(nh, H) + np.float32(-0.5)).astype(np.float32)
    cr, ci = np.zeros((nh, 3), np.float32), np.zeros((nh, 3), np.float32)
    for k, hz in enumerate(TONE_HZ):
        wr, wi = twiddles(hz, rate, nh)
        for n in range(H):
            cr[:, k] = fma32(u[:, n], wr[:, n], cr[:, k])
            ci[:, k] = fma32(-u[:, n], wi[:, n], ci[:, k])
    Q, M = np.zeros(nh, np.float32), np.zeros(nh, np.float32)
    for n in range(H):
        Q = fma32(u[:, n], u[:, n], Q)
        M = (M + u[:, n]).astype(np.float32)
    return cr, ci, Q, M


def pixels(v, ts, cols, line):
    """the pixels of the samples ts (ascending, columns cols) into `line`: the f32 sum in order, one division, the byte"""
    if len(ts) == 0:
        return
    first = np.flatnonzero(np.concatenate([[True], cols[1:] != cols[:-1]]))
    cnt = np.diff(np.concatenate([first, [len(ts)]]))
    acc = np.zeros(len(first), np.float32)
    for k in range(int(cnt.max())):
        m = cnt > k
        acc[m] = (acc[m] + v[ts[first[m] + k]]).astype(np.float32)
    p = (acc / cnt.astype(np.float32)).astype(np.float32)
    line[cols[first]] = np.minimum(255, np.floor(fma32(np.float32(255), p, np.float32(0.5))).astype(np.int64)).astype(np.uint8)


def search(pix, wp):
    """(dev, c*, total) of a line in the pulse's measure"""
    width = len(pix)
    p = pix.astype(np.int64)
    dark = 2 * int(p.sum()) >= 255 * width
    m = 255 - p if dark else p
    cs = np.concatenate([[0], np.cumsum(np.concatenate([m, m[:wp]]))])
    dev = cs[wp:wp + width] - cs[:width]
    c = int(np.argmax(dev))
    return int(dev[c]), c, int(m.sum())


def records(rows, flags, h, rate, **cfg):
    """(REC_DTYPE [F], lines uint8 [kept][width], meta uint32 [kept]) of the stream rows f32 [F][h] from zero state: the model of the
    rule.  It sees the whole stream at once - the rule's records do not depend on the batches.  cfg: fields of DEFAULTS"""
    c = config(**cfg)
    flags = np.asarray(flags)
    rows = np.asarray(rows, np.float32).reshape(len(flags), h).copy()
    rows[flags != 0] = 0
    F, H, NB, width = len(flags), hop_of(rate), nb_of(rate), c["width"]
    T = F * h
    Lq = lq_of(c["lpm"], c["slant_ppm"], rate)
    wp, sb = max(1, width // 20), c["start_blocks"]
    v = discriminator(rows.reshape(-1), rate, c["black_hz"], c["white_hz"])
    auto = c["mode"] == AUTO
    if auto:
        cr, ci, Q, M = hop_sums(v, rate)
    ratio, shift, nbh = np.float32(c["tone_ratio"]), np.float32(c["white_hz"] - c["black_hz"]), np.float32(NB * H)
    origin0 = c["phase_col"] * Lq // width
    state, image, ioc, nlines, skip = (IDLE if auto else IMAGE), 0, 0, 0, int(origin0 != 0)
    lstart = origin0 if origin0 else Lq
    Ff, quality = np.float32(0), np.float32(0)
    cnt = [0, 0, 0]
    run, prevc, plines, ilines = 0, -1, 0, 0
    line = np.zeros(width, np.uint8)
    kept, meta = [], []
    snaps_t, snaps = [-1], [(0, state, 0, 0, np.float32(shift * Ff), np.float32(0))]  # (an inverted picture reads -0 Hz)
    done = 0       # the first sample no line has taken yet
    blk = 0
    nblk = (T // H) // NB if auto else 0

    def snap(t):
        snaps_t.append(t), snaps.append((nlines & 0xFFFFFFFF, state, image, ioc, np.float32(shift * Ff), quality))

    with np.errstate(all="ignore"):
        while True:
            stop = -(-lstart // 65536)                       # the sample whose arrival completes the line
            t_line = stop if stop < T else None
            t_blk = (blk + 1) * NB * H - 1 if blk < nblk else None
            if t_line is None and t_blk is None:
                break
            if t_line is not None and (t_blk is None or t_line <= t_blk):
                ts = np.arange(done, stop, dtype=np.int64)
                pixels(v, ts, ((65536 * ts + Lq - lstart) * width // Lq), line)
                done = max(done, stop)
                move = 0
                if skip:
                    skip = 0
                elif state == PHASING:
                    dev, cstar, total = search(line, wp)
                    if dev >= 192 * wp and total - dev <= 64 * (width - wp):
                        d = abs(cstar - prevc)
                        d = min(d, width - d)
                        run = run + 1 if prevc >= 0 and d <= width // 64 else 1
                        prevc = cstar
                    else:
                        run, prevc = 0, -1
                    plines += 1
                    if run >= c["phase_lines"]:
                        state, move = IMAGE, (cstar + wp // 2) % width * Lq // width
                    elif plines >= PHASING_MAX:
                        state = IMAGE
                elif state == IMAGE:
                    kept.append(line.copy()), meta.append(image << 8 | state)
                    nlines, ilines = nlines + 1, ilines + 1
                    if c["max_lines"] and ilines >= c["max_lines"]:
                        state = IDLE
                lstart += move if move else Lq
                skip = 1 if move else skip
                snap(t_line)
            else:
                hs = slice(blk * NB, (blk + 1) * NB)
                S = np.zeros((3, 2), np.float32)
                SQ = SM = np.float32(0)
                for b in range(hs.start, hs.stop):
                    S[:, 0], S[:, 1] = S[:, 0] + cr[b], S[:, 1] + ci[b]
                    SQ, SM = np.float32(SQ + Q[b]), np.float32(SM + M[b])
                den = np.float32(nbh * SQ)
                rho = (np.float32(2) * fma32(S[:, 0], S[:, 0], (S[:, 1] * S[:, 1]).astype(np.float32))).astype(np.float32) / den
                rho = np.where(np.isfinite(rho), rho, np.float32(0)).astype(np.float32)
                best = int(np.argmax(rho))
                quality = rho[best]
                hit = best if rho[best] >= ratio else -1
                cnt = [min(2 * sb, max(0, n + (1 if k == hit else -1))) for k, n in enumerate(cnt)]
                if hit >= 0:
                    Ff = fma32(np.float32(SM / nbh) - Ff, np.float32(0.125), Ff).reshape(())[()]
                if cnt[1] >= sb:
                    state, cnt = IDLE, [0, 0, 0]
                elif state == IDLE and (cnt[0] >= sb or cnt[2] >= sb):
                    ioc = 576 if cnt[0] >= sb else 288
                    state, image = PHASING, image + 1
                    run, prevc, plines, ilines, cnt = 0, -1, 0, 0, [0, 0, 0]
                blk += 1
                snap(t_blk)
    rec = np.zeros(F, REC_DTYPE)
    D = ((np.arange(F) + 1) * h) // H
    at = np.searchsorted(np.asarray(snaps_t), D * H - 1, side="right") - 1
    for f in range(F):
        rec[f] = snaps[at[f]] if D[f] else snaps[0]
    lines = np.array(kept, np.uint8).reshape(len(kept), width)
    return rec, lines, np.array(meta, np.uint32)


def ring_tail(lines, meta, R):
    """what a ring of R lines still holds of all the kept lines"""
    return lines[max(0, len(lines) - R):], meta[max(0, len(meta) - R):]


# ---- the sender ----------------------------------------------------------------------------------------------------------------
def tx_freq(fs, image, lpm=120.0, black_hz=1500.0, white_hz=2300.0, lead=0.3, start_hz=300.0, start_s=1.5, phasing=8, dark_pulse=False, stop_s=1.5, tail=0.3,
            offset=0.0):
    """(freq f64 [samples], on bool [samples]) at sample rate fs: `lead` s of nothing, start_s of the carrier switched between black
    and white at start_hz (0 s: none), `phasing` lines with a pulse of a twentieth of the line centred on the line's start (white on
    black, or dark on white), the rows of `image` (values 0 .. 1, any width: a pixel lasts line / width), stop_s of 450 Hz
    switching, `tail` s of nothing; `offset` s shifts the sender's line grid"""
    image = np.asarray(image, np.float64)
    line_s = 60.0 / lpm
    parts = [lead, start_s, phasing * line_s, len(image) * line_s, stop_s, tail]
    edges = np.cumsum([0.0] + parts)
    n = int(round(edges[-1] * fs))
    t = np.arange(n) / fs
    val = np.zeros(n)
    on = (t >= edges[1]) & (t < edges[5])
    seg = lambda i: (t >= edges[i]) & (t < edges[i + 1])  # noqa: E731
    m = seg(1)
    val[m] = (np.floor(2 * start_hz * (t[m] - edges[1])) % 2 == 0)
    m = seg(4)
    val[m] = (np.floor(2 * 450.0 * (t[m] - edges[4])) % 2 == 0)
    m = seg(2)
    u = ((t[m] - edges[2] + offset) / line_s) % 1.0
    pulse = (u < 0.025) | (u >= 0.975)
    val[m] = np.where(pulse, 0.0, 1.0) if dark_pulse else np.where(pulse, 1.0, 0.0)
    m = seg(3)
    if m.any():
        lt = (t[m] - edges[3] + offset) / line_s
        row = np.minimum(np.floor(lt).astype(np.int64), len(image) - 1)
        col = np.floor((lt % 1.0) * image.shape[1]).astype(np.int64)
        val[m] = image[row, col]
    return black_hz + (white_hz - black_hz) * val, on


def audio(freq, on, fs, amp=0.5):
    return amp * on * np.cos(2 * np.pi * np.cumsum(freq) / fs)


def framed(x, h):
    F = -(-len(x) // h)
    return np.concatenate([x, np.zeros(F * h - len(x))]).astype(np.float32), np.zeros(F, np.int32)


def test_image(lines, width):
    """a grey ramp along the line plus a checkerboard of 8-pixel squares, values 0 .. 1"""
    r, cidx = np.arange(lines)[:, None], np.arange(width)[None, :]
    ramp = cidx / (width - 1.0)
    check = ((r // 8 + cidx // 8) % 2) * 0.25
    return 0.75 * ramp + check


# ---- the table program ---------------------------------------------------------------------------------------------------------
def build_table(tmp, root=ROOT, extra=(), name="fax_plan_table"):
    exe = os.path.join(str(tmp), name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(root, "phantomsdr_amd", "csrc"),
                           "-I" + os.path.join(root, "tests"), os.path.join(root, "tests", "fax_plan_table.cpp"), "-o", exe])
    return exe


def run_script(exe, script, timeout=900):
    r = subprocess.run([exe], input=script, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def run_streams(exe, tmp, jobs, tag="job", rate=12000):
    """jobs: [(cfg dict like DEFAULTS, rows f32 [F * h], flags [F], h, frames)] ->
    [(rec REC_DTYPE [F], final state bytes, lines uint8 [min(total, R)][width], meta, total, R)], one process"""
    script = []
    for k, (cfg, rows, flags, h, frames) in enumerate(jobs):
        c = config(**cfg)
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1)
        flags = np.ascontiguousarray(flags, np.int32)
        assert sum(frames) == len(flags) and len(rows) == len(flags) * h
        with open(str(tmp / f"{tag}{k}.in"), "wb") as f:
            f.write(struct.pack("=10i5d", h, len(frames), rate, max(frames), c["mode"], c["width"], c["phase_col"], c["start_blocks"], c["phase_lines"], c["max_lines"],
                                c["black_hz"], c["white_hz"], c["lpm"], c["slant_ppm"], c["tone_ratio"]))
            f.write(np.asarray(frames, np.int32).tobytes() + flags.tobytes() + rows.tobytes())
        script.append("run %s %s" % (tmp / f"{tag}{k}.in", tmp / f"{tag}{k}.out"))
    run_script(exe, "\n".join(script) + "\n")
    out = []
    for k, (cfg, rows, flags, h, frames) in enumerate(jobs):
        raw = open(str(tmp / f"{tag}{k}.out"), "rb").read()
        F, width = len(flags), config(**cfg)["width"]
        rec = np.frombuffer(raw, REC_DTYPE, F)
        at = 24 * F + STATE_BYTES * len(frames)
        state = raw[at - STATE_BYTES:at]
        R = int(np.frombuffer(raw, np.int32, 1, at)[0])
        meta = np.frombuffer(raw, np.uint32, R, at + 4)
        ring = np.frombuffer(raw, np.uint8, R * width, at + 4 + 4 * R).reshape(R, width)
        total = int(np.frombuffer(state, np.uint64, 1, 3080)[0])  # FaxState.z.nlines
        idx = [i % R for i in range(max(0, total - R), total)]
        out.append((rec, state, ring[idx], meta[idx], total, R))
        os.remove(str(tmp / f"{tag}{k}.in")), os.remove(str(tmp / f"{tag}{k}.out"))
    return out


def angles(exe, tmp, re, im):
    """fax_angle of the host program over f32 arrays"""
    pairs = np.stack([np.asarray(re, np.float32), np.asarray(im, np.float32)], axis=1)
    open(str(tmp / "angle.in"), "wb").write(pairs.tobytes())
    run_script(exe, "angle %s %s\n" % (tmp / "angle.in", tmp / "angle.out"))
    return np.fromfile(str(tmp / "angle.out"), np.float32)

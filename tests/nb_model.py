"""The impulse blanker's rule (include/psdr.h: psdr_ring_set_blanker) restated in numpy, for all six formats and both input
kinds, written from the words of the header - and the streams the blanker's tests run on (fixture()).  A half-frame is a 1-D
array of raw COMPONENTS in the format's dtype (interleaved I/Q for IQ input)."""
import numpy as np

from helpers import quantize_raw, synth_stream

BLOCK = 256
FMT_ID = {"u8": 0, "s8": 1, "u16": 2, "s16": 3, "f32": 4, "f64": 5}
DTYPE = {"u8": np.uint8, "s8": np.int8, "u16": np.uint16, "s16": np.int16, "f32": np.float32, "f64": np.float64}
OFFSET = {"u8": 128, "s8": 0, "u16": 32768, "s16": 0}  # the MSB flip is a subtraction of the offset


def factor(threshold_db):
    return np.float32(10.0 ** (threshold_db / 10))


def zero_code(fmt):
    return DTYPE[fmt](OFFSET.get(fmt, 0))


def power(raw, fmt, is_real):
    """P, one f32 per sample"""
    comp = raw.reshape(-1, 1 if is_real else 2)
    if fmt in OFFSET:
        v = comp.astype(np.int64) - OFFSET[fmt]
        u = (v * v).sum(axis=1)
        assert int(u.max(initial=0)) <= 1 << 31
        return u.astype(np.float32)  # one conversion, round to nearest even
    with np.errstate(all="ignore"):
        c = comp.astype(np.float32)  # f64 is narrowed first
        sq = c * c  # f32 products, each rounded
        return sq[:, 0] if is_real else (sq[:, 0] + sq[:, 1]).astype(np.float32)


def maximum(P):
    """m = (P > m) ? P : m from +0.0: a NaN is never a maximum"""
    m = np.float32(0.0)
    for p in P:
        if p > m:
            m = p
    return np.float32(m)


def block_maxima(P):
    # np.fmax ignores NaN; an all-NaN block keeps the initial +0.0
    with np.errstate(all="ignore"):
        return np.fmax.reduce(np.fmax(P.reshape(-1, BLOCK), np.float32(0.0)), axis=1).astype(np.float32)


def level(P):
    return np.float32(block_maxima(P).min())


def threshold(kf, R):
    with np.errstate(all="ignore"):
        return np.float32(np.float32(kf) * np.float32(R))


def blank(raw, fmt, is_real, T, guard):
    """-> (the half's new components, samples zeroed)"""
    P = power(raw, fmt, is_real)
    if not (T > 0 and np.isfinite(T)):
        return raw.copy(), 0
    with np.errstate(invalid="ignore"):
        exceed = P > T
    hit = np.zeros(len(P), bool)
    for j in np.flatnonzero(exceed):
        hit[max(0, j - guard):j + guard + 1] = True  # clipped to the half
    out = raw.copy().reshape(len(P), -1)
    out[hit] = zero_code(fmt)
    return out.reshape(-1), int(hit.sum())


class Blanker:
    """one context's blanker: process() is one psdr_process_ring call on `store`, the list of the stream's halves as the ring
    holds them (blanked in place, each once)"""

    def __init__(self, fmt, is_real, threshold_db, guard):
        self.fmt, self.is_real, self.kf, self.guard = fmt, is_real, factor(threshold_db), guard
        self.next, self.fresh, self.R_prev = 0, True, None

    def process(self, store, first, nframes):
        """-> {half: (count, R)} of the halves this call blanked"""
        if self.fresh or first > self.next:
            self.next, self.R_prev = first, None
        self.fresh = False
        out = {}
        for h in range(max(first, self.next), first + nframes + 1):
            R = level(power(store[h], self.fmt, self.is_real))  # from the RAW samples
            T = threshold(self.kf, R if self.R_prev is None else self.R_prev)
            store[h], n = blank(store[h], self.fmt, self.is_real, T, self.guard)
            out[h] = (n, R)
            self.R_prev, self.next = R, h + 1
        return out


# ---- the streams of the tests -------------------------------------------------------------------------------------------------
NHALVES, MAX_BATCH, STREAM_HALVES = 8, 4, 24
THRESHOLD_DB = 12.0
SPLIT_A = [(f, min(4, STREAM_HALVES - 1 - f)) for f in range(0, STREAM_HALVES - 1, 4)]  # 4+4+...
SPLIT_B = []  # 1+3+2+2+...
_f = 0
while _f < STREAM_HALVES - 1:
    for _n in (1, 3, 2, 2):
        _n = min(_n, STREAM_HALVES - 1 - _f)
        if _n:
            SPLIT_B.append((_f, _n))
            _f += _n
JUMP = [(0, 4), (12, 4), (16, 4)]  # halves 5..11 are never read: half 12 starts the reference again


def shape(is_real):
    """N: the smallest the library accepts - 8 blocks per half for IQ input, 16 for real"""
    return 1 << 13 if is_real else 1 << 12


def plants(hs, guard, floats):
    """(half, sample, kind): kind 'imp' an impulse, 'nan' / 'inf' a non-finite sample"""
    near = max(1, min(3, guard))  # two impulses closer together than the guard (guard 0: neighbours)
    p = [(2, 0, "imp"), (3, hs - 1, "imp"), (5, 255, "imp"), (5, 256, "imp"), (6, 1000, "imp"), (6, 1000 + near, "imp"),
         (8, 700, "imp"), (16, 5, "imp"),  # halves that land in slot 0
         (12, 1234, "imp")]  # the half right behind the jump of JUMP
    if floats:
        p += [(10, 300, "nan"), (14, 400, "inf")]
    return p


def fixture(fmt, is_real, guard, planted=True, seed=11):
    """-> (halves: list of raw component arrays, plants)"""
    N = shape(is_real)
    hs = N // 2
    x = synth_stream(STREAM_HALVES * hs, is_real, seed=seed, ntones=0, fft_size=N)
    pl = plants(hs, guard, fmt in ("f32", "f64")) if planted else []
    for h, s, kind in pl:
        v = {"imp": 0.9, "nan": np.nan, "inf": np.inf}[kind]
        x[h * hs + s] = v if is_real else complex(v, -v if kind == "imp" else 0.0)
    raw = quantize_raw(x, fmt, is_real)
    return [h.copy() for h in raw.reshape(STREAM_HALVES, -1)], pl


def expected_hits(hs, pl, half, guard):
    """the samples of `half` the planted impulses (and the +Inf sample) must zero, with their full guard"""
    hit = np.zeros(hs, bool)
    for h, s, kind in pl:
        if h == half and kind != "nan":
            hit[max(0, s - guard):s + guard + 1] = True
    return hit

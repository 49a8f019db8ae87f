"""The impulse blanker's rule (include/psdr.h: psdr_ring_set_blanker) restated in numpy, for all six formats and both input
kinds, written from the words of the header - and the streams the blanker's tests run on (fixture()).  A half-frame is a 1-D
array of raw COMPONENTS in the format's dtype (interleaved I/Q for IQ input)."""
import functools

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


# ---- streams at other shapes (tests/test_blanker_shapes_host.py, tests/test_gpu_blanker_shapes.py) ----------------------------
# plants of stream(): (half, sample, "imp" | "nan" | "inf") as above, and whole-block / whole-half kinds:
#   (half, block, "quiet")     the block's samples scaled down by quiet_scale(fmt): this block alone decides R of the half
#   (half, block, "nanblock")  every component of the block a NaN (floats): M_b = 0, so R = 0
#   (half, 0, "huge")          every component of the half near 7e18 (floats): R near 1e38, kf * R = +Inf
SIGMA = {"u8": 3.0 / 128, "s8": 3.0 / 128}  # 8-bit noise: 3 codes rms, so that a block scaled by 1/3 still has a maximum above 0
QUIET = {"u8": 1.0 / 3, "s8": 1.0 / 3}


def sigma(fmt):
    return SIGMA.get(fmt, 2.0 ** -9)


def quiet_scale(fmt):
    return QUIET.get(fmt, 0.25)


def stream_db(fmt):
    """threshold_db of the streams with quiet blocks: the lowered threshold kf * R_quiet stays above every noise sample and the
    usual one below the impulse (tests/test_blanker_shapes_host.py asserts both)"""
    return 16.0 if fmt in SIGMA else 20.0


class Stream:
    """a stream and the shape it was made for"""

    def __init__(self, fmt, is_real, N, max_batch, nhalves, halves, plants):
        self.fmt, self.is_real, self.N, self.max_batch, self.nhalves = fmt, is_real, N, max_batch, nhalves
        self.halves, self.plants, self.models, self._bmax = halves, plants, {}, {}
        self.hs = N // 2  # samples per half
        self.nblocks = self.hs // BLOCK
        self.sb = np.dtype(DTYPE[fmt]).itemsize * (1 if is_real else 2)
        self.hb = self.hs * self.sb
        self.tiles = self.hb // 4096  # the streaming kernel's tiles per half
        self.cpb = BLOCK * self.sb // 16  # ... and its 16-byte chunks per block

    def split(self, *pattern):
        """calls of pattern[0], pattern[1], .. frames, repeated over the stream"""
        calls, f, last = [], 0, len(self.halves) - 1
        while f < last:
            for n in pattern:
                n = min(n, last - f)
                if n:
                    assert f % self.nhalves + n <= self.nhalves and n <= self.max_batch
                    calls.append((f, n))
                    f += n
        return calls

    def kinds(self, *kinds):
        return [p for p in self.plants if p[2] in kinds]

    def bmax(self, h):
        """the block maxima of the RAW half h"""
        if h not in self._bmax:
            self._bmax[h] = block_maxima(power(self.halves[h], self.fmt, self.is_real))
        return self._bmax[h]

    def listed(self, calls, db):
        """per call, the blocks on the work list: a block of a new half that holds a sample above T, or whose neighbour in the
        half does (calls that start at half 0 and move forward only)"""
        out, nxt = [], 0
        for first, n in calls:
            tot = 0
            for h in range(max(first, nxt), first + n + 1):
                T = threshold(factor(db), self.bmax(h if h == 0 else h - 1).min())
                if T > 0 and np.isfinite(T):
                    ex = self.bmax(h) > T
                    ex[1:] |= ex[:-1].copy()
                    ex[:-1] |= (self.bmax(h) > T)[1:]
                    tot += int(ex.sum())
            out.append(tot)
            nxt = max(nxt, first + n + 1)
        return out


def stream(fmt, is_real, N, max_batch, nhalves, stream_halves, plants, seed=23):
    """noise of sigma(fmt) drawn in f32 (cheap at 2 MiB a half), quantized like helpers.quantize_raw, with `plants`"""
    hs, ncomp = N // 2, N // 2 * (1 if is_real else 2)
    rng = np.random.default_rng(seed)
    off, dt = OFFSET.get(fmt), DTYPE[fmt]
    halves = []
    for h in range(stream_halves):
        x = rng.standard_normal(ncomp, dtype=np.float32) * np.float32(sigma(fmt))
        mine = [p for p in plants if p[0] == h]
        if any(k == "huge" for _, _, k in mine):
            x = np.where(x < 0, np.float32(-7e18), np.float32(7e18)) * (1 + 0.1 * rng.uniform(-1, 1, ncomp).astype(np.float32))
        c = x.reshape(hs, -1)
        for _, s, kind in mine:
            if kind == "quiet":
                c[s * BLOCK:(s + 1) * BLOCK] *= np.float32(quiet_scale(fmt))
            elif kind == "nanblock":
                c[s * BLOCK:(s + 1) * BLOCK] = np.nan
            elif kind != "huge":
                v = {"imp": 0.9, "nan": np.nan, "inf": np.inf}[kind]
                c[s] = v if is_real else (v, -v if kind == "imp" else 0.0)
        if fmt in OFFSET:
            full = 128 if dt().itemsize == 1 else 32768
            raw = (np.clip(np.rint(x * np.float32(full)), -full, full - 1).astype(np.int32) + off).astype(dt)
        else:
            raw = x.astype(dt)
        halves.append(raw)
    return Stream(fmt, is_real, N, max_batch, nhalves, halves, list(plants))


def run_model(st, calls, db, guard):
    """-> (the model-blanked halves, {half: (count, R)}); computed once per stream and arguments and shared: read only"""
    key = (tuple(calls), db, guard)
    if key not in st.models:
        model, nb, seen = [h.copy() for h in st.halves], Blanker(st.fmt, st.is_real, db, guard), {}
        for first, n in calls:
            seen.update(nb.process(model, first, n))
        for h in model:
            h.flags.writeable = False
        st.models[key] = (model, seen)
    return st.models[key]


def dense_plants(half, nblocks):
    """an impulse in every second block at varying offsets - sample 0 and sample 255 of a block among them - and one pair of
    adjacent blocks that both carry one; the odd blocks in between stay clean"""
    offs = (0, 255, 1, 100, 254, 37, 128, 200)
    p = [(half, b * BLOCK + offs[(b // 2) % len(offs)], "imp") for b in range(0, nblocks, 2)]
    return p + [(half, 5 * BLOCK + 255, "imp")]  # block 5 beside block 6 (offset 100) and block 4 (offset 1)


def edge_plants(st_hs, sb, half):
    """the last sample of one 4 KiB tile and the first of the next; the half's first and last sample"""
    t = 4096 // sb
    return [(half, 0, "imp"), (half, 3 * t - 1, "imp"), (half, 3 * t, "imp"), (half, st_hs - 1, "imp")]


# (b): more than 64 and more than 256 blocks; max_batch 8, a ring of 16 halves, 33 halves of stream
B_SHAPES = [("s16", False, 1 << 16), ("u8", True, 1 << 17)]
B_DENSE = list(range(9, 16)) + list(range(25, 30))  # the new halves of the calls (8, 8) and (24, 8) of 8+8+8+8


@functools.lru_cache(maxsize=2)  # (the host file and the GPU file walk the shapes in order)
def stream_b(fmt, is_real, N):
    hs = N // 2
    nblocks, sb = hs // BLOCK, np.dtype(DTYPE[fmt]).itemsize * (1 if is_real else 2)
    pl = [(2, 64, "quiet"), (4, 127, "quiet"), (6, nblocks - 1, "quiet"), (18, 64, "quiet"), (20, nblocks - 1, "quiet"),
          (3, 64 * BLOCK + 9, "imp"), (5, 777, "imp"), (7, hs - 1, "imp"), (19, 1, "imp"), (21, 4000, "imp")]  # behind the lowered thresholds
    for h in B_DENSE:
        pl += dense_plants(h, nblocks)
    pl += edge_plants(hs, sb, 16) + edge_plants(hs, sb, 32) + edge_plants(hs, sb, 24)  # slot 0 twice; the last halves of calls of 8 frames
    return stream(fmt, is_real, N, 8, 16, 33, pl)


# (c): 2 MiB halves of 512 tiles; max_batch 9, a ring of 18 halves, three calls of 9 frames (10, 9 and 9 new halves)
C_SHAPES = [("f64", False, 1 << 18), ("f64", True, 1 << 19), ("s16", False, 1 << 20), ("u8", True, 1 << 22)]
C_CALLS = [(0, 9), (9, 9), (18, 9)]
C_GUARD = [255, 7, 7, 255]  # per shape
C_QUIET = [(8, 3), (9, 500), (18, 300), (27, 510)]  # (half, tile): new half 8 or 9 of its call, tile index in the call >= 4096


@functools.lru_cache(maxsize=1)
def stream_c(fmt, is_real, N):
    hs = N // 2
    sb = np.dtype(DTYPE[fmt]).itemsize * (1 if is_real else 2)
    bpt = 4096 // (sb * BLOCK)  # blocks per tile: 16 (one byte a sample) .. 1 (sixteen)
    pl = [(h, tile * bpt + bpt - 1, "quiet") for h, tile in C_QUIET]
    pl += edge_plants(hs, sb, 9) + edge_plants(hs, sb, 18) + edge_plants(hs, sb, 27)  # each call's last half; 18 lands in slot 0
    pl += [(10, 12345, "imp"), (19, hs // 2 + 7, "imp"), (4, 256 * 300 + 255, "imp"), (4, 256 * 301, "imp")]  # behind the quiet halves 9 and 18
    return stream(fmt, is_real, N, 9, 18, 28, pl)


# (d): thresholds that blank nothing, at the smallest shapes
D_SHAPES = [("f32", True, 1 << 13), ("f64", False, 1 << 12)]
D_PLANTS = [(2, 100, "imp"), (5, 0, "huge"), (6, 900, "imp"), (7, 901, "imp"), (9, 1500, "imp"),
            (12, 3, "nanblock"), (13, 600, "imp"), (14, 601, "imp")]


@functools.lru_cache(maxsize=2)
def stream_d(fmt, is_real, N):
    return stream(fmt, is_real, N, MAX_BATCH, NHALVES, STREAM_HALVES, D_PLANTS)


# (e): rewrites without host waits
E_SHAPE = ("s16", False, 1 << 20)


@functools.lru_cache(maxsize=1)
def stream_e():
    fmt, is_real, N = E_SHAPE
    hs = N // 2
    pl = []
    for h in (0, 5, 8, 16, 24, 31, 32, 40, 47, 48):  # slot 0 four times, the last half of every call of 8 frames
        pl += edge_plants(hs, 4, h)
    return stream(fmt, is_real, N, 8, 16, 49, pl)

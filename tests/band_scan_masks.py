"""The inputs, the sweep and the coverage counters of the band scan's mask tests: what a hot mask must look like for the device-only
parts of the scan (phantomsdr_amd/csrc/scan.hip: the ballots, k_scan_mark's block scan, k_scan_emit's two peak paths and its early
return, the clearing of the list) to have run at all.  tests/test_band_scan_masks_host.py holds the inputs to these conditions on the
CPU oracle's values, without a GPU; tests/test_gpu_band_scan_masks.py runs them and holds the GPU's own values to the same
conditions.  No pytest and no GPU in here.

Inputs (raw s16, cached, deterministic, built like tests/test_gpu_band_scan.py's stream()):
  noise       white noise only.  A bin's power is exponentially distributed, so its int8 value spreads over some 60 counts of
              0.5 dB around the floor and a low threshold cuts a pseudo-random mask.  The hot density of one level-0 frame:
              threshold 1: 0.76, 2: 0.74, 4: 0.69, 8: 0.55, 16: 0.22 - the exponential law leaves 22 % of the bins 8 dB above the
              quartile, whatever sigma is; one in a hundred is reached where the pyramid has narrowed the law (1.3 % at level 2,
              none at level 4).  sigma = 2^-6 keeps every bin of every shape inside (-128, 127).
  gap_edges   low noise and bin-centred tones at level 0 of a 4096-bin band; under the Hann window a tone is the three hot bins
              c - 1 .. c + 1 (a blob).  PAIRS lists the pairs of blobs by the cold bins between them; the groups lie more than 80
              bins apart, so only the two blobs of a pair ever join:
                close    0, 1, 2, 3, 4, 7, 8 and 9 cold bins
                words    62 .. 65 cold bins from bit 23 of a word into the next, both words in one segment
                border   62 .. 65 cold bins across a segment border
                aligned  the lower blob ends on bit 63 of word w - 2, the upper starts on bit 0 of word w: word w - 1 is 64 cold bins,
                         inside the run at gap 64 and outside every run below.  The upper blob is 6 dB stronger: the run's peak is
                         its centre, a peak taken over the lower blob alone is wrong
                beyond   the same with the upper blob on bit 1: 65 cold bins, word w - 1 is all cold between two hot words and
                         inside no run at any gap
              gap_edge_runs(gap) derives the (first, end) pairs from PAIRS alone.
  decay       noise and a comb of strong tones, one every 16 bins, that stops after the first third of the frames: 256 bins and
              their neighbours then fall by some 75 counts, for the rest of the stream.

cover(s, threshold, gap, words_per_thread) counts, for one evaluation of a trace, what the mask exercises; it is numpy and
tests/scan_model.py only.  noise_rules() names the counters that the noise masks of a shape must reach somewhere in the sweep.  One
counter is not among them: an all-cold word inside a run needs a cold stretch of exactly 64 bins on a word's borders (gap is at most
64), which a mask of density p holds with probability p^2 (1 - p)^64 <= 1.3e-4 per word - and 6e-9 at the 22 % that threshold 16
leaves at level 0.  No choice of sigma changes that; the condition is carried by gap_edges, whose aligned pair is built for it."""
import functools

import numpy as np

import scan_model as M
from helpers import quantize_raw

THRESHOLDS = (1, 2, 4, 8, 16, 255)
GAPS = (0, 1, 2, 7, 31, 62, 63, 64)
MARK_THREADS = 1024  # scan.h: SCAN_MARK_THREADS (held to the header by tests/test_band_scan_masks_host.py)

# (fft size, real input, level): the smallest shapes at which each mechanism exists
SHAPES = (
    (1 << 12, False, 0),  # 4096 bins, 64 words: one word per k_scan_mark thread, 960 idle threads
    (1 << 12, False, 4),  # 256 bins, 4 words: one segment
    (1 << 13, True, 0),   # 4096 bins: level-major addressing only
    (1 << 13, True, 2),   # 1024 bins, 16 words
    (1 << 17, False, 0),  # 131 072 bins, 2048 words: two words per k_scan_mark thread, the cap can fall inside a word
    (1 << 17, False, 1),  # 65 536 bins, 1024 words: every k_scan_mark thread owns exactly one word
)
NOISE_SIGMA = 2.0 ** -6
NOISE_TRACES = ((1, 0), (3, 3))  # (frames, avg_shift): one frame as it is - full of ties - and three frames smoothed


def bins_of(N, is_real):
    return N // 2 if is_real else N


def levels_of(N, is_real, floor_bins=256):
    """every level that still holds a segment, as tests/test_gpu_band_scan.py's levels_for"""
    lv = 0
    while (bins_of(N, is_real) >> lv) >= floor_bins:
        lv += 1
    return lv


def words_per_thread(n):
    return -(-(n // 64) // MARK_THREADS)


def level_of(q, R, level):
    """one level of a frame's int8 pyramid"""
    off = sum(R >> t for t in range(level))
    return q[off:off + (R >> level)]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _raw(N, is_real, nframes, seed, sigma, tones, stop=None):
    """noise of `sigma` plus the (client bin, amplitude) tones on bin centres, the tones only in front of sample `stop`"""
    h = N // 2
    ns = (nframes + 1) * h
    rng = np.random.default_rng(seed)
    t = np.arange(ns if stop is None else stop, dtype=np.float64)
    if is_real:
        x = rng.standard_normal(ns) * sigma
        for c, amp in tones:
            x[:len(t)] += 2 * amp * np.cos(2 * np.pi * (c / N) * t + rng.uniform(0, 6.28))
    else:
        x = (rng.standard_normal(ns) + 1j * rng.standard_normal(ns)) * sigma
        for c, amp in tones:
            k = (c + N // 2 + 1) % N  # client bin c is bin k of the transform
            x[:len(t)] += amp * np.exp(1j * (2 * np.pi * ((k * t) % N) / N + rng.uniform(0, 6.28)))
    assert np.abs(x.real).max() < 1.0 and np.abs(x.imag).max() < 1.0  # nothing clips
    return quantize_raw(x, "s16", bool(is_real))


@functools.lru_cache(maxsize=None)
def noise(N, is_real, nframes, seed=5):
    return _raw(N, is_real, nframes, seed, NOISE_SIGMA, ())


EDGE_THR, EDGE_SIGMA, EDGE_AMP, EDGE_STRONG = 40, 2.0 ** -9, 0.01, 0.02
EDGE_GAPS = (0, 1, 2, 3, 7, 8, 62, 63, 64)
EDGE_BINS = 4096
# (group, first hot bin of the lower blob, cold bins between the blobs, amplitude of the upper blob)
PAIRS = tuple(
    [("close", 100 + 100 * i, cold, EDGE_AMP) for i, cold in enumerate((0, 1, 2, 3, 4, 7, 8, 9))]
    + [("words", 64 * (16 + 4 * i) + 20, cold, EDGE_AMP) for i, cold in enumerate((62, 63, 64, 65))]
    + [("aligned", 64 * 34 - 3, 64, EDGE_STRONG), ("beyond", 64 * 38 - 3, 65, EDGE_AMP)]
    + [("border", 256 * (11 + i) - 30, cold, EDGE_AMP) for i, cold in enumerate((62, 63, 64, 65))])
ALIGNED_WORD, BEYOND_WORD = 34, 38  # the all-cold words of the two groups


def edge_blobs():
    """[(first hot bin, amplitude)] of every blob, ascending"""
    out = []
    for _, lo, cold, amp in PAIRS:
        out += [(lo, EDGE_AMP), (lo + 3 + cold, amp)]
    assert out == sorted(out)
    return out


def gap_edge_runs(gap):
    """the (first, end) pairs the placement gives at `gap`: blobs of three bins, joined where at most `gap` cold bins lie between"""
    out = []
    for lo, _ in edge_blobs():
        if out and lo - out[-1][1] <= gap:
            out[-1][1] = lo + 3
        else:
            out.append([lo, lo + 3])
    return [tuple(r) for r in out]


@functools.lru_cache(maxsize=None)
def gap_edges(N, is_real, nframes, seed=9):
    assert bins_of(N, is_real) == EDGE_BINS
    return _raw(N, is_real, nframes, seed, EDGE_SIGMA, tuple((lo + 1, amp) for lo, amp in edge_blobs()))


DECAY_FRAMES, DECAY_BATCHES, DECAY_AMP, DECAY_STEP = 40, (1, 7, 3, 5, 2, 8, 4, 6, 1, 3), 0.004, 16
DECAY_SHIFTS = (8, 1)


def decay_comb(N):
    return tuple(range(8, N, DECAY_STEP))


def decay_on(nframes):
    """the frames that hold the comb whole"""
    return nframes // 3


@functools.lru_cache(maxsize=None)
def decay(N, nframes, seed=13):
    assert sum(DECAY_BATCHES) == DECAY_FRAMES
    return _raw(N, False, nframes, seed, EDGE_SIGMA, tuple((c, DECAY_AMP) for c in decay_comb(N)), stop=(decay_on(nframes) + 1) * (N // 2))


def fallen(before, after):
    """bins whose trace fell by more than 2^8 of its steps (one count) between two states"""
    return int(np.count_nonzero(np.asarray(before, np.int64) - np.asarray(after, np.int64) > 1 << 8))


# ---- coverage ---------------------------------------------------------------------------------------------------------------------
COUNTERS = ("runs", "over_cap", "cap_inside_word", "multi_run_words", "single_run_words", "cold_words_inside", "tied_peaks", "cold_eq_gap",
            "cold_eq_gap1", "stretch_border_runs", "zero_runs")


def cover(s, threshold, gap, per, runs=None):
    """what one evaluation of trace s exercises; per: the mask words a k_scan_mark thread owns; runs: scan_model.runs' of the same
    evaluation where the caller has them already"""
    s = np.asarray(s, np.int64)
    n, W = len(s), len(s) // 64
    F = M.floors(M.quartiles(s))
    runs = M.runs(s, threshold, gap)[1] if runs is None else runs
    hot = M.hot_bins(s, F, threshold)
    first, end = runs["first"].astype(np.int64), runs["end"].astype(np.int64)
    c = dict.fromkeys(COUNTERS, 0)
    c["runs"], c["over_cap"], c["zero_runs"] = len(runs), len(runs) > M.CAP, len(runs) == 0
    idx = np.flatnonzero(hot)
    cold = np.diff(idx) - 1
    c["cold_eq_gap"], c["cold_eq_gap1"] = int(np.count_nonzero(cold == gap)), int(np.count_nonzero(cold == gap + 1))
    if not len(runs):
        return c
    if len(runs) > M.CAP:  # the first dropped run starts in a word that also holds the start of a kept one
        c["cap_inside_word"] = bool(first[M.CAP] >> 6 == first[M.CAP - 1] >> 6)
    # the run of every bin, -1 outside
    step = np.zeros(n + 1, np.int64)
    step[first] += 1
    step[end] -= 1
    inside = np.cumsum(step[:n]) > 0
    rid = np.where(inside, np.cumsum(np.bincount(first, minlength=n)) - 1, -1).reshape(W, 64)
    inw = inside.reshape(W, 64)
    lo, hi = np.where(inw, rid, len(runs)).min(axis=1), rid.max(axis=1)
    c["multi_run_words"] = int(np.count_nonzero(hi > lo))
    c["single_run_words"] = int(np.count_nonzero((inw.sum(axis=1) >= 2) & (hi == lo)))
    c["cold_words_inside"] = int(np.count_nonzero(~hot.reshape(W, 64).any(axis=1) & inw.any(axis=1)))
    # bins that hold their run's maximum
    edges = np.stack([first, end], axis=1).reshape(-1)
    top = np.maximum.reduceat(np.append(s, 0), edges)[::2]
    at_top = np.zeros(n + 1, np.int64)
    at_top[:n] = inside & (s == top[np.maximum(rid.reshape(-1), 0)])
    c["tied_peaks"] = int(np.count_nonzero(np.add.reduceat(at_top, edges)[::2] >= 2))
    fw, lw = first >> 6, (end - 1) >> 6
    c["stretch_border_runs"] = int(np.count_nonzero((fw % per == per - 1) & (lw // per > fw // per)))
    return c


def noise_rules(n, a=0):
    """the counters the noise masks of an n-bin level must reach in at least one (threshold, gap) of the sweep, in a trace of
    avg_shift a: the ties are the matter of a = 0, where the trace is whole counts; two smoothing steps leave 1/64 count"""
    need = ["multi_run_words", "single_run_words", "cold_eq_gap", "cold_eq_gap1", "zero_runs"] + (["tied_peaks"] if a == 0 else [])
    if words_per_thread(n) > 1:
        need.append("stretch_border_runs")
    if n // 2 > M.CAP:  # room for more than CAP runs
        need += ["over_cap", "cap_inside_word"]
    return need


def broken_rules(n, covers, a=0):
    """covers: {(threshold, gap): cover()} over the whole sweep -> the conditions that do not hold"""
    bad = [k for k in noise_rules(n, a) if not any(c[k] for c in covers.values())]
    bad += [f"runs at threshold 255, gap {g}" for (t, g), c in covers.items() if t == 255 and not c["zero_runs"]]
    bad += [f"{t, g} missing" for t in THRESHOLDS for g in GAPS if (t, g) not in covers]
    return bad


def sweep():
    return [(t, g) for t in THRESHOLDS for g in GAPS]

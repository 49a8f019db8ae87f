// scanplan.h - the band scan (include/psdr.h: psdr_scan_set, psdr_scan_batch, psdr_read_signals), everything of it that is not a
// launch: the ONE definition of every step of the rule (the kernels of scan.hip and the host tests run this text), the validation
// of psdr_scan_set with its texts, the run rule, the launch plan and the host's side of a read.  Plain C++17 (no HIP):
// tests/test_scan_host.py builds it with the host compiler.
//
// The rule (include/psdr.h has it in words), in the order the device runs it.  n = R >> level bins, u = q + 128 of a frame's int8 q:
//   trace     the first frame of a run of frames: s = u << 8 (scan_first); later frames, in frame order:
//             s += ((int)(u << 8) - (int)s) >> a, an arithmetic shift (scan_step).  s <= 255 * 256 always: stored as uint16
//   quartile  Q_g = the 63rd smallest (0-based) of the 256 trace values of segment g: a 16-round radix select (scan_select)
//   floor     F_g = min(Q_{g-1}, Q_g, Q_{g+1}) over the neighbours that exist (scan_floor)
//   hot       hot[j] = s[j] >= F_{j >> 8} + (threshold << 8) (scan_hot), kept as a bit mask in 64-bit words, bit j & 63 of word j >> 6
//   starts    hot bin j starts a run if no bin of [j - gap - 1, j - 1] is hot: word w's starts from words w, w - 1 and w - 2
//             (scan_start_word; gap + 1 <= 65 bins reach one bit into the word before the last)
//   index     base[w] = the starts in the words before w; a bin inside a run belongs to run base[w] + (starts of w at or below
//             its bit) - 1 (scan_run_index)
//   inside    a hot bin, or a cold one whose cold stretch - the bins between the nearest hot bin below and the nearest above,
//             both must exist - is at most gap long (scan_inside; the distances come from scan_dist_below / scan_dist_above)
//   ends      hot bin j ends its run, end = j + 1, if no bin of [j + 1, j + 1 + gap] is hot (scan_is_end)
//   peak      the unsigned 64-bit maximum of (s << 32) | (0xFFFFFFFF - j) over the run's bins (scan_key): the largest s, the
//             lowest bin among equals.  The maximum does not depend on the order it is taken in
//   list      entry r < SCAN_CAP of the device's list is {first, end, key}; runs past the cap are counted (the total is the number
//             of starts) and dropped.  scan_record() makes the psdr_signal of an entry on the host: the peak out of the key, the
//             floor out of the floors
// Everything is integer arithmetic: the host and the device cannot differ by a rounding.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/psdr.h"

#ifndef PSDR_HOST_DEVICE
#if defined(__HIPCC__)
#define PSDR_HOST_DEVICE __host__ __device__
#else
#define PSDR_HOST_DEVICE
#endif
#endif

namespace psdr {

constexpr int SCAN_SEG = 256;                    // bins of a segment
constexpr int SCAN_RANK = 63;                    // the quartile: the 63rd smallest (0-based) of 256, (256 - 1) / 4 as in noiseplan.h
constexpr int SCAN_CAP = PSDR_SCAN_MAX_SIGNALS;  // runs the list holds
constexpr int SCAN_MIN_BINS = 256, SCAN_SHIFT_MAX = 8, SCAN_THR_MIN = 1, SCAN_THR_MAX = 255, SCAN_GAP_MAX = 64;
constexpr int SCAN_FAR = 1 << 20;                // "no hot bin within reach" as a distance

// One entry of the device's list
struct ScanRun {
    uint32_t first, end;
    uint64_t key;
};
// ... and the list's head: the untruncated number of runs
struct ScanHead {
    uint32_t total, pad[3];
};
static_assert(sizeof(ScanRun) == 16 && sizeof(ScanHead) == 16 && sizeof(psdr_signal) == 20, "the device tables' layout");

// ---- the trace --------------------------------------------------------------------------------------------------------------
PSDR_HOST_DEVICE inline uint32_t scan_u(int q) { return (uint32_t)(q + 128); }
PSDR_HOST_DEVICE inline uint32_t scan_first(uint32_t u) { return u << 8; }
PSDR_HOST_DEVICE inline uint32_t scan_step(uint32_t s, uint32_t u, int a) {
    const int d = (int)(u << 8) - (int)s;
    return s + (uint32_t)(d >> a);  // (>> of a negative int: arithmetic on every compiler this builds with; the tests pin it)
}

// ---- the floor --------------------------------------------------------------------------------------------------------------
// The k-th smallest (0-based) of a set of values below 2^16, by a radix select from bit 15 down (noiseplan.h: noise_select):
// count(prefix, mask) says how many values x of the set have (x & mask) == prefix
template <class Count>
PSDR_HOST_DEVICE inline uint32_t scan_select(int k, Count count) {
    uint32_t prefix = 0;
    for (int b = 15; b >= 0; b--) {
        const int zeros = count(prefix, (0xFFFFu << b) & 0xFFFFu);
        if (k >= zeros) k -= zeros, prefix |= 1u << b;
    }
    return prefix;
}
inline uint32_t scan_quartile_host(const uint16_t *s) {
    return scan_select(SCAN_RANK, [&](uint32_t prefix, uint32_t mask) {
        int c = 0;
        for (int t = 0; t < SCAN_SEG; t++) c += ((uint32_t)s[t] & mask) == prefix;
        return c;
    });
}
PSDR_HOST_DEVICE inline uint32_t scan_floor(const uint32_t *Q, int g, int G) {
    uint32_t f = Q[g];
    if (g > 0 && Q[g - 1] < f) f = Q[g - 1];
    if (g + 1 < G && Q[g + 1] < f) f = Q[g + 1];
    return f;
}
PSDR_HOST_DEVICE inline bool scan_hot(uint32_t s, uint32_t F, int threshold) { return s >= F + ((uint32_t)threshold << 8); }

// ---- runs of bins -----------------------------------------------------------------------------------------------------------
// word w of the mask moved up by d bins, d in 1..65: bit b is bin 64 w + b - d.  p, pp: words w - 1, w - 2
PSDR_HOST_DEVICE inline uint64_t scan_up(uint64_t cur, uint64_t p, uint64_t pp, int d) {
    if (d < 64) return (cur << d) | (p >> (64 - d));
    if (d == 64) return p;
    return (p << 1) | (pp >> 63);
}
// the starts of word w
PSDR_HOST_DEVICE inline uint64_t scan_start_word(uint64_t cur, uint64_t p, uint64_t pp, int gap) {
    uint64_t near = 0;  // bins with a hot bin among the gap + 1 below them
    for (int d = 1; d <= gap + 1; d++) near |= scan_up(cur, p, pp, d);
    return cur & ~near;
}
PSDR_HOST_DEVICE inline int scan_clz64(uint64_t v) {  // (v != 0)
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)v);
#else
    return __builtin_clzll(v);
#endif
}
PSDR_HOST_DEVICE inline int scan_ctz64(uint64_t v) {  // (v != 0)
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)v) - 1;
#else
    return __builtin_ctzll(v);
#endif
}
PSDR_HOST_DEVICE inline int scan_popc64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}
// the distance from bit b of word w down to the nearest hot bin below it (1: the bin next to it), SCAN_FAR if words w, w - 1 and
// w - 2 hold none
PSDR_HOST_DEVICE inline int scan_dist_below(int b, uint64_t cur, uint64_t p, uint64_t pp) {
    const uint64_t low = b ? cur & (~0ull >> (64 - b)) : 0;
    if (low) return b - (63 - scan_clz64(low));
    if (p) return b + 1 + scan_clz64(p);
    if (pp) return b + 65 + scan_clz64(pp);
    return SCAN_FAR;
}
// ... and up to the nearest hot bin above it.  nx, nnx: words w + 1, w + 2
PSDR_HOST_DEVICE inline int scan_dist_above(int b, uint64_t cur, uint64_t nx, uint64_t nnx) {
    const uint64_t high = b < 63 ? cur & (~0ull << (b + 1)) : 0;
    if (high) return scan_ctz64(high) - b;
    if (nx) return 64 - b + scan_ctz64(nx);
    if (nnx) return 128 - b + scan_ctz64(nnx);
    return SCAN_FAR;
}
PSDR_HOST_DEVICE inline bool scan_inside(bool hot, int below, int above, int gap) { return hot || below + above - 1 <= gap; }
PSDR_HOST_DEVICE inline bool scan_is_end(bool hot, int above, int gap) { return hot && above > gap + 1; }
// the run of a bin inside one: starts = word w's, b its bit
PSDR_HOST_DEVICE inline uint32_t scan_run_index(uint32_t base, uint64_t starts, int b) {
    return base + (uint32_t)scan_popc64(starts & (~0ull >> (63 - b))) - 1u;
}
PSDR_HOST_DEVICE inline uint64_t scan_key(uint32_t s, uint32_t j) { return ((uint64_t)s << 32) | (uint64_t)(0xFFFFFFFFu - j); }
// an entry of the list as the caller sees it
inline psdr_signal scan_record(const ScanRun &r, const uint32_t *F) {
    psdr_signal o;
    o.first = r.first, o.end = r.end;
    o.peak_bin = 0xFFFFFFFFu - (uint32_t)r.key;
    o.peak = (uint32_t)(r.key >> 32);
    o.floor = F[o.peak_bin >> 8];
    return o;
}
// psdr_read_signals: the entries at least min_width wide, the first `cap` of them to out (may be null); returns how many passed
inline int scan_filter(const ScanRun *list, int kept, const uint32_t *F, int min_width, psdr_signal *out, int cap) {
    int n = 0;
    for (int i = 0; i < kept; i++) {
        if ((int64_t)list[i].end - (int64_t)list[i].first < (int64_t)min_width) continue;
        if (out && n < cap) out[n] = scan_record(list[i], F);
        n++;
    }
    return n;
}
inline int scan_kept(uint32_t total) { return total < (uint32_t)SCAN_CAP ? (int)total : SCAN_CAP; }

// ---- the whole rule on the host, step by step as the kernels run it ----------------------------------------------------------
// frames[f][j]: the int8 values of the level; fresh: the first frame starts the trace
inline void scan_trace_host(uint16_t *s, size_t n, const int8_t *const *frames, int nframes, bool fresh, int a) {
    for (size_t j = 0; j < n; j++) {
        uint32_t v = s[j];
        for (int f = 0; f < nframes; f++) {
            const uint32_t u = scan_u(frames[f][j]);
            v = fresh && f == 0 ? scan_first(u) : scan_step(v, u, a);
        }
        s[j] = (uint16_t)v;
    }
}
struct ScanEval {
    std::vector<uint32_t> Q, F;
    std::vector<uint64_t> hot, starts;
    std::vector<uint32_t> base;
    std::vector<ScanRun> list;  // scan_kept(total) entries
    uint32_t total = 0;
};
inline ScanEval scan_evaluate_host(const uint16_t *s, size_t n, int threshold, int gap) {
    ScanEval e;
    const int G = (int)(n / SCAN_SEG);
    const size_t W = n / 64;
    e.Q.resize(G), e.F.resize(G);
    for (int g = 0; g < G; g++) e.Q[g] = scan_quartile_host(s + (size_t)g * SCAN_SEG);
    for (int g = 0; g < G; g++) e.F[g] = scan_floor(e.Q.data(), g, G);
    e.hot.assign(W, 0), e.starts.assign(W, 0), e.base.assign(W, 0);
    for (size_t j = 0; j < n; j++)
        if (scan_hot(s[j], e.F[j >> 8], threshold)) e.hot[j >> 6] |= 1ull << (j & 63);
    auto word = [&](size_t w, long o) { return (long)w + o < 0 || (size_t)((long)w + o) >= W ? 0ull : e.hot[(size_t)((long)w + o)]; };
    for (size_t w = 0; w < W; w++) {
        e.starts[w] = scan_start_word(word(w, 0), word(w, -1), word(w, -2), gap);
        e.base[w] = e.total;
        e.total += (uint32_t)scan_popc64(e.starts[w]);
    }
    e.list.assign((size_t)scan_kept(e.total), ScanRun{0, 0, 0});
    for (size_t j = 0; j < n; j++) {
        const size_t w = j >> 6;
        const int b = (int)(j & 63);
        const bool hot = (e.hot[w] >> b) & 1;
        const int below = scan_dist_below(b, word(w, 0), word(w, -1), word(w, -2)), above = scan_dist_above(b, word(w, 0), word(w, 1), word(w, 2));
        if (!scan_inside(hot, below, above, gap)) continue;
        const uint32_t r = scan_run_index(e.base[w], e.starts[w], b);
        if (r >= (uint32_t)SCAN_CAP) continue;
        if ((e.starts[w] >> b) & 1) e.list[r].first = (uint32_t)j;
        if (scan_is_end(hot, above, gap)) e.list[r].end = (uint32_t)j + 1;
        const uint64_t k = scan_key(s[j], (uint32_t)j);
        if (k > e.list[r].key) e.list[r].key = k;
    }
    return e;
}

// ---- the call ---------------------------------------------------------------------------------------------------------------
// psdr_scan_set's refusals, in the order they are looked for
enum ScanVerdict { SCAN_OK, SCAN_BAD_LEVEL, SCAN_TOO_FEW_BINS, SCAN_BAD_SHIFT, SCAN_BAD_THRESHOLD, SCAN_BAD_GAP };
inline ScanVerdict scan_check(size_t R, int levels, const psdr_scan_config &c) {
    if (c.level < 0 || c.level >= levels) return SCAN_BAD_LEVEL;
    if ((R >> c.level) < (size_t)SCAN_MIN_BINS) return SCAN_TOO_FEW_BINS;
    if (c.avg_shift < 0 || c.avg_shift > SCAN_SHIFT_MAX) return SCAN_BAD_SHIFT;
    if (c.threshold < SCAN_THR_MIN || c.threshold > SCAN_THR_MAX) return SCAN_BAD_THRESHOLD;
    if (c.gap < 0 || c.gap > SCAN_GAP_MAX) return SCAN_BAD_GAP;
    return SCAN_OK;
}
inline std::string scan_text(ScanVerdict v, size_t R, int levels, const psdr_scan_config &c) {
    switch (v) {
    case SCAN_BAD_LEVEL: return "scan level " + std::to_string(c.level) + " outside [0, " + std::to_string(levels) + ")";
    case SCAN_TOO_FEW_BINS:
        return "scan level " + std::to_string(c.level) + " has " + std::to_string(R >> c.level) + " bins, fewer than one segment of " +
               std::to_string(SCAN_MIN_BINS);
    case SCAN_BAD_SHIFT: return "scan avg_shift " + std::to_string(c.avg_shift) + " outside [0, " + std::to_string(SCAN_SHIFT_MAX) + "]";
    case SCAN_BAD_THRESHOLD:
        return "scan threshold " + std::to_string(c.threshold) + " outside [" + std::to_string(SCAN_THR_MIN) + ", " + std::to_string(SCAN_THR_MAX) + "] counts";
    case SCAN_BAD_GAP: return "scan gap " + std::to_string(c.gap) + " outside [0, " + std::to_string(SCAN_GAP_MAX) + "] bins";
    default: return "";
    }
}

// ---- runs of frames ---------------------------------------------------------------------------------------------------------
// What the context keeps between psdr_scan_batch calls.  psdr_scan_set: run = false, evaluated = false
struct ScanState {
    bool run = false;        // the trace belongs to a run ...
    uint64_t next = 0;       // ... that the call with this first_frame_num continues
    bool evaluated = false;  // the read calls have something to deliver
    uint64_t last_frame = 0; // the number of the last frame in the trace
};
struct ScanStep {
    bool fresh;        // the batch's first frame starts the trace
    ScanState after;   // the state once everything is enqueued
};
inline ScanStep scan_step_plan(const ScanState &st, uint64_t first_frame_num, int nframes) {
    ScanStep p;
    p.fresh = !(st.run && first_frame_num == st.next);
    p.after.run = true;
    p.after.next = first_frame_num + (uint64_t)nframes;
    p.after.evaluated = true;
    p.after.last_frame = first_frame_num + (uint64_t)nframes - 1;
    return p;
}

// ---- the launches -----------------------------------------------------------------------------------------------------------
// Which form k_scan_trace takes and how large the five grids are.  Levels at or below tiled_lt live in the tiled records
// (quantize.h): `per` = tile_ch >> level values of the level side by side per record, one lane per record; the others in the
// level-major buffer at byte qoff, 16 values per lane (n and every level's offset are multiples of 256)
struct ScanFacts {
    size_t R = 0;
    int levels = 0, tiled_lt = -1, tile_ch = 16;
};
struct ScanLaunch {
    size_t n = 0;       // bins
    int G = 0;          // segments
    size_t words = 0;   // mask words
    bool tiled = false;
    int per = 16;       // values per lane of k_scan_trace
    int loff = 0;       // tiled: the level's byte offset inside a record
    size_t qoff = 0;    // level-major: the level's byte offset inside a frame
    unsigned trace_blocks = 0, floor_blocks = 0, hot_blocks = 0, emit_blocks = 0;  // 256 threads each; k_scan_mark is one work-group
};
inline ScanLaunch scan_launch(const ScanFacts &f, int level) {
    ScanLaunch l;
    l.n = f.R >> level;
    l.G = (int)(l.n / SCAN_SEG);
    l.words = l.n / 64;
    l.tiled = level <= f.tiled_lt;
    if (l.tiled) {
        l.per = f.tile_ch >> level;
        l.loff = level == 0 ? 0 : 2 * f.tile_ch - (2 * f.tile_ch >> level);  // quantize.h: tiled_level_offset
    } else {
        l.per = 16;
        for (int t = 0; t < level; t++) l.qoff += f.R >> t;
    }
    const size_t lanes = l.n / (size_t)l.per;
    l.trace_blocks = (unsigned)((lanes + 255) / 256);
    l.floor_blocks = (unsigned)((l.G + 3) / 4);       // a wave per segment
    l.hot_blocks = (unsigned)((l.words + 3) / 4);     // a wave per mask word
    l.emit_blocks = l.hot_blocks;
    return l;
}
// what the first psdr_scan_set(on) allocates, sized for level 0: trace, mask (+ the start words), quartiles and floors, list, scratch
inline size_t scan_bytes(size_t R) { return R * 2 + 2 * (R / 64) * 8 + 2 * (R / SCAN_SEG) * 4 + (size_t)SCAN_CAP * sizeof(ScanRun) + (R / 64) * 4 + sizeof(ScanHead); }

}  // namespace psdr

// forwardplan.h - what the forward path decides on the host, resolved in pure functions of a few facts: the chain segments
// of the fused real second pass (which batches hand off, the table k_fft_pass2_real walks, what the seam buffers must
// hold), the pyramid levels above the tile (which kernel takes which level from which scratch buffer) and the waterfall
// batch (who is sent what, where, and what becomes of the detectors' carry).  Plain host C++17 (no HIP): forward.hip
// enqueues from the plans, tests/test_forward_plan.py prints them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/psdr.h"
#include "types.h"

namespace psdr {

// ---- chain segments of the fused real second pass (k_fft_pass2_real, fft_pass.h) ----------------------------------------
// Two forms:
//  * uniform segments of seg_len() tiles, frame-major, every segment's first tile WITHOUT a carry-in (it leaves its
//    partial octets in seamP, k_real_seam completes them): small batches, PSDR_SEG_LEN, static tile hand-out;
//  * hand-off (batches of more than one frame per work-group - seg_handoff): a frame is cut into segments of G/4, G/4, G/4, G/8, ... 2,
//    1, 1 tiles from the top, handed out LEVEL-major - all frames' top segments first, then all second segments, ... - by
//    the ticket counter alone.  Only the top segment of a frame has no carry-in (the ring closes through tile 0's row
//    M1/2: one seam per frame, as with whole-frame segments); every other segment reads the carried row its predecessor -
//    handed out nframes tickets earlier, i.e. finished about a round of segments ago - left in seamC behind its flag.
//    What it buys: the work-groups of a launch differ by +-3.5 % in speed (the even XCDs are ~3 % slower: tools/trace_real.py),
//    and with two whole-frame segments each nothing balanced that - the launch ended with its slowest work-group, 3.4 %
//    after the median one.  With tickets and segments that shrink to single tiles the spread at the end is one tile, at
//    a cost of 8 KiB of traffic per hand-off (a seam: 92 KiB and a record written twice).
struct SegFacts {
    int G = 0;            // tiles of a frame (M1 / T2)
    int num_cus = 256;
    int seg_len_env = 0;  // PSDR_SEG_LEN (0: unset)
};
// a table entry as the kernels read it (a uint4; ctx.h ties the size): x frame, y first tile | tiles << 16, z the segment
// above, w flags
struct SegEntry {
    unsigned x, y, z, w;
};
constexpr unsigned SEG_CARRY_MEM = 1;  // w: the first tile's carry-in comes through memory (fft_pass.h PSDR_SEG_CARRY_MEM)

// Tiles of one frame a work-group walks in a chain: long chains carry the mirror-side octets in LDS
// (nothing extra in HBM), short chains give the persistent grid enough independent segments.  Aim
// for about two segments per work-group: the pass is bound by memory, not by balance (256 frames of
// 2^21 points, same box: 1012-1023 us with 16 segments per work-group, 990-1030 with 8, 4 or 2), and
// every segment costs one seam (k_real_seam: 177 / 89 / 52 / 31 us at 4 / 8 / 16 / 32 tiles per segment,
// run beside the next batch's pass 1, which it slows).
inline int seg_len(const SegFacts &s, int nframes) {
    const int G = s.G;
    if (s.seg_len_env > 0) {
        int sl = 1;
        while (sl * 2 <= s.seg_len_env && sl * 2 <= G) sl *= 2;
        return sl;
    }
    const int W = std::max(s.num_cus, 1);
    const long long tiles = (long long)G * nframes;  // of the batch
    const long long want = tiles / (2LL * W);
    // What the measurements say (cfg3's stream, tools/ab_small_batches.sh, profiles/r04b_uniform_segments_small_batches.jsonl):
    // up to 16 tiles per work-group ONE static segment each, rounded up to a power of two (32 frames: 256 segments of 8
    // tiles 151 GS/s, 512 of 4 - the old choice - 140; 48 frames: 192 of 16 tiles 155, 768 of 4 141); two static segments per
    // work-group when that comes out even (128, 256 frames of 2^21 points: nothing to balance, nothing drawn); else five
    // to ten segments per work-group, so that the ticket counter has something to balance with - a work-group draws two
    // tickets ahead, and with three or four segments each half the chip ends up with one more than the other half (192
    // frames: 16-tile segments 158 GS/s, 8-tile segments 168; 384 frames: 162 / 182).
    const long long per_wg = (tiles + W - 1) / W;
    if (per_wg <= 16) {
        int sl = 1;
        while (sl < per_wg && sl * 2 <= G) sl *= 2;
        return sl;
    }
    if (2LL * W * want == tiles && (want & (want - 1)) == 0 && want <= G) return (int)want;
    const long long v = tiles / (5LL * W);
    int sl = 1;
    while (sl * 2 <= v && sl * 2 <= G) sl *= 2;
    return sl;
}
// (PSDR_SEG_LEN=n is the way back to uniform segments)
// Which batches take the hand-off plan: those of more than one frame per work-group (cfg3's stream at 258 / 288 / 320 /
// 384 / 448 / 512 frames: +11 / +29 / +25 / +12 / +6 / +1.5 % over the uniform segments of round 3; against the uniform
// segments seg_len() picks now it is level at 320 and 384 frames and 1 - 5 % ahead at 512).  Up to one frame per
// work-group a segment's predecessor is less than a segment ahead, most hand-offs end as seams, and well-chosen uniform
// segments are 3 - 9 % faster (profiles/r04b_handoff_vs_uniform_by_batch.jsonl, r04b_uniform_segments_small_batches.jsonl).
inline bool seg_handoff(const SegFacts &s, int nframes) {
    return s.seg_len_env <= 0 && s.G >= 16 && nframes >= std::max(s.num_cus, 1) + 1;
}
// hand-off: tiles per segment from the top of a frame: G/4, G/4, G/4, G/8, ... 2, 1, 1; returns how many (log2 G + 2)
constexpr int SEG_LEVELS_MAX = 34;
inline int seg_handoff_lens(int G, int lens[SEG_LEVELS_MAX]) {
    int n = 0;
    lens[n++] = G / 4, lens[n++] = G / 4, lens[n++] = G / 4;
    for (int l = G / 8; l >= 1; l >>= 1) lens[n++] = l;
    lens[n++] = 1;
    return n;
}
// segments of a batch: table entries, seams k_real_seam may have to close (in hand-off mode any segment may fall back to
// one), carried rows and flags
inline unsigned seg_count(const SegFacts &s, int nframes) {
    if (seg_handoff(s, nframes)) {
        int lens[SEG_LEVELS_MAX];
        return (unsigned)(seg_handoff_lens(s.G, lens) * nframes);
    }
    return (unsigned)(nframes * (s.G / seg_len(s, nframes)));
}
// what the seam buffers and the flags must hold for every batch size up to max_batch
inline unsigned seg_cap(const SegFacts &s, int max_batch) {
    unsigned cap = 0;
    for (int nf = 1; nf <= max_batch; nf++) cap = std::max(cap, seg_count(s, nf));
    return cap;
}
// out[seg_count(s, nframes)]
inline void seg_table(const SegFacts &s, int nframes, SegEntry *out) {
    const int G = s.G;
    if (seg_handoff(s, nframes)) {
        int lens[SEG_LEVELS_MAX];
        const int levels = seg_handoff_lens(G, lens);
        // Level-major, frames in order: a segment's predecessor - the same frame one level up - is handed out nframes >=
        // 2 * grid indices earlier, i.e. about two segments of every work-group earlier.
        int g = G - 1;
        for (int lv = 0; lv < levels; lv++) {
            for (int f = 0; f < nframes; f++) {
                const unsigned above = (unsigned)((lv ? lv - 1 : levels - 1) * nframes + f);  // (the top segment's: the bottom one)
                out[(size_t)lv * nframes + f] = SegEntry{(unsigned)f, (unsigned)g | ((unsigned)lens[lv] << 16), above, lv ? SEG_CARRY_MEM : 0u};
            }
            g -= lens[lv];
        }
        return;
    }
    const int SL = seg_len(s, nframes), S = G / SL;
    for (int f = 0; f < nframes; f++)
        for (int si = 0; si < S; si++)
            out[(size_t)f * S + si] = SegEntry{(unsigned)f, (unsigned)((si + 1) * SL - 1) | ((unsigned)SL << 16), (unsigned)(f * S + (si + 1) % S), 0u};
}

// ---- the pyramid levels above the tile --------------------------------------------------------------------------------
// Pass 2 (or k_untangle_real) leaves the sums of level LT in scratch buffer 0.  Tile-major sums of a fused pass 2 (rows of
// 1024 outputs): one thread per output row takes the levels inside a row (k_col_tail), the generic kernel
// (k_pyramid_tail, seven levels a launch) the few above; every step reads one scratch buffer and leaves the sums of its
// last level in the other.
struct TailFacts {
    size_t R = 0;
    int levels = 0, LT = 0, log2M2 = 0, M2 = 0;
    bool real_fused = false;
    int mapped = 0, l2gpt = 0, pair = 0;  // RecMap (quantize.h)
};
enum TailKind { TAIL_COL_64, TAIL_COL_128, TAIL_COL_256, TAIL_COL_256_PAIRED, TAIL_GENERIC };
struct TailStep {
    TailKind kind = TAIL_GENERIC;
    int lvl_in = 0;     // the level whose sums it reads; it produces the levels above, up to lvl_in + log2(groups per row) / + 7
    size_t len_in = 0;  // sums of that level per frame
    int src = 0, dst = 1;  // scratch buffers
    bool mapped = false;   // its input is still in RecMap order (only pass 2's own output is tile-major)
};
// (levels <= 23 and LT >= 2: at most 21 levels to produce, at least six a step)
constexpr int TAIL_STEPS_MAX = 4;
struct TailPlan {
    int n = 0;
    TailStep step[TAIL_STEPS_MAX];
};
inline TailPlan tails_plan(const TailFacts &f) {
    TailPlan p;
    int lvl = f.LT;
    size_t len = f.R >> lvl;
    int cur = 0;
    const int ng = (int)(len >> f.log2M2);  // groups per output row
    const bool col_tail = f.mapped && (f.M2 == 1024 || (f.M2 == 2048 && f.real_fused)) && f.l2gpt == 0 && (ng == 64 || ng == 128 || ng == 256);
    if (col_tail && lvl + 1 < f.levels) {
        TailStep &s = p.step[p.n++];
        // (PAIRED: quartet records side by side (2048-point rows): one 8-byte load per (tile, column))
        s.kind = ng == 64 ? TAIL_COL_64 : (ng == 128 ? TAIL_COL_128 : (f.pair ? TAIL_COL_256_PAIRED : TAIL_COL_256));
        s.lvl_in = lvl, s.len_in = len, s.src = 0, s.dst = 1, s.mapped = true;
        for (int g = ng; g > 1; g >>= 1) lvl++;
        len = (size_t)f.M2;
        cur = 1;
    }
    const int lvl_mapped = col_tail ? -1 : f.LT;  // the level whose sums are still in RecMap order
    while (lvl + 1 < f.levels && len >= 2 && p.n < TAIL_STEPS_MAX) {
        TailStep &s = p.step[p.n++];
        s.kind = TAIL_GENERIC;
        s.lvl_in = lvl, s.len_in = len, s.src = cur, s.dst = cur ^ 1, s.mapped = f.mapped && lvl == lvl_mapped;
        lvl += 7;
        len >>= 7;
        cur ^= 1;
    }
    return p;
}

// ---- the waterfall batch (psdr_waterfall_batch) ------------------------------------------------------------------------
struct WfSlot {
    bool active = false;
    int level = 0, l = 0, r = 0;
    int det = PSDR_WF_SAMPLE;  // psdr_waterfall_set_detector
    // the last psdr_waterfall_batch: what was gathered, and with which window (set_range may run
    // on another thread between the batch and psdr_read_waterfall)
    size_t out_off = 0;
    int nsent = 0;
    int b_level = 0, b_l = 0, b_r = 0;
    int b_det = PSDR_WF_SAMPLE;
};
struct WfFacts {
    size_t R = 0;
    int levels = 0;
    int tiled_lt = -1, tile_ch = 16;  // levels 0..tiled_lt live in tiled records of tile_ch channels (quantize.h)
    int skip_num = 1;
};
// The detectors' carry is the reduction of the frames of the current RUN of psdr_waterfall_batch calls that lie behind the
// run's last sent frame - what the next sent row's window holds of earlier batches.
struct WfCarry {
    bool run = false;   // the last psdr_waterfall_batch kept the carry (some client had a detector)
    uint64_t next = 0;  // ... and the first_frame_num that continues it
    int carry_n = 0;    // frames the carry stands for
};
struct WfPlan {
    int nsent = 0;     // frames sent: h_sent[0 .. nsent)
    size_t total = 0;  // bytes of the batch's rows
    int maxid = -1;    // highest active client id
    bool gather = false;                    // there are rows to write
    bool hold = false, any_sample = false;  // an active client with a detector / on PSDR_WF_SAMPLE
    int carry_n = 0;   // frames the carry stands for when the batch starts (0: this call does not continue its run)
    // the carry for the next call: the frames from f0 on - behind the batch's last sent frame - replace it; a batch without a
    // sent frame is reduced onto it (onto nothing, at the start of a run)
    int f0 = 0, accumulate = 0;
    WfCarry after;     // the state once everything is enqueued
};
// Writes the ring slot's host image (h_wf[n], h_sent[<= nframes]) and the slots' snapshot of the batch in place.
inline WfPlan wf_plan(WfSlot *slots, size_t n, const WfFacts &f, const WfCarry &state, uint64_t first_frame_num, int nframes, WfClient *h_wf,
                      int *h_sent) {
    WfPlan p;
    for (int fr = 0; fr < nframes; fr++)
        if ((first_frame_num + (uint64_t)fr) % (uint64_t)f.skip_num == 0) h_sent[p.nsent++] = fr;
    for (size_t i = 0; i < n; i++) {
        WfSlot &s = slots[i];
        WfClient &w = h_wf[i];
        w.active = s.active ? 1 : 0;
        w.level = s.level;
        w.l = s.l;
        w.r = s.r;
        w.qoff = 0;
        for (int t = 0; t < s.level; t++) w.qoff += f.R >> t;
        w.out_off = p.total;
        w.det = s.det;
        // (k_waterfall_hold) tiled records hold ch >> level values of the level side by side, at a multiple of that many
        // bytes; a level-major level starts at qoff and a dword must not reach past its end
        w.vec = s.level <= f.tiled_lt ? ((f.tile_ch >> s.level) >= 4) : ((f.R >> s.level) % 4 == 0 && w.qoff % 4 == 0);
        s.out_off = p.total;
        s.nsent = s.active ? p.nsent : 0;
        s.b_level = s.level;
        s.b_l = s.l;
        s.b_r = s.r;
        s.b_det = s.det;
        if (s.active) {
            p.total += (size_t)p.nsent * (size_t)(s.r - s.l);
            p.total = (p.total + 15) & ~(size_t)15;
            p.maxid = (int)i;
            (s.det != PSDR_WF_SAMPLE ? p.hold : p.any_sample) = true;
        }
    }
    p.gather = p.maxid >= 0 && p.nsent > 0 && p.total > 0;
    // detectors: does this call continue the run the carry belongs to?  (header: psdr_waterfall_batch)
    p.carry_n = p.hold && state.run && first_frame_num == state.next ? state.carry_n : 0;
    p.f0 = p.nsent > 0 ? h_sent[p.nsent - 1] + 1 : 0;
    p.accumulate = p.nsent == 0 && p.carry_n > 0;
    p.after.next = state.next;  // (without a detector: no run, nothing carried)
    if (p.hold) {
        p.after.carry_n = (p.accumulate ? p.carry_n : 0) + (nframes - p.f0);
        p.after.next = first_frame_num + (uint64_t)nframes;
        p.after.run = true;
    }
    return p;
}
// The carry mirrors one frame's records and upper levels (types.h WfHoldArgs): [0, lenA) the tiled records, behind them
// bytes [qB0, qB0 + lenB) of the level-major buffer - the levels above tiled_lt, widened to whole 16-byte pieces.
struct WfCarryLayout {
    bool ok = false;  // false: the record buffers are no whole 16-byte pieces (unsupported)
    size_t lenA = 0, qB0 = 0, lenB = 0;
};
inline WfCarryLayout wf_carry_layout(int tiled_lt, int levels, size_t R, size_t q_len, size_t q_stride, size_t qt_stride) {
    WfCarryLayout l;
    size_t q_up = 0;  // byte offset of level tiled_lt + 1 in the level-major buffer
    for (int t = 0; t <= tiled_lt && t < levels; t++) q_up += R >> t;
    l.lenA = tiled_lt >= 0 ? qt_stride : 0;
    l.qB0 = q_up & ~(size_t)15;
    const size_t qB1 = (q_len + 15) & ~(size_t)15;  // <= q_stride, a multiple of 128
    l.lenB = qB1 > l.qB0 ? qB1 - l.qB0 : 0;
    l.ok = !((l.lenA & 15) || (qt_stride & 15) || qB1 > q_stride);
    return l;
}

}  // namespace psdr

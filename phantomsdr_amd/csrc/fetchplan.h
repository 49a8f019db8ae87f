// fetchplan.h - what the served end of the path decides on the host, resolved in pure functions of a few facts: which slots
// a fetch's IQ, carrier and squelch copies span, how many bytes of waterfall rows it moves, the ordered list of its copies
// (which buffer, from where, plain or pitched, on which copy stream, which event behind it), the ring of host sets, and
// whose rows a slot of a fetched set holds.  Plain host C++17 (no HIP): fetch.hip validates, snapshots, allocates and
// enqueues from the plan, tests/test_fetch_plan.py prints it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/psdr.h"
#include "forwardplan.h"

namespace psdr {

// ---- facts ---------------------------------------------------------------------------------------------------------------
struct FetchFacts {
    unsigned what = 0;     // PSDR_FETCH_* bits
    size_t S = 0, mb = 0;  // audio slots, max_batch
    size_t F = 0, h = 0;   // frames of the last demodulation batch, n / 2
    bool pcm16 = false;    // the chain's PCM rows are int16 (PSDR_OPT_POST_CHAIN_PCM16 at that batch)
};
// an audio slot at the time of the fetch (the waterfall slots: WfSlot, forwardplan.h - active, nsent, out_off, b_l, b_r)
struct FetchSlot {
    bool active = false, in_batch = false;  // in_batch: part of the last demodulation batch
    int mode = PSDR_USB;                    // ... demodulated as
    bool sq_on = false;                     // ... with squelch
};
inline bool fetch_wants_audio(unsigned what) { return (what & (PSDR_FETCH_AUDIO | PSDR_FETCH_PCM | PSDR_FETCH_IQ)) != 0; }

// ---- spans -----------------------------------------------------------------------------------------------------------------
// Rows that only some slots have - IQ rows, carrier records, squelch flags - travel in ONE copy from the lowest to the highest
// slot of the batch that has them: the IQ rows with PSDR_FETCH_IQ, the other two with any of the audio bits.
enum FetchSpanKind { SPAN_IQ, SPAN_CAR, SPAN_SQ, SPAN_COUNT };
struct FetchSpan {
    int lo = 0, n = 0;  // (nobody: 0, 0)
    bool holds(int id) const { return id >= lo && id < lo + n; }
};
inline bool fetch_in_span(unsigned what, const FetchSlot &s, FetchSpanKind k) {
    if (!s.active || !s.in_batch) return false;
    if (k == SPAN_IQ) return (what & PSDR_FETCH_IQ) && s.mode == PSDR_IQ;
    return fetch_wants_audio(what) && (k == SPAN_CAR ? s.mode == PSDR_SAM : s.sq_on);
}
inline FetchSpan span_of(unsigned what, const FetchSlot *slots, size_t S, FetchSpanKind k) {
    int lo = (int)S, hi = -1;
    for (size_t i = 0; i < S; i++)
        if (fetch_in_span(what, slots[i], k)) {
            lo = std::min(lo, (int)i);
            hi = (int)i;
        }
    return hi < 0 ? FetchSpan{0, 0} : FetchSpan{lo, hi - lo + 1};
}
// the bytes of d_wfout the batch's rows reach to: the end of the client that reaches furthest, in whole 16-byte pieces
inline size_t wf_bytes(unsigned what, const WfSlot *slots, size_t n) {
    size_t bytes = 0;
    if (what & PSDR_FETCH_WATERFALL)
        for (size_t i = 0; i < n; i++) {
            const WfSlot &w = slots[i];
            if (w.active && w.nsent > 0) bytes = std::max(bytes, (w.out_off + (size_t)w.nsent * (size_t)(w.b_r - w.b_l) + 15) & ~(size_t)15);
        }
    return bytes;
}

// ---- the copies ------------------------------------------------------------------------------------------------------------
enum FetchBuf { FB_WF, FB_PWR, FB_NAN, FB_AUDIO, FB_IQ, FB_CAR, FB_SQ, FB_PCM, FB_COUNT };
enum FetchEvent { FE_NONE, FE_WF, FE_AUDIO, FE_PCM };  // (`done` follows the first stream's last copy in every fetch)
// Rows [slot][0..F) of a device array [slot][max_batch][row]: ONE plain copy of rows * pitch bytes when the batch fills
// max_batch (the DMA engines' case; a pitched copy may be done by a copy kernel on the CUs the passes are using), else one
// pitched copy of `rows` pieces of `width` bytes.  Either way rows * width bytes that matter, to the start of the host buffer.
struct FetchCopy {
    FetchBuf buf = FB_WF;
    size_t src_off = 0;  // elements of the device buffer
    size_t width = 0, pitch = 0, rows = 0;
    bool pitched = false;
    int stream = 0;      // 0: the copy stream, 1: the PCM's own
    FetchEvent after = FE_NONE;
    size_t bytes() const { return rows * width; }
};
constexpr int FETCH_COPIES_MAX = FB_COUNT;
struct FetchPlan {
    FetchSpan span[SPAN_COUNT];
    size_t wf_bytes = 0, iq_bytes = 0;  // iq_bytes: what the IQ copy moves
    int n = 0, n0 = 0;                  // copies; the first n0 on stream 0, `done` behind them, then the PCM's
    FetchCopy copy[FETCH_COPIES_MAX];
    int frames = 0;                     // what the set records: the batch's frames, and whether it carries the batch's seq
    bool carries_seq = false, has_pcm = false;
};
inline FetchCopy fetch_rows(const FetchFacts &f, FetchBuf buf, size_t first_slot, size_t slots, size_t row_elems, size_t elem_bytes) {
    FetchCopy k;
    k.buf = buf;
    k.src_off = first_slot * f.mb * row_elems;
    k.width = f.F * row_elems * elem_bytes, k.pitch = f.mb * row_elems * elem_bytes, k.rows = slots;
    k.pitched = f.F != f.mb;
    return k;
}
// the waterfall rows first (small; their device buffer exists once: the next gather waits for ev_wf alone), then pwr, NaN
// flags, audio and the three spans (ev_audio: what the demodulation of batch b + 2 overwrites); the PCM on a stream of its own
inline FetchPlan fetch_plan(const FetchFacts &f, const FetchSlot *slots, const WfSlot *wslots, size_t nw) {
    FetchPlan p;
    const bool audio = fetch_wants_audio(f.what);
    for (int k = 0; k < SPAN_COUNT; k++) p.span[k] = span_of(f.what, slots, f.S, (FetchSpanKind)k);
    p.wf_bytes = wf_bytes(f.what, wslots, nw);
    if (p.wf_bytes) {
        FetchCopy &k = p.copy[p.n++];
        k.buf = FB_WF, k.width = k.pitch = p.wf_bytes, k.rows = 1, k.after = FE_WF;
    }
    if (audio) {
        p.copy[p.n++] = fetch_rows(f, FB_PWR, 0, f.S, 1, sizeof(float));
        p.copy[p.n++] = fetch_rows(f, FB_NAN, 0, f.S, 1, sizeof(int32_t));
        if (f.what & PSDR_FETCH_AUDIO) p.copy[p.n++] = fetch_rows(f, FB_AUDIO, 0, f.S, f.h, sizeof(float));
        const FetchBuf sb[SPAN_COUNT] = {FB_IQ, FB_CAR, FB_SQ};
        const size_t row[SPAN_COUNT] = {f.h, 1, 1}, eb[SPAN_COUNT] = {2 * sizeof(float), 2 * sizeof(float), sizeof(int32_t)};
        for (int k = 0; k < SPAN_COUNT; k++)
            if (p.span[k].n > 0) p.copy[p.n++] = fetch_rows(f, sb[k], (size_t)p.span[k].lo, (size_t)p.span[k].n, row[k], eb[k]);
        if (p.span[SPAN_IQ].n > 0) p.iq_bytes = (size_t)p.span[SPAN_IQ].n * f.F * f.h * 2 * sizeof(float);
        p.copy[p.n - 1].after = FE_AUDIO;
    }
    p.n0 = p.n;
    if (f.what & PSDR_FETCH_PCM) {
        FetchCopy &k = p.copy[p.n++];
        k = fetch_rows(f, FB_PCM, 0, f.S, f.h, f.pcm16 ? sizeof(int16_t) : sizeof(int32_t));
        k.stream = 1, k.after = FE_PCM;
        p.has_pcm = true;
    }
    p.frames = audio ? (int)f.F : 0;
    p.carries_seq = audio;
    return p;
}

// ---- the ring of host sets -------------------------------------------------------------------------------------------------
// psdr_fetch_begin fills set `fill` and moves on; the fetches in flight are the `inflight` sets behind it, oldest first.  A
// begin onto a set that is still in flight (every set is) gives that fetch up; a begin onto the set psdr_fetched_* read
// takes it from them.
inline int ring_oldest(int fill, int inflight) { return (fill - inflight + 2 * PSDR_FETCH_SETS) % PSDR_FETCH_SETS; }
inline int ring_next(int fill) { return (fill + 1) % PSDR_FETCH_SETS; }
inline int ring_cur_after_begin(int cur, int fill) { return cur == fill ? -1 : cur; }

// ---- whose rows a slot of a fetched set holds ------------------------------------------------------------------------------
// per audio slot: what the batch was demodulated with
struct FetchWin {
    uint64_t last_seq = 0, born = 0;  // last_seq: 0 for a slot without a client at the time of the fetch
    int l = 0, r = 0;
    double mid = 0;
    int mode = PSDR_USB;
    bool sq = false;  // the batch ran with squelch for the slot (psdr_fetched_squelch: 1 for every frame otherwise)
};
// the slot was part of the set's batch, and the client that holds it now is the one that was (a slot handed to a new client
// since holds the previous occupant's rows)
inline bool fetched_member(const FetchWin &w, uint64_t set_seq, uint64_t born_now) { return w.last_seq == set_seq && w.born == born_now; }
// a batch demodulated as PSDR_IQ holds complex rows and no audio / PCM, any other batch no IQ rows
inline bool iq_kind_matches(int mode, bool want_iq) { return (mode == PSDR_IQ) == want_iq; }
// rows of [slot][max_batch][...] and of a span's [slot - lo][max_batch][...]
inline size_t fetch_row(int id, size_t mb, int frame) { return (size_t)id * mb + (size_t)frame; }
inline size_t span_row(const FetchSpan &s, int id, size_t mb, int frame) { return (size_t)(id - s.lo) * mb + (size_t)frame; }

}  // namespace psdr

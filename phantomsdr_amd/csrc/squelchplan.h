// squelchplan.h - the per-client squelch (include/psdr.h: psdr_client_set_squelch), everything of it that is not a launch: the
// ONE definition of the per-frame step (k_squelch in squelch.h and the host tests run this text), the dB-to-f32 conversion, the
// argument validation and squelch_plan(), which walks the audio slots behind demod_plan() and says who is gated in the batch,
// whose state starts from zero and which slots a fetch copies.  Plain C++17 (no HIP): tests/test_squelch_host.py builds it
// with the host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "demodplan.h"

// the step is host code and device code alike
#if defined(__HIPCC__)
#define PSDR_HOST_DEVICE __host__ __device__
#else
#define PSDR_HOST_DEVICE
#endif

namespace psdr {

// what a client carries from frame to frame and batch to batch: the gate and a run counter
struct SquelchState {
    int open, cnt;
};
// One entry of the batch's squelch table.  attack >= 1: a squelch client.  attack == 0: an audio client WITHOUT squelch in a
// post-chain batch that has squelch clients - its drop flags are its NaN flags, copied (the chain reads one array).
// pad: the squelch's reference (include/psdr.h: psdr_client_set_squelch_reference) - 0: the thresholds are absolute, 1:
// relative to the frame's noise power W_f (noiseplan.h).
struct SquelchEntry {
    int slot, attack, hang, pad;
    float t_open, t_close;
};
static_assert(sizeof(SquelchState) == 8 && sizeof(SquelchEntry) == 24, "the device tables' layout");

constexpr double SQUELCH_DB_MAX = 300.0;       // |open_db|, |close_db| <= 300: 1e-30 .. 1e30, normal f32 numbers both
constexpr int SQUELCH_FRAMES_MAX = 1 << 20;    // attack_frames 1..2^20, hang_frames 0..2^20: the counter stays far from overflow

// T = (float)pow(10, db / 10): computed in double, rounded once
inline float squelch_threshold(double db) { return (float)std::pow(10.0, db / 10.0); }

// the two comparisons of a frame: NaN compares false both ways (never above T_open, never at or above T_close), +Inf is above
PSDR_HOST_DEVICE inline bool squelch_ge(float p, float t) { return p >= t; }

// One frame: ge_open = (P >= T_open), ge_close = (P >= T_close).  Returns the frame's flag: `open` AFTER the update - the frame
// that completes the attack is heard, the frame that exhausts the hang is not.
PSDR_HOST_DEVICE inline int squelch_step(SquelchState &s, bool ge_open, bool ge_close, int attack, int hang) {
    if (!s.open) {
        s.cnt = ge_open ? s.cnt + 1 : 0;
        if (s.cnt >= attack) s.open = 1, s.cnt = 0;
    } else {
        s.cnt = !ge_close ? s.cnt + 1 : 0;
        if (s.cnt > hang) s.open = 0, s.cnt = 0;
    }
    return s.open;
}
PSDR_HOST_DEVICE inline int squelch_frame(SquelchState &s, float p, const SquelchEntry &e) {
    return squelch_step(s, squelch_ge(p, e.t_open), squelch_ge(p, e.t_close), e.attack, e.hang);
}
// A noise-referenced entry's threshold of frame f: one f32 product with the frame's noise power.  W_f = 0 (before the first
// estimate, digital silence): any power that is not NaN is at or above it.
PSDR_HOST_DEVICE inline float squelch_relative(float t, float w) { return t * w; }
PSDR_HOST_DEVICE inline int squelch_frame_relative(SquelchState &s, float p, float w, const SquelchEntry &e) {
    return squelch_step(s, squelch_ge(p, squelch_relative(e.t_open, w)), squelch_ge(p, squelch_relative(e.t_close, w)), e.attack, e.hang);
}

// A chunk of up to 64 consecutive frames whose comparisons are two masks (bit j: frame j; k_squelch's ballots): the mask of the
// frames that are heard
PSDR_HOST_DEVICE inline unsigned long long squelch_walk(SquelchState &s, unsigned long long ge_open, unsigned long long ge_close, int nframes, int attack,
                                                        int hang) {
    // a chunk that cannot move the gate needs no walk: closed and no frame above T_open, or open and every frame at or above
    // T_close - each frame of it sets cnt = 0 and keeps `open`, which is what the walk would leave (nframes >= 1)
    const unsigned long long all = nframes >= 64 ? ~0ull : (1ull << nframes) - 1ull;
    if (nframes > 0 && !s.open && (ge_open & all) == 0) {
        s.cnt = 0;
        return 0;
    }
    if (nframes > 0 && s.open && (ge_close & all) == all) {
        s.cnt = 0;
        return all;
    }
    unsigned long long heard = 0;
    for (int j = 0; j < nframes; j++)
        if (squelch_step(s, (ge_open >> j) & 1ull, (ge_close >> j) & 1ull, attack, hang)) heard |= 1ull << j;
    return heard;
}

// psdr_client_set_squelch's refusals, in the order they are looked for; on = 0 ignores everything behind the id
enum SquelchVerdict { SQ_OK, SQ_BAD_ID, SQ_BAD_DB, SQ_CLOSE_ABOVE_OPEN, SQ_BAD_ATTACK, SQ_BAD_HANG };
inline SquelchVerdict squelch_check(const AudioSlot *slots, size_t S, int id, int on, double open_db, double close_db, int attack, int hang) {
    if (id < 0 || (size_t)id >= S || !slots[id].active) return SQ_BAD_ID;
    if (!on) return SQ_OK;
    if (!std::isfinite(open_db) || !std::isfinite(close_db) || std::fabs(open_db) > SQUELCH_DB_MAX || std::fabs(close_db) > SQUELCH_DB_MAX) return SQ_BAD_DB;
    if (close_db > open_db) return SQ_CLOSE_ABOVE_OPEN;
    if (attack < 1 || attack > SQUELCH_FRAMES_MAX) return SQ_BAD_ATTACK;
    if (hang < 0 || hang > SQUELCH_FRAMES_MAX) return SQ_BAD_HANG;
    return SQ_OK;
}
// ... and what an accepted call does to the slot: switching it ON starts the state from (closed, 0) at the client's next batch
// (also while paused); new thresholds or counts of a client that is on keep the state
inline void squelch_apply(AudioSlot &s, int on, double open_db, double close_db, int attack, int hang) {
    if (!on) {
        s.sq_on = 0;
        return;
    }
    if (!s.sq_on) s.sq_fresh = true;
    s.sq_on = 1;
    s.sq_t_open = squelch_threshold(open_db), s.sq_t_close = squelch_threshold(close_db);
    s.sq_attack = attack, s.sq_hang = hang;
}

struct SquelchPlan {
    int nsq = 0;    // table[0, nsq): the batch's squelch clients, in slot order
    int ncopy = 0;  // table[nsq, nsq + ncopy): the chain's other audio clients (attack == 0), in slot order
    std::vector<size_t> zero;  // slots whose state starts this batch from (closed, 0)
    int lo = 0, n = 0;         // the fetch's span: the n slots from the lowest to the highest squelch slot (n == 0: none)
    bool any_ref = false;      // a squelch client of the batch is noise-referenced: k_squelch reads the batch's W rows
    bool any() const { return nsq > 0; }  // no squelch client in the batch: nothing is uploaded, zeroed or launched
};

// One batch, behind demod_plan(): the clients it demodulated are those whose last_seq is the batch's demod_seq.  Writes the
// table (room for S entries), moves b_sq_on and sq_fresh on.  chain: the post chain runs behind this batch.
inline SquelchPlan squelch_plan(AudioSlot *slots, size_t S, uint64_t demod_seq, bool chain, SquelchEntry *table) {
    SquelchPlan p;
    int hi = -1;
    for (size_t i = 0; i < S; i++) {
        AudioSlot &s = slots[i];
        if (!s.active || s.paused || s.last_seq != demod_seq) continue;  // a paused client's state stands still
        s.b_sq_on = s.sq_on != 0;
        if (!s.sq_on) continue;
        if (s.sq_fresh) p.zero.push_back(i);
        s.sq_fresh = false;
        const int ref = s.sq_ref == PSDR_SQ_NOISE ? 1 : 0;  // (PSDR_SQ_NOISE is only ever set on a noise-floor client)
        p.any_ref |= ref != 0;
        table[p.nsq++] = SquelchEntry{(int)i, s.sq_attack, s.sq_hang, ref, s.sq_t_open, s.sq_t_close};
        if (hi < 0) p.lo = (int)i;
        hi = (int)i;
    }
    if (!p.any()) return p;
    p.n = hi - p.lo + 1;
    if (chain)
        for (size_t i = 0; i < S; i++) {
            const AudioSlot &s = slots[i];
            if (s.active && !s.paused && s.last_seq == demod_seq && !s.sq_on && s.b_mode != PSDR_IQ)
                table[p.nsq + p.ncopy++] = SquelchEntry{(int)i, 0, 0, 0, 0.f, 0.f};
        }
    return p;
}

}  // namespace psdr

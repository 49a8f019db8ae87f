// noiseplan.h - the per-client noise floor (include/psdr.h: psdr_client_set_noise_floor, psdr_client_set_squelch_reference),
// everything of it that is not a launch: the ONE definition of every step of the rule (k_noise_floor in noise.h and the host
// tests run this text), the validation of the two calls and noise_plan(), which walks the audio slots behind demod_plan() as
// squelch_plan() does and says who is listed in the batch, whose state starts from zero and which slots a fetch copies.  Plain
// C++17 (no HIP): tests/test_noise_host.py builds it with the host compiler.
//
// The rule, for a client with window [l, r), len = r - l, and period = max(1, audio_rate / audio_fft_size) frames:
//   bin power   p = fmaf(re, re, im * im) of the raw spectrum bin l + t (un-notched, as the auto-notch detector takes it)
//   sums        acc[t] += p, per bin, in frame order
//   evaluation  every `period` frames: q = the k-th smallest sum, k = (len - 1) / 4, in the order of the sums' bit patterns as
//               unsigned integers (numeric order for the non-negative sums, +Inf above every finite value, NaN above +Inf);
//               e = q / (float)period goes into a ring of the last NOISE_RING evaluations, the sums start again from zero
//   estimate    n0 = the smallest FINITE ring entry, 0 if there is none (before the first evaluation, or all of them Inf / NaN)
//   record      W_f = n0 * (float)len, with n0 as it stands behind frame f: the window's noise power in the units of pwr
// Every float operation above is one correctly rounded f32 operation, and a sum grows in frame order: the bits do not depend on
// how the frames are split into batches.
//
// What n0 is NOT: the mean noise power per bin.  The lower quartile of `len` sums of `period` exponentially distributed powers
// lies below their mean, and the minimum over the ring's 8 evaluations (4 s) lies lower still; for Gaussian noise the factor
// depends on `period` (about 0.29 at period 1, towards 1 as period grows).  A threshold against W - the relative squelch's, a
// front end's SNR pwr / W - is relative to THIS number, not to the mean, as the blanker's is to its own reference level.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "demodplan.h"

// the steps are host code and device code alike
#if defined(__HIPCC__)
#define PSDR_HOST_DEVICE __host__ __device__
#else
#define PSDR_HOST_DEVICE
#endif

namespace psdr {

constexpr int NOISE_RING = 8;  // evaluations the estimate looks back over

// What a client carries from frame to frame and batch to batch beside its sums acc[audio_fft_size]: the ring, how many of its
// entries are filled, where the next one goes, and the frames summed since the last evaluation.  All zero: the start.
struct NoiseState {
    float ring[NOISE_RING];
    int fill, pos, cnt, pad;
};
// One entry of the batch's table: a noise-floor client's slot and the window of the batch's snapshot
struct NoiseEntry {
    int slot, l, r, pad;
};
static_assert(sizeof(NoiseState) == 48 && sizeof(NoiseEntry) == 16, "the device tables' layout");

inline int noise_period(int audio_rate, int audio_fft_size) { return audio_rate / audio_fft_size > 1 ? audio_rate / audio_fft_size : 1; }

// ---- the steps -------------------------------------------------------------------------------------------------------------
PSDR_HOST_DEVICE inline float noise_fma(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fmaf(a, b, c);
#else
    return std::fmaf(a, b, c);
#endif
}
PSDR_HOST_DEVICE inline float noise_bin_power(float re, float im) { return noise_fma(re, re, im * im); }
PSDR_HOST_DEVICE inline int noise_rank(int len) { return (len - 1) / 4; }  // (len >= 1)
PSDR_HOST_DEVICE inline uint32_t noise_bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
PSDR_HOST_DEVICE inline float noise_float(uint32_t u) {
    float v;
    memcpy(&v, &u, 4);
    return v;
}
// The k-th smallest (0-based) of a set of 32-bit patterns, by a radix select from the top bit down: `prefix` holds the bits of
// the answer found so far, count(prefix, mask) says how many patterns x of the set have (x & mask) == prefix - those that
// agree with the answer's upper bits and have a 0 in the bit under test.  Exact, no sort; ties need no rule.
template <class Count>
PSDR_HOST_DEVICE inline uint32_t noise_select(int k, Count count) {
    uint32_t prefix = 0;
    for (int b = 31; b >= 0; b--) {
        const int zeros = count(prefix, ~0u << b);
        if (k >= zeros) k -= zeros, prefix |= 1u << b;
    }
    return prefix;
}
// ... as a scalar function over an array of sums (the kernel counts with ballots, lane i owning the bins i + 64 j)
inline float noise_select_host(const float *sums, int len, int k) {
    return noise_float(noise_select(k, [&](uint32_t prefix, uint32_t mask) {
        int c = 0;
        for (int t = 0; t < len; t++) c += (noise_bits(sums[t]) & mask) == prefix;
        return c;
    }));
}
// an evaluation's entry: the selected sum as power per frame
PSDR_HOST_DEVICE inline float noise_entry(float q, int period) { return q / (float)period; }
// ... into the ring (written without a variable index: on the device the state lives in registers)
PSDR_HOST_DEVICE inline void noise_push(NoiseState &s, float e) {
    for (int i = 0; i < NOISE_RING; i++)
        if (i == s.pos) s.ring[i] = e;
    s.pos = (s.pos + 1) % NOISE_RING;
    if (s.fill < NOISE_RING) s.fill++;
}
// the estimate: a NaN or Inf entry is never the minimum
PSDR_HOST_DEVICE inline float noise_estimate(const NoiseState &s) {
    float m = HUGE_VALF;
    for (int i = 0; i < NOISE_RING; i++)
        if (i < s.fill) {
            const float x = s.ring[i];
            m = (x < m) ? x : m;
        }
    return (m < HUGE_VALF) ? m : 0.f;
}
PSDR_HOST_DEVICE inline float noise_window_power(float n0, int len) { return n0 * (float)len; }

// ---- the two calls -----------------------------------------------------------------------------------------------------------
// psdr_client_set_noise_floor's refusals, in the order they are looked for
enum NoiseVerdict { NF_OK, NF_BAD_ID, NF_NO_RATE, NF_IN_USE };
inline NoiseVerdict noise_floor_check(const AudioSlot *slots, size_t S, int id, int on, int audio_rate) {
    if (id < 0 || (size_t)id >= S || !slots[id].active) return NF_BAD_ID;
    if (audio_rate <= 0) return NF_NO_RATE;
    if (!on && slots[id].sq_ref == PSDR_SQ_NOISE) return NF_IN_USE;  // the squelch would lose its reference
    return NF_OK;
}
// ... and what an accepted call does to the slot: switching it ON starts the state from zero at the client's next batch (also
// while paused)
inline void noise_floor_apply(AudioSlot &s, int on) {
    if (on && !s.nf_on) s.nf_fresh = true;
    s.nf_on = on ? 1 : 0;
}
// psdr_client_set_squelch_reference's refusals, in the order they are looked for
enum SqRefVerdict { SR_OK, SR_BAD_ID, SR_BAD_VALUE, SR_NOISE_OFF };
inline SqRefVerdict squelch_reference_check(const AudioSlot *slots, size_t S, int id, int ref) {
    if (id < 0 || (size_t)id >= S || !slots[id].active) return SR_BAD_ID;
    if (ref != PSDR_SQ_ABSOLUTE && ref != PSDR_SQ_NOISE) return SR_BAD_VALUE;
    if (ref == PSDR_SQ_NOISE && !slots[id].nf_on) return SR_NOISE_OFF;
    return SR_OK;
}
// (a setting and nothing else: the gate's state is not touched)
inline void squelch_reference_apply(AudioSlot &s, int ref) { s.sq_ref = ref; }

// ---- the batch ---------------------------------------------------------------------------------------------------------------
struct NoisePlan {
    int n = 0;                 // table[0, n): the batch's noise-floor clients, in slot order
    std::vector<size_t> zero;  // slots whose sums and record start this batch from zero
    int lo = 0, nspan = 0;     // the fetch's span: the nspan slots from the lowest to the highest listed slot (nspan == 0: none)
    bool any() const { return n > 0; }  // no noise-floor client in the batch: nothing is uploaded, zeroed or launched
};
// One batch, behind demod_plan(): the clients it demodulated are those whose last_seq is the batch's demod_seq, and b_l / b_r
// the window they were demodulated with.  Writes the table (room for S entries), moves b_nf_on, nf_fresh and the window the state
// belongs to (nf_l, nf_r) on.  The state starts from zero when the feature was switched on since the slot's last batch and
// whenever [l, r) is not the one of the client's previous batch; a mode change, a change of audio_mid alone or of the notches
// does not touch it, and a paused client's stands still.
inline NoisePlan noise_plan(AudioSlot *slots, size_t S, uint64_t demod_seq, NoiseEntry *table) {
    NoisePlan p;
    int hi = -1;
    for (size_t i = 0; i < S; i++) {
        AudioSlot &s = slots[i];
        if (!s.active || s.paused || s.last_seq != demod_seq) continue;
        s.b_nf_on = s.nf_on != 0;
        if (!s.nf_on) continue;
        if (s.nf_fresh || s.nf_l != s.b_l || s.nf_r != s.b_r) p.zero.push_back(i);
        s.nf_fresh = false;
        s.nf_l = s.b_l, s.nf_r = s.b_r;
        table[p.n++] = NoiseEntry{(int)i, s.b_l, s.b_r, 0};
        if (hi < 0) p.lo = (int)i;
        hi = (int)i;
    }
    if (p.any()) p.nspan = hi - p.lo + 1;
    return p;
}
// the span a fetch of the batch `demod_seq` copies, from the slots as they stand at the fetch: lo, n (nobody: 0, 0)
inline void noise_fetch_span(const AudioSlot *slots, size_t S, uint64_t demod_seq, int *lo, int *n) {
    int first = (int)S, hi = -1;
    for (size_t i = 0; i < S; i++)
        if (slots[i].active && slots[i].last_seq == demod_seq && slots[i].b_nf_on) {
            if (hi < 0) first = (int)i;
            hi = (int)i;
        }
    *lo = hi < 0 ? 0 : first, *n = hi < 0 ? 0 : hi - first + 1;
}

// ---- one client's frames on the host: what k_noise_floor does, run by run -------------------------------------------------------
// `power(t, f)`: the power of window bin t in frame f of the batch.  Adds the batch's nframes frames to the sums (acc[len]) and
// the state, writes W[nframes].  len <= 0: nothing is added, the state stands, W = 0.
template <class Power>
inline void noise_batch_host(NoiseState &st, float *acc, int len, int period, int nframes, Power power, float *W) {
    if (len <= 0) {
        for (int f = 0; f < nframes; f++) W[f] = 0.f;
        return;
    }
    int f = 0;
    while (f < nframes) {
        const int fe = f + period - st.cnt < nframes ? f + period - st.cnt : nframes;
        for (int t = 0; t < len; t++)
            for (int g = f; g < fe; g++) acc[t] += power(t, g);
        const float before = noise_window_power(noise_estimate(st), len);
        st.cnt += fe - f;
        const bool evaluate = st.cnt >= period;
        if (evaluate) {
            noise_push(st, noise_entry(noise_select_host(acc, len, noise_rank(len)), period));
            for (int t = 0; t < len; t++) acc[t] = 0.f;
            st.cnt = 0;
        }
        const float after = noise_window_power(noise_estimate(st), len);
        for (int g = f; g < fe; g++) W[g] = (evaluate && g == fe - 1) ? after : before;
        f = fe;
    }
}

}  // namespace psdr

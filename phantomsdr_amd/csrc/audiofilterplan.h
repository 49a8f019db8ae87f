// audiofilterplan.h - the per-client audio filter (include/psdr.h: psdr_client_set_audio_filter), everything of it that is not a
// launch: the ONE definition of the section's step and of its blocked evaluation (k_audio_filter in audiofilter.h and the host
// tests run this text), the table entry with the state matrix's powers, the argument validation, the design formulas and
// audio_filter_plan(), which walks the audio slots behind demod_plan() and says who is filtered in the batch and whose state
// starts from zero.  Plain C++17 (no HIP): tests/test_audio_filter_host.py builds it with the host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "demodplan.h"

// the step is host code and device code alike
#ifndef PSDR_HOST_DEVICE
#if defined(__HIPCC__)
#define PSDR_HOST_DEVICE __host__ __device__
#else
#define PSDR_HOST_DEVICE
#endif
#endif
#if defined(__HIPCC__)
#define PSDR_AF_UNROLL _Pragma("unroll")
#else
#define PSDR_AF_UNROLL
#endif

namespace psdr {

constexpr int AF_CHUNK = 16;                    // consecutive samples of one lane
constexpr int AF_LANES = 64;                    // chunks of one block: a wave
constexpr int AF_BLOCK = AF_CHUNK * AF_LANES;   // samples per block
constexpr int AF_LEVELS = 6;                    // scan levels: 2^6 lanes
// A pole radius above this is refused.  It admits a 700 Hz peak filter of Q 20 at 12 kHz (0.9911) and at 48 kHz (0.9977) and keeps
// the f32 state and the scan's powers well conditioned (the highest power the scan uses, M^32 = A^512, still has 0.77 of a
// mode at this radius); a design constant, not a measurement
constexpr double AF_POLE_MAX = 0.9995;

// One entry of the batch's table: a filtered client
struct AfEntry {
    int slot, nsec, pad[2];
    AfSection sec[PSDR_AUDIO_FILTER_SECTIONS];
};
static_assert(sizeof(AfEntry) == 16 + 128 * PSDR_AUDIO_FILTER_SECTIONS, "the device table's layout");

// ---- the rule -----------------------------------------------------------------------------------------------------------------
// One sample of one section, transposed direct form II: every operation an fmaf, or the lone multiply -a2 * y
PSDR_HOST_DEVICE inline float af_step(const AfSection &c, float x, float &s1, float &s2) {
    const float y = fmaf(c.b0, x, s1);
    s1 = fmaf(c.b1, x, fmaf(-c.a1, y, s2));
    s2 = fmaf(c.b2, x, -c.a2 * y);
    return y;
}
// Step 1, the zero-state pass: the state a chunk's AF_CHUNK samples leave behind when they start from (0, 0)
PSDR_HOST_DEVICE inline void af_chunk_zero(const AfSection &c, const float *x, float &c1, float &c2) {
    c1 = 0.f, c2 = 0.f;
    PSDR_AF_UNROLL
    for (int k = 0; k < AF_CHUNK; k++) af_step(c, x[k], c1, c2);
}
// Step 2's combine, v <- v + P u, in this order: v1 = fma(P00, u1, fma(P01, u2, v1)), v2 = fma(P10, u1, fma(P11, u2, v2)).
// The scan: v_j starts as chunk j's zero-state end state; the carried state enters as lane -1, that is v_0 <- v_0 + P[0] carry;
// then for k = 0..5, d = 2^k, every lane j >= d takes v_j <- v_j + P[k] v_(j-d) with the v of before the level (an inclusive
// Hillis-Steele scan).  The state ENTERING lane j is v_(j-1), and the carried state itself for lane 0.
PSDR_HOST_DEVICE inline void af_combine(const float *P, float u1, float u2, float &v1, float &v2) {
    v1 = fmaf(P[0], u1, fmaf(P[1], u2, v1));
    v2 = fmaf(P[2], u1, fmaf(P[3], u2, v2));
}
// Step 3, the true pass: the chunk again, in place, from the state that enters it.  The state moves over the first cnt samples
// only (cnt < AF_CHUNK: the stream ends inside the chunk; what the samples behind the end yield is not stored)
PSDR_HOST_DEVICE inline void af_chunk_run(const AfSection &c, float *x, int cnt, float &s1, float &s2) {
    PSDR_AF_UNROLL
    for (int k = 0; k < AF_CHUNK; k++) {
        float t1 = s1, t2 = s2;
        x[k] = af_step(c, x[k], t1, t2);
        if (k < cnt) s1 = t1, s2 = t2;
    }
}
// One section over one block of len <= AF_BLOCK samples, x[AF_BLOCK] in place (zeros behind len), the host's loop over "lanes":
// the chunks 0..last that hold data.  The state the section carries on is the last data chunk's state behind its samples.
inline void af_block_section(const AfSection &c, float *x, int len, float &s1, float &s2) {
    const int last = (len - 1) / AF_CHUNK;
    float v1[AF_LANES], v2[AF_LANES];
    for (int j = 0; j <= last; j++) af_chunk_zero(c, x + AF_CHUNK * j, v1[j], v2[j]);
    af_combine(c.P[0], s1, s2, v1[0], v2[0]);
    for (int k = 0; k < AF_LEVELS; k++)
        for (int d = 1 << k, j = last; j >= d; j--) af_combine(c.P[k], v1[j - d], v2[j - d], v1[j], v2[j]);  // (descending: v[j - d] is still the level's input)
    for (int j = last; j >= 0; j--) {
        float e1 = j ? v1[j - 1] : s1, e2 = j ? v2[j - 1] : s2;
        af_chunk_run(c, x + AF_CHUNK * j, std::min(AF_CHUNK, len - AF_CHUNK * j), e1, e2);
        if (j == last) v1[last] = e1, v2[last] = e2;
    }
    s1 = v1[last], s2 = v2[last];
}
// A client's batch on the host, as k_audio_filter runs it: rows[nframes * h] in place, flags[nframes] the frames' NaN flags,
// state[2 sections][2] carried.  A flagged frame enters as zeros and its row is left alone.
inline void af_stream(const AfEntry &e, float *rows, const int *flags, int h, int nframes, float *state) {
    const long L = (long)nframes * h;
    float x[AF_BLOCK];
    for (long b0 = 0; b0 < L; b0 += AF_BLOCK) {
        const int len = (int)std::min<long>(AF_BLOCK, L - b0);
        for (int i = 0; i < AF_BLOCK; i++) x[i] = i < len && !flags[(b0 + i) / h] ? rows[b0 + i] : 0.f;
        for (int s = 0; s < e.nsec; s++) af_block_section(e.sec[s], x, len, state[2 * s], state[2 * s + 1]);
        for (int i = 0; i < len; i++)
            if (!flags[(b0 + i) / h]) rows[b0 + i] = x[i];
    }
}

// ---- the table entry ----------------------------------------------------------------------------------------------------------
// The coefficients rounded once to f32; from the ROUNDED a1, a2 (the system the f32 recurrence runs) the powers in double, each
// rounded once
inline AfSection af_section(const psdr_biquad &q) {
    AfSection s;
    s.b0 = (float)q.b0, s.b1 = (float)q.b1, s.b2 = (float)q.b2, s.a1 = (float)q.a1, s.a2 = (float)q.a2;
    double m[4] = {-(double)s.a1, 1.0, -(double)s.a2, 0.0};
    auto square = [&] {
        const double r[4] = {m[0] * m[0] + m[1] * m[2], m[0] * m[1] + m[1] * m[3], m[2] * m[0] + m[3] * m[2], m[2] * m[1] + m[3] * m[3]};
        for (int i = 0; i < 4; i++) m[i] = r[i];
    };
    for (int i = 0; i < 4; i++) square();  // A^16 (AF_CHUNK = 2^4)
    static_assert(AF_CHUNK == 16, "af_section squares four times");
    for (int k = 0; k < AF_LEVELS; k++) {
        for (int i = 0; i < 4; i++) s.P[k][i] = (float)m[i];
        square();
    }
    return s;
}

// ---- validation ---------------------------------------------------------------------------------------------------------------
// psdr_client_set_audio_filter's refusals, in the order they are looked for (each in every section before the next);
// nsections = 0 ignores everything behind it
enum AfVerdict { AF_OK, AF_BAD_ID, AF_BAD_COUNT, AF_NULL, AF_NONFINITE, AF_UNSTABLE, AF_POLE };
// the larger pole radius of a stable section against AF_POLE_MAX: complex poles have radius sqrt(a2) (compared squared: the limit
// itself passes), real ones (|a1| + sqrt(a1^2 - 4 a2)) / 2
inline bool af_pole_outside(double a1, double a2) {
    const double disc = a1 * a1 - 4.0 * a2;
    if (disc < 0) return a2 > AF_POLE_MAX * AF_POLE_MAX;
    return (std::fabs(a1) + std::sqrt(disc)) / 2.0 > AF_POLE_MAX;
}
// (stability and radius are judged on the doubles as given, as include/psdr.h says: the f32 rounding of a1, at most 1.2e-7, and of
// a2, 3e-8, cannot use up the 2.5e-7 that (1 - p1)(1 - p2) = 1 + a1 + a2 keeps with both real poles at AF_POLE_MAX)
inline AfVerdict audio_filter_check_sections(int nsections, const psdr_biquad *sec) {
    if (nsections < 0 || nsections > PSDR_AUDIO_FILTER_SECTIONS) return AF_BAD_COUNT;
    if (nsections == 0) return AF_OK;
    if (!sec) return AF_NULL;
    for (int i = 0; i < nsections; i++)
        if (!std::isfinite(sec[i].b0) || !std::isfinite(sec[i].b1) || !std::isfinite(sec[i].b2) || !std::isfinite(sec[i].a1) || !std::isfinite(sec[i].a2))
            return AF_NONFINITE;
    // (the coefficients must be f32 numbers too: a finite double beyond FLT_MAX would round to infinity)
    for (int i = 0; i < nsections; i++)
        if (!std::isfinite((float)sec[i].b0) || !std::isfinite((float)sec[i].b1) || !std::isfinite((float)sec[i].b2)) return AF_NONFINITE;
    for (int i = 0; i < nsections; i++)
        if (!(std::fabs(sec[i].a2) < 1.0) || !(std::fabs(sec[i].a1) < 1.0 + sec[i].a2)) return AF_UNSTABLE;
    for (int i = 0; i < nsections; i++)
        if (af_pole_outside(sec[i].a1, sec[i].a2)) return AF_POLE;
    return AF_OK;
}
inline AfVerdict audio_filter_check(const AudioSlot *slots, size_t S, int id, int nsections, const psdr_biquad *sec) {
    if (id < 0 || (size_t)id >= S || !slots[id].active) return AF_BAD_ID;
    return audio_filter_check_sections(nsections, sec);
}
// ... and what an accepted call does to the slot: with nsections >= 1 the state starts from zero at the client's next filtered
// batch - switching on or new coefficients alike (also while paused, or while the client is an IQ client)
inline void audio_filter_apply(AudioSlot &s, int nsections, const psdr_biquad *sec) {
    s.af_n = nsections;
    if (nsections == 0) return;
    for (int i = 0; i < nsections; i++) s.af_sec[i] = af_section(sec[i]);
    s.af_fresh = true;
}

// ---- design -------------------------------------------------------------------------------------------------------------------
// psdr_audio_filter_design: the bilinear transform with K = tan(pi f0 / rate), in double (include/psdr.h has the formulas)
enum AfDesignVerdict { AD_OK, AD_NULL, AD_BAD_KIND, AD_BAD_RATE, AD_BAD_F0, AD_BAD_Q, AD_REFUSED };
inline AfDesignVerdict audio_filter_design(int kind, double rate, double f0, double q, psdr_biquad *out) {
    if (!out) return AD_NULL;
    if (kind < PSDR_AF_DEEMPHASIS || kind > PSDR_AF_PEAK) return AD_BAD_KIND;
    if (!std::isfinite(rate) || rate <= 0) return AD_BAD_RATE;
    if (!std::isfinite(f0) || f0 <= 0 || f0 >= rate / 2) return AD_BAD_F0;
    if (kind != PSDR_AF_DEEMPHASIS && (!std::isfinite(q) || q <= 0)) return AD_BAD_Q;
    const double K = std::tan(M_PI * f0 / rate);
    psdr_biquad b{};
    if (kind == PSDR_AF_DEEMPHASIS) {
        b.b0 = b.b1 = K / (1.0 + K);
        b.a1 = (K - 1.0) / (K + 1.0);
    } else {
        const double N = 1.0 / (1.0 + K / q + K * K);
        b.a1 = 2.0 * (K * K - 1.0) * N, b.a2 = (1.0 - K / q + K * K) * N;
        if (kind == PSDR_AF_LOWPASS) b.b0 = b.b2 = K * K * N, b.b1 = 2.0 * b.b0;
        if (kind == PSDR_AF_HIGHPASS) b.b0 = b.b2 = N, b.b1 = -2.0 * N;
        if (kind == PSDR_AF_PEAK) b.b0 = K / q * N, b.b2 = -b.b0;
    }
    if (audio_filter_check_sections(1, &b) != AF_OK) return AD_REFUSED;
    *out = b;
    return AD_OK;
}

// ---- the batch ----------------------------------------------------------------------------------------------------------------
struct AfPlan {
    int n = 0;                 // table[0, n): the batch's filtered clients, in slot order
    std::vector<size_t> zero;  // slots whose state starts this batch from zero
    bool any() const { return n > 0; }  // no filter client in the batch: nothing is uploaded, zeroed or launched
};
// One batch, behind demod_plan(): the clients it demodulated are those whose last_seq is the batch's demod_seq; of these the ones
// with a filter whose kind wrote audio rows are listed.  Writes the table (room for S entries) and moves af_fresh on.  An IQ
// client and a paused one keep setting, state and a pending fresh start.
inline AfPlan audio_filter_plan(AudioSlot *slots, size_t S, uint64_t demod_seq, AfEntry *table) {
    AfPlan p;
    for (size_t i = 0; i < S; i++) {
        AudioSlot &s = slots[i];
        if (!s.active || s.paused || s.last_seq != demod_seq || s.b_mode == PSDR_IQ || s.af_n == 0) continue;
        if (s.af_fresh) p.zero.push_back(i);
        s.af_fresh = false;
        AfEntry &e = table[p.n++];
        e.slot = (int)i, e.nsec = s.af_n, e.pad[0] = e.pad[1] = 0;
        for (int k = 0; k < PSDR_AUDIO_FILTER_SECTIONS; k++) e.sec[k] = k < s.af_n ? s.af_sec[k] : AfSection();
    }
    return p;
}

}  // namespace psdr

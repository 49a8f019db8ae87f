// anbplan.h - the per-client audio blanker (include/psdr.h: psdr_client_set_audio_blanker), everything of it that is not a launch:
// the ONE definition of the detector and of the gap repair (k_audio_nb in anb.hip and the host tests run this text), of the
// stream's bookkeeping, the argument validation, the presets and anb_plan(), which walks the audio slots behind demod_plan() and
// says who is listed in the batch and whose state starts from zero.  Plain C++17 (no HIP): tests/test_anb_host.py builds it with
// the host compiler.  (The wideband blanker on the ingest ring is blanker*.h; this one works on a client's audio rows.)
//
// The rule.  A client's stream is its audio rows in frame order (a flagged frame enters as zeros and its row is left alone, as in
// nr_stream); samples before the stream's start are zero.  Block b covers [s, s + B), s = b B, B = 256, and reads only INPUT
// samples x[s - E .. s + B + E), E = 24 - never a repaired one, so a block is a pure function of the input:
//   1. R[i] = sum x[n] x[n + i], i = 0..P, P = 10, over the n of the block with n + i inside the block.  Order: 64 partial sums,
//      partial l over n = s + l + 64 r, r = 0..3 ascending, each term an fmaf onto the sum (from +0.0); then the tree
//      p[l] += p[l + o], l < o, for o = 32, 16, 8, 4, 2, 1 (anb_tree; a wave's xor butterfly gives every lane these bits).
//   2. Levinson-Durbin (anb_levinson) gives a[0..P], a[0] = 1.  No detections in a block whose R[0] is not finite or not above
//      ANB_R0_MIN.  Order i: acc = R[i], then acc = fmaf(a[j], R[i - j], acc) for j = 1..i-1 ascending; k = -acc / E;
//      a'[j] = fmaf(k, a[i - j], a[j]); a'[i] = k; E' = fmaf(k, acc, E).  Where E' is not positive and finite the filter of the
//      order before stands, the higher coefficients are 0 and the recursion ends.
//   3. e[n] = x[n], then fmaf(a[j], x[n - j], e) for j = 1..P ascending (n in [s, s + B + P)); m[n] = e[n], then
//      fmaf(a[j], e[n + j], m) for j = 1..P ascending (n in the block).
//   4. mean = S / 256 with S the sum of m in the order of step 1 (partials by plain adds), var = V / 256 with V the sum of
//      (m - mean)^2 in that order (each term an fmaf onto the partial); T = threshold * sqrtf(var), a lone multiply.
//   5. n ascending; |m[n]| > T (strictly; never true for a T that is NaN) makes c = n a centre, the scan goes on at n + PL + 1,
//      it ends behind 16 centres.  PL = (width - 1) / 2.
//   6. The gap of c is [c - PL, c + PL].  f[i] = -(sum over j = 1..P ascending of a[j] f[i - j], fmaf onto +0.0), seeded with the P
//      input samples in front of the gap; b[i] likewise backwards in i, seeded with the P input samples behind the gap.  With
//      w = (float)i / (float)(width - 1) (the f32 quotient) and u = 1 - w, gap sample i is fmaf(w, b[i], fmaf(u, f[i], +0.0)).
//      The block's own a is used whatever block the gap's samples lie in.
//   7. A sample in more than one gap takes the value of the gap with the later centre; every other sample passes through.
//   8. Output sample i of the stream is processed sample i - D, D = 2 B + E = 536; the first D outputs are +0.0.
// Every operation is an explicit fmaf, a lone multiply or divide, or an add or a subtract none of whose operands is a multiply's
// result: contraction (-ffp-contract) has nothing to fuse, so the host and the device give the same bits.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cfloat>
#include <cmath>
#include <vector>

#include "demodplan.h"

// the steps are host code and device code alike
#ifndef PSDR_HOST_DEVICE
#if defined(__HIPCC__)
#define PSDR_HOST_DEVICE __host__ __device__
#else
#define PSDR_HOST_DEVICE
#endif
#endif
// the loops over the lags are unrolled on the device, where a[] and the predictors' histories live in registers; the loops over a
// gap's samples stay loops
#if defined(__HIPCC__)
#define ANB_UNROLL _Pragma("unroll")
#define ANB_ROLLED _Pragma("unroll 1")
#else
#define ANB_UNROLL
#define ANB_ROLLED
#endif

namespace psdr {

constexpr int ANB_B = 256;              // block
constexpr int ANB_P = 10;               // prediction order
constexpr int ANB_E = 24;               // input a block reads on either side (>= PL_max + P = 17, a multiple of 8)
constexpr int ANB_MAX = 16;             // impulses per block
constexpr int ANB_WMAX = 15;            // the widest gap
constexpr int ANB_D = 2 * ANB_B + ANB_E;  // the delay
constexpr int ANB_G = 8;                // a gap reaches less than this far out of its block (PL_max = 7)
// the input a batch still needs from before it: its first output is processed sample T - D, which may lie ANB_G - 1 behind the
// start of a block whose predecessor's gaps reach it; that predecessor reads E in front of itself
constexpr int ANB_H = ANB_D + ANB_G + ANB_B + ANB_E;  // 824
constexpr float ANB_R0_MIN = 1e-20f;    // a block whose R[0] is not above this has no detections (a mean square of 4e-23)
constexpr double ANB_THR_MIN = 2.0, ANB_THR_MAX = 12.0;
constexpr int ANB_WIDTH_MIN = 3;

// One entry of the batch's table: a listed client's slot and parameters
struct AnbEntry {
    int slot;
    float threshold;
    int width, pad;
};
// What a client carries from batch to batch: hist[cur & 1] holds the last ANB_H input samples [pos - H, pos) (flagged frames as
// zeros, zeros before the stream's start) - a batch writes the other half while it still reads this one, then cur changes sides -,
// pos the samples taken, impulses and samples the totals over the blocks whose input is complete, b < anb_blocks_done(pos).  All
// zero: the start.
struct AnbState {
    float hist[2][ANB_H];
    uint64_t pos, impulses, samples, cur;
};
static_assert(sizeof(AnbEntry) == 16 && sizeof(AnbState) == 6624 && ANB_H % 8 == 0 && ANB_D % 8 == 0, "the device tables' layout");

// a product that an add takes next: the rounded product, and no multiply that contraction could fuse (nrplan.h: nr_mul)
PSDR_HOST_DEVICE inline float anb_mul(float a, float b) { return fmaf(a, b, 0.f); }

// ---- a block ------------------------------------------------------------------------------------------------------------------
// step 1, partial l of lag i: x -> the block's first sample.  A product whose second factor lies behind the block is taken with
// 0 in its place (the sample is read: it is inside the edge): it adds nothing to a finite sum, and a block with a sample that is
// not finite has no usable R[0] anyway
PSDR_HOST_DEVICE inline float anb_corr_partial(const float *x, int l, int i) {
    float p = 0.f;
    ANB_UNROLL
    for (int r = 0; r < 4; r++) {
        const int n = l + 64 * r;
        const float y = x[n + i];
        p = fmaf(x[n], n + i < ANB_B ? y : 0.f, p);
    }
    return p;
}
// the 64 partials' sum on the host; a wave runs v += shfl_xor(v, o) for the same o, which leaves these bits in every lane
inline float anb_tree(float *p) {
    for (int o = 32; o; o >>= 1)
        for (int l = 0; l < o; l++) p[l] = p[l] + p[l + o];
    return p[0];
}
PSDR_HOST_DEVICE inline bool anb_usable(float R0) { return fabsf(R0) <= FLT_MAX && R0 > ANB_R0_MIN; }
// step 2; returns the order that stands
PSDR_HOST_DEVICE inline int anb_levinson(const float *R, float *a) {
    a[0] = 1.f;
    ANB_UNROLL
    for (int j = 1; j <= ANB_P; j++) a[j] = 0.f;
    float E = R[0];
    bool live = true;
    int order = 0;
    ANB_UNROLL
    for (int i = 1; i <= ANB_P; i++) {
        float acc = R[i];
        ANB_UNROLL
        for (int j = 1; j < i; j++) acc = fmaf(a[j], R[i - j], acc);
        const float k = -acc / E;
        const float En = fmaf(k, acc, E);
        live = live && En > 0.f && En <= FLT_MAX;
        // (a'[j] and a'[i - j] are made from a[j] and a[i - j] alone: pair by pair, in place)
        ANB_UNROLL
        for (int j = 1; 2 * j <= i - 1; j++) {
            const float lo = fmaf(k, a[i - j], a[j]), hi = fmaf(k, a[j], a[i - j]);
            a[j] = live ? lo : a[j], a[i - j] = live ? hi : a[i - j];
        }
        if (i % 2 == 0) a[i / 2] = live ? fmaf(k, a[i / 2], a[i / 2]) : a[i / 2];
        a[i] = live ? k : a[i];
        E = live ? En : E;
        order = live ? i : order;
    }
    return order;
}
// step 3: x -> sample n of the input, e -> e[n]
PSDR_HOST_DEVICE inline float anb_residual(const float *a, const float *x) {
    float e = x[0];
    ANB_UNROLL
    for (int j = 1; j <= ANB_P; j++) e = fmaf(a[j], x[-j], e);
    return e;
}
PSDR_HOST_DEVICE inline float anb_matched(const float *a, const float *e) {
    float m = e[0];
    ANB_UNROLL
    for (int j = 1; j <= ANB_P; j++) m = fmaf(a[j], e[j], m);
    return m;
}
// step 4: from the sums
PSDR_HOST_DEVICE inline float anb_mean(float S) { return S * (1.f / ANB_B); }
PSDR_HOST_DEVICE inline float anb_dev2(float m, float mean, float acc) {
    const float d = m - mean;
    return fmaf(d, d, acc);
}
PSDR_HOST_DEVICE inline float anb_level(float V, float threshold) { return threshold * sqrtf(V * (1.f / ANB_B)); }
// step 6: xg -> the gap's first input sample (P samples on either side of the gap are read), out[width] the repaired gap
PSDR_HOST_DEVICE inline void anb_repair(const float *a, const float *xg, int width, float *out) {
    float h[ANB_P];  // h[j - 1]: f[i - j]
    ANB_UNROLL
    for (int j = 0; j < ANB_P; j++) h[j] = xg[-1 - j];
    ANB_ROLLED
    for (int i = 0; i < width; i++) {
        float acc = 0.f;
        ANB_UNROLL
        for (int j = 1; j <= ANB_P; j++) acc = fmaf(a[j], h[j - 1], acc);
        const float f = -acc;
        out[i] = f;
        ANB_UNROLL
        for (int j = ANB_P - 1; j > 0; j--) h[j] = h[j - 1];
        h[0] = f;
    }
    ANB_UNROLL
    for (int j = 0; j < ANB_P; j++) h[j] = xg[width + j];  // h[j - 1]: b[i + j]
    const float span = (float)(width - 1);
    ANB_ROLLED
    for (int i = width - 1; i >= 0; i--) {
        float acc = 0.f;
        ANB_UNROLL
        for (int j = 1; j <= ANB_P; j++) acc = fmaf(a[j], h[j - 1], acc);
        const float b = -acc;
        const float w = (float)i / span, u = 1.f - w;
        out[i] = fmaf(w, b, anb_mul(u, out[i]));
        ANB_UNROLL
        for (int j = ANB_P - 1; j > 0; j--) h[j] = h[j - 1];
        h[0] = b;
    }
}
// the samples of centre c's gap that lie in the stream (c: the stream's index), for the samples total
PSDR_HOST_DEVICE inline int anb_gap_samples(int64_t c, int width) {
    const int pl = (width - 1) / 2;
    return c >= pl ? width : width - (int)(pl - c);
}

// One block on the host.  x -> the block's first input sample, with E samples readable on either side; centres (relative to the
// block) and rep[k][i], the repaired gaps; returns the number of centres.  order, level: what steps 2 and 4 gave (may be null)
inline int anb_block(const AnbEntry &en, const float *x, int *centres, float (*rep)[ANB_WMAX], int *order = nullptr, float *level = nullptr,
                     float *mout = nullptr) {
    float R[ANB_P + 1], a[ANB_P + 1], p[64];
    for (int i = 0; i <= ANB_P; i++) {
        for (int l = 0; l < 64; l++) p[l] = anb_corr_partial(x, l, i);
        R[i] = anb_tree(p);
    }
    if (order) *order = -1;
    if (level) *level = 0.f;
    if (!anb_usable(R[0])) return 0;
    const int ord = anb_levinson(R, a);
    if (order) *order = ord;
    float e[ANB_B + ANB_P], m[ANB_B];
    for (int n = 0; n < ANB_B + ANB_P; n++) e[n] = anb_residual(a, x + n);
    for (int n = 0; n < ANB_B; n++) m[n] = anb_matched(a, e + n);
    if (mout)
        for (int n = 0; n < ANB_B; n++) mout[n] = m[n];
    for (int l = 0; l < 64; l++) p[l] = ((m[l] + m[l + 64]) + m[l + 128]) + m[l + 192];
    const float mean = anb_mean(anb_tree(p));
    for (int l = 0; l < 64; l++) {
        float v = 0.f;
        for (int r = 0; r < 4; r++) v = anb_dev2(m[l + 64 * r], mean, v);
        p[l] = v;
    }
    const float T = anb_level(anb_tree(p), en.threshold);
    if (level) *level = T;
    const int pl = (en.width - 1) / 2;
    int cnt = 0;
    for (int n = 0; n < ANB_B && cnt < ANB_MAX;) {
        if (fabsf(m[n]) > T) {
            centres[cnt] = n;
            anb_repair(a, x + n - pl, en.width, rep[cnt]);
            cnt++;
            n += pl + 1;
        } else {
            n++;
        }
    }
    return cnt;
}

// ---- the stream ---------------------------------------------------------------------------------------------------------------
// the blocks whose input is complete after T samples: (b + 1) B + E <= T
PSDR_HOST_DEVICE inline int64_t anb_blocks_done(uint64_t T) { return T < (uint64_t)(ANB_B + ANB_E) ? 0 : (int64_t)((T - ANB_B - ANB_E) / ANB_B) + 1; }
// the first block a batch that starts at T derives (again): the one whose successor holds processed sample T - D - G
PSDR_HOST_DEVICE inline int64_t anb_first_block(uint64_t T) { return T < (uint64_t)(ANB_D + ANB_G) ? 0 : (int64_t)((T - ANB_D - ANB_G) / ANB_B); }

// what the host program may report of every block a batch derives for the first time
struct AnbTrace {
    std::vector<int64_t> centres;  // the stream's indices
    std::vector<int> orders;       // per block (-1: R[0] not usable)
    std::vector<float> levels;     // per block: T
    std::vector<float> m;          // per block: 256 values (zeros where R[0] is not usable)
};
// A client's batch on the host, as k_audio_nb runs it: rows[nframes * h] in place, flags[nframes] the frames' NaN flags, st
// carried.  The batch derives blocks [anb_first_block(T), anb_blocks_done(T + L)) from hist ++ rows - the first of them again, for
// the gaps that reach the samples now due - and applies their gaps in the order of the centres onto a copy of the input.
inline void anb_stream(const AnbEntry &en, float *rows, const int *flags, int h, int nframes, AnbState &st, AnbTrace *trace = nullptr) {
    const int64_t T = (int64_t)st.pos, L = (int64_t)nframes * h;
    std::vector<float> X((size_t)(ANB_H + L + ANB_E), 0.f);  // stream samples [T - H, T + L), zeros behind
    for (int i = 0; i < ANB_H; i++) X[i] = st.hist[st.cur & 1][i];
    for (int64_t p = 0; p < L; p++) X[ANB_H + p] = flags[p / h] ? 0.f : rows[p];
    const int64_t qF = anb_first_block(st.pos), qL = anb_blocks_done(st.pos + (uint64_t)L), q0 = anb_blocks_done(st.pos);
    std::vector<float> Y(X);  // the processed samples, in X's coordinates
    const int pl = (en.width - 1) / 2;
    for (int64_t q = qF; q < qL; q++) {
        const int64_t at = q * ANB_B - (T - ANB_H);  // the block's first sample in X: >= E
        int centres[ANB_MAX], order = -1;
        float rep[ANB_MAX][ANB_WMAX], level = 0.f;
        std::vector<float> m(ANB_B, 0.f);
        const int cnt = anb_block(en, X.data() + at, centres, rep, &order, &level, m.data());
        for (int k = 0; k < cnt; k++)
            for (int i = 0; i < en.width; i++) Y[(size_t)(at + centres[k] - pl + i)] = rep[k][i];
        if (q < q0) continue;  // derived before: counted then
        for (int k = 0; k < cnt; k++) st.impulses++, st.samples += (uint64_t)anb_gap_samples(q * ANB_B + centres[k], en.width);
        if (trace) {
            for (int k = 0; k < cnt; k++) trace->centres.push_back(q * ANB_B + centres[k]);
            trace->orders.push_back(order), trace->levels.push_back(level);
            trace->m.insert(trace->m.end(), m.begin(), m.end());
        }
    }
    for (int64_t p = 0; p < L; p++) {
        if (flags[p / h]) continue;
        const int64_t j = T + p - ANB_D;
        rows[p] = j < 0 ? 0.f : Y[(size_t)(j - (T - ANB_H))];
    }
    for (int i = 0; i < ANB_H; i++) st.hist[(st.cur & 1) ^ 1][i] = X[(size_t)(L + i)];
    st.cur ^= 1;
    st.pos += (uint64_t)L;
}

// ---- the call -----------------------------------------------------------------------------------------------------------------
// psdr_client_set_audio_blanker's refusals, in the order they are looked for; on = 0 ignores the numbers, and an IQ client may
// switch it off
enum AnbVerdict { ANB_OK, ANB_BAD_ID, ANB_INACTIVE, ANB_IQ, ANB_NONFINITE, ANB_BAD_THRESHOLD, ANB_BAD_WIDTH };
inline AnbVerdict anb_check(const AudioSlot *slots, size_t S, int id, int on, double threshold, int width) {
    if (id < 0 || (size_t)id >= S) return ANB_BAD_ID;
    if (!slots[id].active) return ANB_INACTIVE;
    if (!on) return ANB_OK;
    if (slots[id].mode == PSDR_IQ) return ANB_IQ;
    if (!std::isfinite(threshold)) return ANB_NONFINITE;
    if (threshold < ANB_THR_MIN || threshold > ANB_THR_MAX) return ANB_BAD_THRESHOLD;
    if (width < ANB_WIDTH_MIN || width > ANB_WMAX || width % 2 == 0) return ANB_BAD_WIDTH;
    return ANB_OK;
}
// ... and what an accepted call does to the slot: switching it ON - from off, or again with other numbers - starts the state
// from zero at the client's next listed batch (also while paused)
inline void anb_apply(AudioSlot &s, int on, double threshold, int width) {
    s.anb_on = on ? 1 : 0;
    if (!on) return;
    s.anb_threshold = (float)threshold, s.anb_width = width;
    s.anb_fresh = true;
}
// psdr_audio_blanker_preset
inline bool anb_preset(int kind, double *threshold, int *width) {
    switch (kind) {
    case PSDR_ANB_LIGHT: *threshold = 6.0, *width = 5; return true;
    case PSDR_ANB_NORMAL: *threshold = 4.5, *width = 7; return true;
    case PSDR_ANB_STRONG: *threshold = 3.5, *width = 11; return true;
    }
    return false;
}

// ---- the batch ----------------------------------------------------------------------------------------------------------------
struct AnbPlan {
    int n = 0;                 // table[0, n): the batch's blanker clients, in slot order
    std::vector<size_t> zero;  // slots whose state starts this batch from zero
    bool any() const { return n > 0; }  // no such client in the batch: nothing is uploaded, zeroed or launched
};
// One batch, behind demod_plan(), by nr_plan()'s rule: listed are the batch's clients with the blanker on whose kind wrote audio
// rows.  The state starts from zero when the call switched it on since the client's last listed batch (anb_fresh), on a mode
// change and on a retune: when the mode, [l, r) or floor(audio_mid) are not those of its last listed batch.  An IQ client and a
// paused one keep setting, state and a pending fresh start.
inline AnbPlan anb_plan(AudioSlot *slots, size_t S, uint64_t demod_seq, AnbEntry *table) {
    AnbPlan p;
    for (size_t i = 0; i < S; i++) {
        AudioSlot &s = slots[i];
        if (!s.active || s.paused || s.last_seq != demod_seq || s.b_mode == PSDR_IQ || !s.anb_on) continue;
        const int m = (int)std::floor(s.b_mid);
        if (s.anb_fresh || s.anb_mode != s.b_mode || s.anb_l != s.b_l || s.anb_r != s.b_r || s.anb_m != m) p.zero.push_back(i);
        s.anb_fresh = false;
        s.anb_mode = s.b_mode, s.anb_l = s.b_l, s.anb_r = s.b_r, s.anb_m = m;
        table[p.n++] = AnbEntry{(int)i, s.anb_threshold, s.anb_width, 0};
    }
    return p;
}

}  // namespace psdr

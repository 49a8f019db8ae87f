// nrplan.h - the per-client noise reduction (include/psdr.h: psdr_client_set_noise_reduction), everything of it that is not a
// launch: the ONE definition of the windowed transform pair, of the per-bin gain rule and of the stream's bookkeeping (k_audio_nr
// in nr.h and the host tests run this text), the tables, the argument validation, the presets and nr_plan(), which walks the audio
// slots behind demod_plan() and says who is listed in the batch and whose state starts from zero.  Plain C++17 (no HIP):
// tests/test_nr_host.py builds it with the host compiler.
//
// The rule.  A client's stream is its audio rows in frame order (a flagged frame enters as zeros and its row is left alone, as in
// af_stream).  Block b covers stream samples [b R, b R + M), M = 256, R = 128; it is multiplied by the periodic square-root Hann
// window, transformed by a 256-point complex transform (imaginary parts zero), its bins k = 0..128 go through nr_bin(), the
// applied gain of bin min(k, 256 - k) multiplies all 256 bins, the inverse transform's real part is multiplied by the window again
// and overlap-added.  Output sample i of the stream is the overlap-added sample i - M: a fixed delay of M samples, the first M
// outputs +0.0.
//
// The transform is one radix-4 Stockham network of four stages over the table W_256^k: in stage s (Ns = 4^s) butterfly j = 0..63
// reads points j + 64 r, r = 0..3, multiplies points 1..3 by W_256^(r (j mod Ns) 64 / Ns) (stages 1..3; stage 0 has no multiply)
// and writes (j / Ns) 4 Ns + j mod Ns + r Ns.  The inverse is the same network on the data with real and imaginary parts swapped,
// and 1 / 256 as a lone multiply.  Every operation is an explicit fmaf, a lone multiply, or an add or a subtract none of whose
// operands is a multiply's result (nr_mul): contraction (-ffp-contract) has nothing to fuse, so the host and the device give the
// same bits.
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

namespace psdr {

constexpr int NR_M = 256;      // block length
constexpr int NR_R = 128;      // hop
constexpr int NR_BINS = 129;   // bins of a real block's transform
constexpr int NR_PAD = 132;    // ... as the state and the kernel's buffers hold them
constexpr int NR_STAGES = 4;   // 256 = 4^4
// design constants of the gain rule (include/psdr.h has them in words)
constexpr float NR_A_S = 0.5f;        // power smoothing
constexpr float NR_A_DN = 0.25f;      // the noise track follows a falling power
constexpr double NR_UP_SECONDS = 3.0; // ... and a rising one with this time constant
constexpr float NR_A_G_UP = 0.5f;     // gain smoothing: the faster rise keeps speech onsets
constexpr float NR_A_G_DN = 0.25f;
constexpr double NR_DEPTH_MIN = 0.0, NR_DEPTH_MAX = 40.0, NR_BETA_MIN = 0.5, NR_BETA_MAX = 4.0;

// The tables of the plan, computed in double and rounded once: win[n] = sqrt(0.5 - 0.5 cos(2 pi n / 256)) = sin(pi n / 256), both
// the analysis and the synthesis window (their product is the periodic Hann window, which sums to 1 at hop 128);
// tw[k] = W_256^k = (cos(2 pi k / 256), -sin(2 pi k / 256))
struct NrTables {
    float win[NR_M];
    float tw[NR_M][2];
};
inline void nr_tables(NrTables &t) {
    for (int n = 0; n < NR_M; n++) {
        t.win[n] = (float)std::sin(M_PI * n / NR_M);
        t.tw[n][0] = (float)std::cos(2.0 * M_PI * n / NR_M);
        t.tw[n][1] = (float)-std::sin(2.0 * M_PI * n / NR_M);
    }
}
// One entry of the batch's table: a listed client's slot and rounded parameters
struct NrEntry {
    int slot;
    float g_min, beta, a_up;
};
// What a client carries from batch to batch.  With T = pos samples taken so far, nb = T < M ? 0 : (T - M) / R + 1 blocks are
// done: tail holds the unconsumed input [nb R, T) (fewer than M samples, flagged frames as zeros), ola the last block's second
// half, pend the finished outputs that are not due yet - output samples [T, M + nb R), at most R of them, none while nb = 0 - and
// Ps, N, G the bins' records.  All zero: the start.
struct NrState {
    float tail[NR_M], ola[NR_R], pend[NR_R];
    float Ps[NR_PAD], N[NR_PAD], G[NR_PAD];
    uint64_t pos, pad;
};
static_assert(sizeof(NrEntry) == 16 && sizeof(NrState) == 3648 && sizeof(NrTables) == 3072, "the device tables' layout");

struct NrC {
    float re, im;
};

// ---- the transform ------------------------------------------------------------------------------------------------------------
// a (wr + i wi)
PSDR_HOST_DEVICE inline NrC nr_cmul(NrC a, float wr, float wi) {
    NrC o;
    o.re = fmaf(a.re, wr, -(a.im * wi));
    o.im = fmaf(a.re, wi, a.im * wr);
    return o;
}
// butterfly j of stage s, in place on its four points: the twiddles (stages 1..3), then the 4-point transform
PSDR_HOST_DEVICE inline void nr_butterfly(int s, int j, NrC *v, const float (*tw)[2]) {
    if (s > 0) {
        const int k = (j & ((1 << (2 * s)) - 1)) * (64 >> (2 * s));
        for (int r = 1; r < 4; r++) v[r] = nr_cmul(v[r], tw[r * k][0], tw[r * k][1]);
    }
    NrC a0, a1, a2, a3;
    a0.re = v[0].re + v[2].re, a0.im = v[0].im + v[2].im;
    a1.re = v[0].re - v[2].re, a1.im = v[0].im - v[2].im;
    a2.re = v[1].re + v[3].re, a2.im = v[1].im + v[3].im;
    a3.re = v[1].re - v[3].re, a3.im = v[1].im - v[3].im;
    v[0].re = a0.re + a2.re, v[0].im = a0.im + a2.im;
    v[2].re = a0.re - a2.re, v[2].im = a0.im - a2.im;
    v[1].re = a1.re + a3.im, v[1].im = a1.im - a3.re;  // a1 - i a3
    v[3].re = a1.re - a3.im, v[3].im = a1.im + a3.re;  // a1 + i a3
}
// where point r of butterfly j of stage s goes (it is read from j + 64 r); behind the last stage this is j + 64 r again: the
// butterfly that wrote a bin is the one that reads it in the next transform's first stage
PSDR_HOST_DEVICE inline int nr_out_index(int s, int j, int r) {
    const int Ns = 1 << (2 * s);
    return (j / Ns) * 4 * Ns + (j & (Ns - 1)) + r * Ns;
}
// the whole network on the host: x[256] in place
inline void nr_fft(NrC *x, const float (*tw)[2]) {
    NrC y[NR_M];
    for (int s = 0; s < NR_STAGES; s++) {
        for (int j = 0; j < 64; j++) {
            NrC v[4] = {x[j], x[j + 64], x[j + 128], x[j + 192]};
            nr_butterfly(s, j, v, tw);
            for (int r = 0; r < 4; r++) y[nr_out_index(s, j, r)] = v[r];
        }
        for (int i = 0; i < NR_M; i++) x[i] = y[i];
    }
}
// a sample into the forward transform, and out of the inverse one (the inverse's real part is the imaginary part of the
// network's output on swapped data)
// A product that an add or a subtract takes next - the first stage's inputs, the overlap-add's - is written fmaf(a, b, +0.0): the
// rounded product (a -0.0 becomes +0.0), and no multiply that contraction could fuse with the add behind it
PSDR_HOST_DEVICE inline float nr_mul(float a, float b) { return fmaf(a, b, 0.f); }
PSDR_HOST_DEVICE inline float nr_window_in(float x, float w) { return nr_mul(x, w); }
PSDR_HOST_DEVICE inline float nr_window_out(float im, float w) { return nr_mul(im * (1.f / NR_M), w); }
// the bin whose gain bin kk of the 256 takes
PSDR_HOST_DEVICE inline int nr_mirror(int kk) { return kk <= NR_M / 2 ? kk : NR_M - kk; }

// ---- the gain rule ------------------------------------------------------------------------------------------------------------
PSDR_HOST_DEVICE inline float nr_power(float re, float im) { return fmaf(re, re, im * im); }
// Steps 2 to 5 and 7 for one bin of one block; first: the stream's first block, which sets N = Ps = P and G = g (the gain starts
// on its target, inside [g_min, 1]).  Returns what the bin hands to the smoothing across bins: its G, or -g_min where P is not
// finite - that bin's records stand, it is given g_min itself and counts as g_min to its neighbours.
PSDR_HOST_DEVICE inline float nr_bin(float P, bool first, float g_min, float beta, float a_up, float &Ps, float &N, float &G) {
    if (!(fabsf(P) <= FLT_MAX)) return -g_min;
    if (first) {
        Ps = P, N = P;
    } else {
        Ps = fmaf(NR_A_S, P - Ps, Ps);
        N = fmaf(Ps < N ? NR_A_DN : a_up, Ps - N, N);
    }
    float g = g_min;
    if (Ps > 0.f) {
        g = 1.f - (beta * N) / Ps;
        g = !(g >= g_min) ? g_min : g;
        g = g > 1.f ? 1.f : g;
    }
    G = first ? g : fmaf(g > G ? NR_A_G_UP : NR_A_G_DN, g - G, G);
    return G;
}
// Step 6: B[129] as nr_bin returned it; (B[k-1] + 2 B[k] + B[k+1]) / 4 as 0.25 * (fma(2, B[k], B[k-1]) + B[k+1]), the edge bins
// mirrored (k = 0 takes B[1] twice, k = 128 B[127]), kept inside [g_min, 1] (the two roundings may leave it by an ulp)
PSDR_HOST_DEVICE inline float nr_applied(const float *B, int k, float g_min) {
    if (B[k] < 0.f) return g_min;
    const float m = fabsf(B[k == 0 ? 1 : k - 1]), p = fabsf(B[k == NR_BINS - 1 ? NR_BINS - 2 : k + 1]);
    float a = 0.25f * (fmaf(2.f, B[k], m) + p);
    a = a < g_min ? g_min : a;
    return a > 1.f ? 1.f : a;
}
// the overlap-add: the earlier block's second half, then the later block's first
PSDR_HOST_DEVICE inline float nr_ola(float earlier, float later) { return earlier + later; }

// One block on the host: x[256] of the stream, s[256] the windowed inverse; applied: the 129 applied gains (may be null)
inline void nr_block(const NrTables &t, const NrEntry &e, bool first, const float *x, NrState &st, float *s, float *applied = nullptr) {
    NrC X[NR_M];
    for (int i = 0; i < NR_M; i++) X[i].re = nr_window_in(x[i], t.win[i]), X[i].im = 0.f;
    nr_fft(X, t.tw);
    float B[NR_BINS], a[NR_BINS];
    for (int k = 0; k < NR_BINS; k++) B[k] = nr_bin(nr_power(X[k].re, X[k].im), first, e.g_min, e.beta, e.a_up, st.Ps[k], st.N[k], st.G[k]);
    for (int k = 0; k < NR_BINS; k++) a[k] = nr_applied(B, k, e.g_min);
    if (applied)
        for (int k = 0; k < NR_BINS; k++) applied[k] = a[k];
    for (int i = 0; i < NR_M; i++) {
        const float g = a[nr_mirror(i)];
        const NrC z = {nr_mul(X[i].im, g), nr_mul(X[i].re, g)};  // (swapped)
        X[i] = z;
    }
    nr_fft(X, t.tw);
    for (int i = 0; i < NR_M; i++) s[i] = nr_window_out(X[i].im, t.win[i]);
}

// ---- the stream ---------------------------------------------------------------------------------------------------------------
// the blocks done after T samples
PSDR_HOST_DEVICE inline uint64_t nr_blocks_done(uint64_t T) { return T < (uint64_t)NR_M ? 0 : (T - NR_M) / NR_R + 1; }
// A client's batch on the host, as k_audio_nr runs it: rows[nframes * h] in place, flags[nframes] the frames' NaN flags, st
// carried.  In the batch's own coordinates u = stream index - nb0 R the input is X(u) = tail ++ rows for u in [0, U), the batch
// finishes blocks q = 0 .. nbn - 1 and with them Y(u), u in [0, nbn R); output p of the rows is Y(t0 + p - M), or what was pending.
// gains: if not null, the applied gains of every block the batch finishes are appended (129 each).
inline void nr_stream(const NrTables &t, const NrEntry &e, float *rows, const int *flags, int h, int nframes, NrState &st,
                      std::vector<float> *gains = nullptr) {
    const long L = (long)nframes * h;
    const uint64_t nb0 = nr_blocks_done(st.pos);
    const long t0 = (long)(st.pos - nb0 * NR_R), U = t0 + L;
    const long nbn = U >= NR_M ? (U - NR_M) / NR_R + 1 : 0;
    std::vector<float> X((size_t)U), Y((size_t)(nbn * NR_R));
    for (long u = 0; u < U; u++) X[u] = u < t0 ? st.tail[u] : (flags[(u - t0) / h] ? 0.f : rows[u - t0]);
    float s[NR_M], a[NR_BINS];
    for (long q = 0; q < nbn; q++) {
        nr_block(t, e, nb0 + (uint64_t)q == 0, X.data() + q * NR_R, st, s, a);
        if (gains) gains->insert(gains->end(), a, a + NR_BINS);
        for (int i = 0; i < NR_R; i++) Y[q * NR_R + i] = nr_ola(st.ola[i], s[i]), st.ola[i] = s[NR_R + i];
    }
    // what is due, or pending, at output p (p < L: a row's sample; behind it: the new pending ones)
    auto out = [&](long p) {
        const long u = t0 + p - NR_M;
        return u >= 0 ? Y[u] : (nb0 ? st.pend[p] : 0.f);
    };
    for (long p = 0; p < L; p++)
        if (!flags[p / h]) rows[p] = out(p);
    float pend[NR_R] = {};
    if (nb0 + (uint64_t)nbn > 0)
        for (long i = 0; i < NR_M - (U - nbn * NR_R); i++) pend[i] = out(L + i);
    for (int i = 0; i < NR_R; i++) st.pend[i] = pend[i];
    float tail[NR_M] = {};
    for (long u = nbn * NR_R; u < U; u++) tail[u - nbn * NR_R] = X[u];
    for (int i = 0; i < NR_M; i++) st.tail[i] = tail[i];
    st.pos += (uint64_t)L;
}

// ---- the call -----------------------------------------------------------------------------------------------------------------
// psdr_client_set_noise_reduction's refusals, in the order they are looked for; on = 0 ignores depth_db and beta, and an IQ client
// may switch it off
enum NrVerdict { NR_OK, NR_BAD_ID, NR_INACTIVE, NR_IQ, NR_NONFINITE, NR_BAD_DEPTH, NR_BAD_BETA, NR_NO_RATE };
inline NrVerdict nr_check(const AudioSlot *slots, size_t S, int id, int on, double depth_db, double beta, int audio_rate) {
    if (id < 0 || (size_t)id >= S) return NR_BAD_ID;
    if (!slots[id].active) return NR_INACTIVE;
    if (!on) return NR_OK;
    if (slots[id].mode == PSDR_IQ) return NR_IQ;
    if (!std::isfinite(depth_db) || !std::isfinite(beta)) return NR_NONFINITE;
    if (depth_db < NR_DEPTH_MIN || depth_db > NR_DEPTH_MAX) return NR_BAD_DEPTH;
    if (beta < NR_BETA_MIN || beta > NR_BETA_MAX) return NR_BAD_BETA;
    if (audio_rate <= 0) return NR_NO_RATE;
    return NR_OK;
}
// the noise track's rising coefficient: a time constant of NR_UP_SECONDS at one block per R samples
inline float nr_a_up(int audio_rate) { return (float)(1.0 - std::exp(-(double)NR_R / (NR_UP_SECONDS * (double)audio_rate))); }
inline float nr_g_min(double depth_db) { return (float)std::pow(10.0, -depth_db / 20.0); }
// ... and what an accepted call does to the slot: switching it ON - from off, or again with other numbers - starts the state
// from zero at the client's next listed batch (also while paused)
inline void nr_apply(AudioSlot &s, int on, double depth_db, double beta) {
    s.nr_on = on ? 1 : 0;
    if (!on) return;
    s.nr_g_min = nr_g_min(depth_db), s.nr_beta = (float)beta;
    s.nr_fresh = true;
}
// psdr_noise_reduction_preset
inline bool nr_preset(int kind, double *depth_db, double *beta) {
    switch (kind) {
    case PSDR_NR_LIGHT: *depth_db = 8.0, *beta = 1.0; return true;
    case PSDR_NR_NORMAL: *depth_db = 14.0, *beta = 1.5; return true;
    case PSDR_NR_STRONG: *depth_db = 22.0, *beta = 2.0; return true;
    }
    return false;
}

// ---- the batch ----------------------------------------------------------------------------------------------------------------
struct NrPlan {
    int n = 0;                 // table[0, n): the batch's noise-reduction clients, in slot order
    std::vector<size_t> zero;  // slots whose state starts this batch from zero
    bool any() const { return n > 0; }  // no such client in the batch: nothing is uploaded, zeroed or launched
};
// One batch, behind demod_plan(): the clients it demodulated are those whose last_seq is the batch's demod_seq, with b_l, b_r,
// b_mid and b_mode what they were demodulated with.  Of these the ones with noise reduction on whose kind wrote audio rows are
// listed.  The state starts from zero when the call switched it on since the client's last listed batch (nr_fresh, as af_fresh),
// on a mode change and on a retune: when the mode, [l, r) or floor(audio_mid) are not those of its last listed batch.  An IQ
// client and a paused one keep setting, state and a pending fresh start.
inline NrPlan nr_plan(AudioSlot *slots, size_t S, uint64_t demod_seq, NrEntry *table, float a_up) {
    NrPlan p;
    for (size_t i = 0; i < S; i++) {
        AudioSlot &s = slots[i];
        if (!s.active || s.paused || s.last_seq != demod_seq || s.b_mode == PSDR_IQ || !s.nr_on) continue;
        const int m = (int)std::floor(s.b_mid);
        if (s.nr_fresh || s.nr_mode != s.b_mode || s.nr_l != s.b_l || s.nr_r != s.b_r || s.nr_m != m) p.zero.push_back(i);
        s.nr_fresh = false;
        s.nr_mode = s.b_mode, s.nr_l = s.b_l, s.nr_r = s.b_r, s.nr_m = m;
        table[p.n++] = NrEntry{(int)i, s.nr_g_min, s.nr_beta, a_up};
    }
    return p;
}

}  // namespace psdr

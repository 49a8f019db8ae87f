// toneplan.h - the per-client tone decoder (include/psdr.h: psdr_client_set_tone_decoder), everything of it that is not a launch:
// the ONE definition of the phase-to-twiddle rule, of the block correlation, the window sum, the decision and the stream's
// bookkeeping (k_audio_tone in tone.h and the host tests run this text), the tables, the argument validation, the defaults and
// tone_plan(), which walks the audio slots behind demod_plan() and says who is listed in the batch, whose state starts from zero
// and whose drop flags are copied.  Plain C++17 (no HIP): tests/test_tone_host.py builds it with the host compiler.
//
// The rule.  A client's stream is its audio rows in frame order as the demodulator wrote them (a flagged frame enters as zeros),
// sample t counting from the state's start.  Tone k has the phase increment inc_k = round(f_k / audio_rate * 2^32); the phase of
// sample t is the low 32 bits of inc_k t.  Block b covers samples [256 b, 256 b + 256).  Its twiddle starts at
// w = coarse[phase >> 20] * fine[(phase >> 8) & 4095] with phase = phase(256 b) - two tables of 4096 entries, exp(2 pi i j / 2^12)
// and exp(2 pi i j / 2^24), the low 8 bits of the phase dropped (3.7e-7 rad at most) - and goes on by w <- w * rot_k,
// rot_k = exp(2 pi i inc_k / 2^32), once per sample.  C[b][k] = sum_n x[256 b + n] conj(w_n), n ascending, one accumulator.
// Every operation is an explicit fmaf or a lone multiply: contraction (-ffp-contract) has nothing to fuse, so the host and the
// device give the same bits.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <cfloat>
#include <cmath>
#include <vector>

#include "demodplan.h"
#include "squelchplan.h"

#ifndef PSDR_HOST_DEVICE
#if defined(__HIPCC__)
#define PSDR_HOST_DEVICE __host__ __device__
#else
#define PSDR_HOST_DEVICE
#endif
#endif

namespace psdr {

constexpr int TONE_N = PSDR_TONE_COUNT;  // the standard tones
constexpr int TONE_LANES = 64;           // ... as the tables, the history and the kernel hold them: lane = tone
constexpr int TONE_B = 256;              // block length
constexpr int TONE_TAB = 4096;           // entries of either twiddle table
constexpr int TONE_REF_RANK = 12;        // ref: the 12th smallest (0-based) of the 50 powers, the lower quartile
constexpr int TONE_GROUP = 4;            // blocks the kernel derives at once, one per wave
constexpr int TONE_RATE_MIN = 2000, TONE_RATE_MAX = 48000;
constexpr int TONE_NB_MAX = 75;          // the window's blocks at TONE_RATE_MAX
constexpr double TONE_SNR_MIN = 6.0, TONE_SNR_MAX = 60.0, TONE_SNR_DEFAULT = 22.0;
constexpr int TONE_BLOCKS_MAX = 1024;    // attack_blocks 1..1024, hang_blocks 0..1024

// the 50 standard tones in Hz, ascending: index = the tone's number
static const double TONE_HZ[TONE_N] = {67.0,  69.3,  71.9,  74.4,  77.0,  79.7,  82.5,  85.4,  88.5,  91.5,  94.8,  97.4,  100.0,
                                       103.5, 107.2, 110.9, 114.8, 118.8, 123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7,
                                       159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9, 183.5, 186.2, 189.9, 192.8, 196.6,
                                       199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1};

// NB = ceil(0.4 audio_rate / 256), as 2 rate / 1280 so that no rounding of 0.4 decides it: 13, 19, 75 at 8, 12, 48 kHz
inline int tone_nb(double audio_rate) { return (int)std::ceil(2.0 * audio_rate / 1280.0); }
// the history ring's rows per slot: the NB - 1 blocks behind the newest one and the group the kernel derives at once
inline int tone_ring(int nb) { return nb - 1 + TONE_GROUP; }

struct ToneC {
    float re, im;
};
// The tables of the plan, computed in double and rounded once.  inc, rot: per tone (lanes 50..63: 0 and 1); h: the window,
// h_j = 0.5 - 0.5 cos(2 pi (j + 0.5) / NB); lscale = 4 / (256 sum h)^2 with the sum over the rounded h in double: level = P lscale
struct ToneTables {
    float coarse[TONE_TAB][2], fine[TONE_TAB][2];
    uint32_t inc[TONE_LANES];
    float rot[TONE_LANES][2];
    float h[TONE_NB_MAX + 1];
    int nb;
    float lscale;
};
// the two seed tables and one lane's increment and rotation (hz <= 0: a lane without a tone, 0 and 1): the CW decoder's lanes
// (cwplan.h) are made by the same two functions
inline void tone_seed_tables(ToneTables &t) {
    for (int j = 0; j < TONE_TAB; j++) {
        const double a = 2.0 * M_PI * j / 4096.0, b = 2.0 * M_PI * j / 16777216.0;
        t.coarse[j][0] = (float)std::cos(a), t.coarse[j][1] = (float)std::sin(a);
        t.fine[j][0] = (float)std::cos(b), t.fine[j][1] = (float)std::sin(b);
    }
}
// (the RTTY decoder's lanes are the client's own: rttyplan.h keeps them in the batch's table, made by tone_inc_rot)
inline void tone_inc_rot(double hz, double audio_rate, uint32_t &inc, float *rot) {
    inc = hz > 0 ? (uint32_t)std::floor(hz / audio_rate * 4294967296.0 + 0.5) : 0u;
    const double a = 2.0 * M_PI * (double)inc / 4294967296.0;
    rot[0] = (float)std::cos(a), rot[1] = (float)std::sin(a);
}
inline void tone_lane(ToneTables &t, int k, double hz, double audio_rate) { tone_inc_rot(hz, audio_rate, t.inc[k], t.rot[k]); }
inline void tone_tables(ToneTables &t, double audio_rate) {
    memset(&t, 0, sizeof(t));
    tone_seed_tables(t);
    for (int k = 0; k < TONE_LANES; k++) tone_lane(t, k, k < TONE_N ? TONE_HZ[k] : 0.0, audio_rate);
    t.nb = tone_nb(audio_rate);
    double sum = 0;
    for (int j = 0; j < t.nb; j++) {
        t.h[j] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (j + 0.5) / t.nb));
        sum += (double)t.h[j];
    }
    t.lscale = (float)(4.0 / ((256.0 * sum) * (256.0 * sum)));
}
// One entry of the batch's table.  attack >= 1: a tone client.  attack == 0: an audio client WITHOUT the decoder in a post-chain
// batch that has gated tone clients - its drop flags are the previous ones, copied (the chain reads one array)
struct ToneEntry {
    int slot, want, gate, attack, hang;
    float ratio, min_level;
    int pad;
};
// What a client carries from batch to batch: the samples of the unfinished block (part[0, pos % 256)), the position, the gate
// and the last decision.  All zero is the start: the tone is kept as tone + 1.
struct ToneState {
    float part[TONE_B];
    uint64_t pos;
    int open, cnt;
    int tone_plus1;  // the last decision's tone + 1 (0: none or no hit), so that zeroed memory is the start
    float level;
};
// One frame's record
struct ToneRec {
    int tone;
    float level;
    int open, pad;
};
static_assert(sizeof(ToneEntry) == 32 && sizeof(ToneState) == 1048 && sizeof(ToneRec) == 16 && sizeof(ToneTables) == 66616 && sizeof(ToneC) == 8,
              "the device tables' layout");

// ---- the correlation ----------------------------------------------------------------------------------------------------------
PSDR_HOST_DEVICE inline ToneC tone_cmul(ToneC a, ToneC b) {
    ToneC o;
    o.re = fmaf(a.re, b.re, -(a.im * b.im));
    o.im = fmaf(a.re, b.im, a.im * b.re);
    return o;
}
// the low 32 bits of inc t, t the stream position of a block's first sample
PSDR_HOST_DEVICE inline uint32_t tone_phase(uint32_t inc, uint64_t t) { return inc * (uint32_t)t; }
PSDR_HOST_DEVICE inline ToneC tone_seed(const ToneTables *t, uint32_t phase) {
    const ToneC c = {t->coarse[phase >> 20][0], t->coarse[phase >> 20][1]};
    const ToneC f = {t->fine[(phase >> 8) & (TONE_TAB - 1)][0], t->fine[(phase >> 8) & (TONE_TAB - 1)][1]};
    return tone_cmul(c, f);
}
// one sample: acc += x conj(w), then w <- w rot
PSDR_HOST_DEVICE inline void tone_step(ToneC &acc, ToneC &w, ToneC rot, float x) {
    acc.re = fmaf(x, w.re, acc.re);
    acc.im = fmaf(-x, w.im, acc.im);
    w = tone_cmul(w, rot);
}
// C[b][k] over the block's 256 samples
PSDR_HOST_DEVICE inline ToneC tone_block(const ToneTables *t, int k, uint64_t b, const float *x) {
    ToneC w = tone_seed(t, tone_phase(t->inc[k], b * TONE_B));
    const ToneC rot = {t->rot[k][0], t->rot[k][1]};
    ToneC acc = {0.f, 0.f};
    for (int n = 0; n < TONE_B; n++) tone_step(acc, w, rot, x[n]);
    return acc;
}
// ---- the window and the decision ----------------------------------------------------------------------------------------------
PSDR_HOST_DEVICE inline void tone_window_step(ToneC &S, float h, ToneC c) {
    S.re = fmaf(h, c.re, S.re);
    S.im = fmaf(h, c.im, S.im);
}
PSDR_HOST_DEVICE inline float tone_power(ToneC S) { return fmaf(S.re, S.re, S.im * S.im); }
PSDR_HOST_DEVICE inline bool tone_finite(float P) { return fabsf(P) <= FLT_MAX; }
PSDR_HOST_DEVICE inline float tone_level(float P, float lscale) { return P * lscale; }
PSDR_HOST_DEVICE inline bool tone_hit(float Pbest, float ref, float level, int best, const ToneEntry &e) {
    return Pbest >= e.ratio * ref && level >= e.min_level && (e.want < 0 || best == e.want);
}
PSDR_HOST_DEVICE inline uint32_t tone_bits(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(v);
#else
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
#endif
}
struct ToneDecision {
    int hit, best;  // hit < 0: no decision (the window has not filled)
    float level;
};
// the decision over the 50 powers on the host (the kernel does the same with wave operations): a power that is not finite
// gives no hit and level 0; else best = the lowest k with the largest P, ref = the power of rank 12, both ordered as unsigned
// integers on the bit pattern (the powers are >= +0), ties by the lower index
inline ToneDecision tone_decide(const float *P, const ToneEntry &e, float lscale) {
    ToneDecision d = {0, 0, 0.f};
    for (int k = 0; k < TONE_N; k++)
        if (!tone_finite(P[k])) return d;
    for (int k = 1; k < TONE_N; k++)
        if (tone_bits(P[k]) > tone_bits(P[d.best])) d.best = k;
    float ref = 0.f;
    for (int k = 0; k < TONE_N; k++) {
        int rank = 0;
        for (int j = 0; j < TONE_N; j++) rank += tone_bits(P[j]) < tone_bits(P[k]) || (tone_bits(P[j]) == tone_bits(P[k]) && j < k);
        if (rank == TONE_REF_RANK) ref = P[k];
    }
    d.level = tone_level(P[d.best], lscale);
    d.hit = tone_hit(P[d.best], ref, d.level, d.best, e) ? 1 : 0;
    return d;
}
// the gate is squelch_step's state machine in units of blocks; the last decision is kept beside it
PSDR_HOST_DEVICE inline void tone_gate(SquelchState &g, int &tone_plus1, float &level, int hit, int best, float lvl, const ToneEntry &e) {
    squelch_step(g, hit != 0, hit != 0, e.attack, e.hang);
    tone_plus1 = hit ? best + 1 : 0;
    level = lvl;
}
// ---- the stream ---------------------------------------------------------------------------------------------------------------
// the first frame of a batch (frames of h samples from stream position pos0 on) at whose last sample D blocks are complete:
// the smallest f >= 0 with pos0 + (f + 1) h >= 256 D.  The frames that take the state behind block D - 1 are
// [tone_first_frame(D), tone_first_frame(D + 1)).  (256 D - pos0 is at most the batch's length + 256)
PSDR_HOST_DEVICE inline int tone_first_frame(uint64_t D, uint64_t pos0, int h) {
    const int64_t d = (int64_t)(D * TONE_B) - (int64_t)pos0;
    return d <= 0 ? 0 : ((int)d + h - 1) / h - 1;
}
// sample t of the stream during a batch that starts at pos0 with the carried partial block part (whose first sample is 256 b0)
PSDR_HOST_DEVICE inline float tone_sample(uint64_t t, uint64_t pos0, uint64_t b0, const float *part, const float *rows, const int *flags, int h) {
    if (t < pos0) return part[t - b0 * TONE_B];
    const uint32_t o = (uint32_t)(t - pos0);  // (a batch is shorter than 2^31 samples: one 32-bit division)
    return flags[o / (uint32_t)h] ? 0.f : rows[o];
}
PSDR_HOST_DEVICE inline ToneRec tone_record(const SquelchState &g, int tone_plus1, float level) { return ToneRec{tone_plus1 - 1, level, g.open, 0}; }
// the drop flag of a frame for the chain: what was dropped before, and for a gated client the closed frames
PSDR_HOST_DEVICE inline int tone_drop(int prev, int gate, int open) { return (prev != 0 || (gate && !open)) ? 1 : 0; }

// A client's batch on the host, as k_audio_tone runs it: rows[nframes * h] and flags[nframes] are read, st and hist
// ([tone_ring(nb)][64], block b in row b % ring) carried, rec[nframes] written; prev_drop / drop: [nframes] or null
inline void tone_stream(const ToneTables &t, const ToneEntry &e, const float *rows, const int *flags, int h, int nframes, ToneState &st, ToneC *hist,
                        ToneRec *rec, const int *prev_drop = nullptr, int *drop = nullptr) {
    const uint64_t pos0 = st.pos, L = (uint64_t)nframes * (uint64_t)h, b0 = pos0 / TONE_B, b1 = (pos0 + L) / TONE_B;
    const int ring = tone_ring(t.nb);
    SquelchState g = {st.open, st.cnt};
    int tp1 = st.tone_plus1;
    float level = st.level;
    auto emit = [&](uint64_t D) {  // the frames at whose end D blocks are complete
        const int lo = tone_first_frame(D, pos0, h), hi = std::min(nframes, tone_first_frame(D + 1, pos0, h));
        for (int f = lo; f < hi; f++) {
            rec[f] = tone_record(g, tp1, level);
            if (drop) drop[f] = tone_drop(prev_drop[f], e.gate, g.open);
        }
    };
    emit(b0);
    float x[TONE_B];
    for (uint64_t b = b0; b < b1; b++) {
        for (int n = 0; n < TONE_B; n++) x[n] = tone_sample(b * TONE_B + n, pos0, b0, st.part, rows, flags, h);
        ToneC *row = hist + (size_t)(b % (uint64_t)ring) * TONE_LANES;
        for (int k = 0; k < TONE_LANES; k++) row[k] = tone_block(&t, k, b, x);
        if (b + 1 >= (uint64_t)t.nb) {
            float P[TONE_N];
            for (int k = 0; k < TONE_N; k++) {
                ToneC S = {0.f, 0.f};
                for (int j = 0; j < t.nb; j++) tone_window_step(S, t.h[j], hist[(size_t)((b + 1 - t.nb + j) % (uint64_t)ring) * TONE_LANES + k]);
                P[k] = tone_power(S);
            }
            const ToneDecision d = tone_decide(P, e, t.lscale);
            tone_gate(g, tp1, level, d.hit, d.best, d.level, e);
        }
        emit(b + 1);
    }
    float part[TONE_B] = {};
    for (uint64_t u = b1 * TONE_B; u < pos0 + L; u++) part[u - b1 * TONE_B] = tone_sample(u, pos0, b0, st.part, rows, flags, h);
    memcpy(st.part, part, sizeof(part));
    st.pos = pos0 + L, st.open = g.open, st.cnt = g.cnt, st.tone_plus1 = tp1, st.level = level;
}

// ---- the call -----------------------------------------------------------------------------------------------------------------
// psdr_client_set_tone_decoder's refusals, in the order they are looked for; cfg == null switches it off (an IQ client may)
enum ToneVerdict { TONE_OK, TONE_BAD_ID, TONE_INACTIVE, TONE_IQ, TONE_BAD_WANT, TONE_BAD_GATE, TONE_BAD_SNR, TONE_BAD_LEVEL, TONE_BAD_ATTACK, TONE_BAD_HANG, TONE_BAD_RATE };
inline ToneVerdict tone_check(const AudioSlot *slots, size_t S, int id, const psdr_tone_config *cfg, int audio_rate) {
    if (id < 0 || (size_t)id >= S) return TONE_BAD_ID;
    if (!slots[id].active) return TONE_INACTIVE;
    if (!cfg) return TONE_OK;
    if (slots[id].mode == PSDR_IQ) return TONE_IQ;
    if (cfg->want < PSDR_TONE_ANY || cfg->want >= TONE_N) return TONE_BAD_WANT;
    if (cfg->gate != 0 && cfg->gate != 1) return TONE_BAD_GATE;
    if (!std::isfinite(cfg->snr_db) || cfg->snr_db < TONE_SNR_MIN || cfg->snr_db > TONE_SNR_MAX) return TONE_BAD_SNR;
    if (!std::isfinite(cfg->min_level) || cfg->min_level < 0) return TONE_BAD_LEVEL;
    if (cfg->attack_blocks < 1 || cfg->attack_blocks > TONE_BLOCKS_MAX) return TONE_BAD_ATTACK;
    if (cfg->hang_blocks < 0 || cfg->hang_blocks > TONE_BLOCKS_MAX) return TONE_BAD_HANG;
    if (audio_rate < TONE_RATE_MIN || audio_rate > TONE_RATE_MAX) return TONE_BAD_RATE;
    return TONE_OK;
}
inline float tone_ratio(double snr_db) { return (float)std::pow(10.0, snr_db / 10.0); }
// ... and what an accepted call does to the slot: switching it ON - from off, or again - starts the state from zero at the
// client's next listed batch (also while paused)
inline void tone_apply(AudioSlot &s, const psdr_tone_config *cfg) {
    s.tone_on = cfg ? 1 : 0;
    if (!cfg) return;
    s.tone_want = cfg->want, s.tone_gate = cfg->gate;
    s.tone_ratio = tone_ratio(cfg->snr_db), s.tone_min_level = (float)cfg->min_level;
    s.tone_attack = cfg->attack_blocks, s.tone_hang = cfg->hang_blocks;
    s.tone_fresh = true;
}
// psdr_tone_defaults
inline bool tone_defaults(double audio_rate, psdr_tone_config *out) {
    if (!out || !(audio_rate >= TONE_RATE_MIN && audio_rate <= TONE_RATE_MAX)) return false;
    out->want = PSDR_TONE_ANY, out->gate = 1;
    out->snr_db = TONE_SNR_DEFAULT, out->min_level = 0.0;
    out->attack_blocks = 2, out->hang_blocks = tone_nb(audio_rate);
    return true;
}

// ---- the batch ----------------------------------------------------------------------------------------------------------------
struct TonePlan {
    int n = 0;      // table[0, n): the batch's tone clients, in slot order
    int ncopy = 0;  // table[n, n + ncopy): the chain's other audio clients (attack == 0), in slot order; only with `gated`
    bool gated = false;        // the chain runs behind this batch and a listed client has gate = 1: the chain reads the tone drop array
    std::vector<size_t> zero;  // slots whose state starts this batch from zero
    bool any() const { return n > 0; }  // no such client in the batch: nothing is uploaded, zeroed or launched
};
// One batch, behind demod_plan(): nr_plan with other fields.  Of the clients the batch demodulated the ones with the decoder on
// whose kind wrote audio rows are listed; the state starts from zero when the call switched it on since the client's last listed
// batch, on a mode change and on a retune.  An IQ client and a paused one keep setting, state and a pending fresh start.
// b_tone_on: the last batch ran with the decoder for this client (psdr_read_tone).  chain: the post chain runs behind this batch.
inline TonePlan tone_plan(AudioSlot *slots, size_t S, uint64_t demod_seq, bool chain, ToneEntry *table) {
    TonePlan p;
    for (size_t i = 0; i < S; i++) {
        AudioSlot &s = slots[i];
        if (!s.active || s.paused || s.last_seq != demod_seq) continue;
        s.b_tone_on = false;
        if (s.b_mode == PSDR_IQ || !s.tone_on) continue;
        s.b_tone_on = true;
        const int m = (int)std::floor(s.b_mid);
        if (s.tone_fresh || s.tone_mode != s.b_mode || s.tone_l != s.b_l || s.tone_r != s.b_r || s.tone_m != m) p.zero.push_back(i);
        s.tone_fresh = false;
        s.tone_mode = s.b_mode, s.tone_l = s.b_l, s.tone_r = s.b_r, s.tone_m = m;
        p.gated |= chain && s.tone_gate != 0;
        table[p.n++] = ToneEntry{(int)i, s.tone_want, s.tone_gate, s.tone_attack, s.tone_hang, s.tone_ratio, s.tone_min_level, 0};
    }
    if (!p.gated) return p;
    for (size_t i = 0; i < S; i++) {
        const AudioSlot &s = slots[i];
        if (s.active && !s.paused && s.last_seq == demod_seq && !s.b_tone_on && s.b_mode != PSDR_IQ)
            table[p.n + p.ncopy++] = ToneEntry{(int)i, 0, 0, 0, 0, 0.f, 0.f, 0};
    }
    return p;
}

}  // namespace psdr

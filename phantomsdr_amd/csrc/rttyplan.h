// rttyplan.h - the per-client RTTY decoder (include/psdr.h: psdr_client_set_rtty_decoder), everything of it that is not a launch:
// the ONE definition of the hop correlation, the bit window, the pair follower, the slicer with its threshold correction, the
// presence, the framing machine, the Baudot table, the records and the stream's bookkeeping (k_audio_rtty in rtty.h and the host
// tests run this text), the tables, the argument validation, the defaults and rtty_plan(), which walks the audio slots behind
// demod_plan() and says who is listed in the batch and whose state starts from zero.  Plain C++17 (no HIP):
// tests/test_rtty_host.py builds it with the host compiler.
//
// The rule is written out in include/psdr.h.  Phases, seeds and the per-sample rotation are toneplan.h's functions; the lanes are
// the client's own (they follow mark_hz and shift_hz), so increments and rotations travel in the batch's table and the context's
// tables hold the two seed tables and the code table.  The frames of a hop, the sample of a stream and the 1/64 follower are
// cwplan.h's.  Every f32 operation is an explicit fmaf, a lone multiply, a lone add or the one division of `quality`, so
// contraction has nothing to fuse; the framing is integer arithmetic.
#pragma once
#include "cwplan.h"

namespace psdr {

constexpr int RTTY_LANES = PSDR_RTTY_LANES;  // 16 pairs: lane 2 j the mark tone of pair j, lane 2 j + 1 its space tone
constexpr int RTTY_PAIRS = RTTY_LANES / 2;
constexpr int RTTY_P0 = 8;                   // the pair on the configured tones, where the follower starts
constexpr int RTTY_GROUP = 8;                // hops the kernel correlates at once, two per wave
constexpr int RTTY_HMAX = 64;                // the longest hop
constexpr int RTTY_WMAX = 24;                // hops of correlations the state keeps: the bit window is 7 to 22 of them
constexpr int RTTY_FILL = 256;               // hops before the presence is read: one time constant of T and Nn
constexpr int RTTY_TEXT = 1024;              // characters the device keeps per slot
constexpr int RTTY_RATE_MIN = 4000, RTTY_RATE_MAX = 48000;
constexpr double RTTY_DF = 20.0;             // pair j sits 20 (j - 8) Hz off the configured tones
constexpr double RTTY_MARK_MIN = 300.0, RTTY_MARK_MAX = 3000.0, RTTY_MARK_DEFAULT = 2125.0, RTTY_MARK_LOW = 915.0;
constexpr double RTTY_SHIFT_MIN = 85.0, RTTY_SHIFT_MAX = 1000.0, RTTY_SHIFT_DEFAULT = 170.0;
constexpr double RTTY_BAUD_MIN = 45.0, RTTY_BAUD_MAX = 75.0, RTTY_BAUD_DEFAULT = 45.45;
constexpr double RTTY_SEARCH_MIN = 0.0, RTTY_SEARCH_MAX = 160.0, RTTY_SEARCH_DEFAULT = 60.0;
constexpr double RTTY_SNR_MIN = 3.0, RTTY_SNR_MAX = 30.0, RTTY_SNR_DEFAULT = PSDR_RTTY_SNR_DEFAULT;
constexpr double RTTY_EDGE = 160.0;          // what the outermost pair adds to either tone
constexpr double RTTY_TOP = 0.45, RTTY_BOTTOM = 100.0;  // the tones and their pairs stay under 0.45 audio_rate and above 100 Hz

// a hop lasts 1 to 2 ms
inline int rtty_hop(double audio_rate) { return audio_rate < 8000 ? 8 : audio_rate < 16000 ? 16 : audio_rate < 32000 ? 32 : 64; }
inline double rtty_pair_hz(int j) { return RTTY_DF * (j - RTTY_P0); }
// the bit window in hops, and the bit length in 1/16 hop: both rounded to nearest, in double
inline int rtty_wn_of(double baud, double audio_rate) {
    const int w = (int)std::floor(audio_rate / (baud * rtty_hop(audio_rate)) + 0.5);
    return w < 2 ? 2 : w;
}
inline int rtty_u_of(double baud, double audio_rate) { return (int)std::floor(16.0 * audio_rate / (baud * rtty_hop(audio_rate)) + 0.5); }
inline uint32_t rtty_candidates(double search_hz) {
    uint32_t m = 1u << RTTY_P0;
    for (int j = 0; j < RTTY_PAIRS; j++)
        if (std::fabs(rtty_pair_hz(j)) <= search_hz) m |= 1u << j;
    return m;
}

// ITA2 with the US-TTY figures, by code; 0: the code prints nothing (null, LTRS 31, FIGS 27)
static const char RTTY_LTRS[33] = "\0E\nA SIU\rDRJNFCKTZLWHYPQOBG\0MXV";
static const char RTTY_FIGS[33] = "\0" "3\n- \a87\r$4',!:(5\")2#6019?&\0./;";
constexpr int RTTY_CODE_LTRS = 31, RTTY_CODE_FIGS = 27, RTTY_CODE_SPACE = 4;

// The tables of the context: the seed tables (of t, inc, rot, h, nb and lscale are not used) and the characters by shift and code
struct RttyTables {
    ToneTables t;
    uint8_t baudot[2][32];
    int H, pad;
};
inline void rtty_tables(RttyTables &c, double audio_rate) {
    memset(&c, 0, sizeof(c));
    tone_seed_tables(c.t);
    for (int k = 0; k < 32; k++) c.baudot[0][k] = (uint8_t)RTTY_LTRS[k], c.baudot[1][k] = (uint8_t)RTTY_FIGS[k];
    c.H = rtty_hop(audio_rate);
}
// One entry of the batch's table: the client's window, bit length, candidates and lanes
struct RttyEntry {
    int slot, wn, u, usos;
    float ratio, lscale;  // lscale = 4 / (wn H)^2: level = max(em, es) lscale
    uint32_t cand;        // the pairs that may be followed
    int pad;
    uint32_t inc[RTTY_LANES];
    float rot[RTTY_LANES][2];
};
// the framing machine, in hops: busy - a character is being read, k hops since the hop that started it, i the next sample point
// (0 the start bit, 1..5 the data bits, 6 the stop bit), code the bits so far; sp - the line of the hop before was space;
// figs - the shift
struct RttyFrame {
    int busy, k, i, code, sp, figs;
};
// What a client carries from batch to batch.  All zero is the start; p is set to RTTY_P0 with the first batch (pos == 0 says so)
struct RttyState {
    float part[RTTY_HMAX];               // the unfinished hop's samples, part[0, pos % H)
    ToneC ring[RTTY_WMAX][RTTY_LANES];   // C of hop b in row b % 24
    float A[RTTY_PAIRS];                 // the followers
    uint64_t pos, nchars;
    float em, es, T, Nn;
    uint32_t errors;
    int p, present, pad;
    RttyFrame f;
};
// One frame's record
struct RttyRec {
    uint32_t nchars, errors;
    float offset_hz, level, quality;
    int present;
};
static_assert(sizeof(RttyEntry) == 416 && sizeof(RttyState) == 6536 && sizeof(RttyRec) == 24 && sizeof(RttyFrame) == 24 &&
                  sizeof(RttyTables) == sizeof(ToneTables) + 72,
              "the device tables' layout");

// ---- the hop ------------------------------------------------------------------------------------------------------------------
// C[b][k] over the hop's H samples: toneplan.h's seed and step, the phase of stream position b H
PSDR_HOST_DEVICE inline ToneC rtty_corr(const ToneTables *t, uint32_t inc, ToneC rot, uint64_t b, const float *x, int H) {
    ToneC w = tone_seed(t, tone_phase(inc, b * (uint64_t)H));
    ToneC acc = {0.f, 0.f};
    for (int n = 0; n < H; n++) tone_step(acc, w, rot, x[n]);
    return acc;
}
// one term of the bit window's sum
PSDR_HOST_DEVICE inline void rtty_window_step(ToneC &S, ToneC c) { S.re = S.re + c.re, S.im = S.im + c.im; }
// E = |S|^2; an energy that is not finite enters as 0
PSDR_HOST_DEVICE inline float rtty_energy(ToneC S) {
    const float E = tone_power(S);
    return tone_finite(E) ? E : 0.f;
}
// A_j follows E_2j + E_2j+1 with weight 1/64
PSDR_HOST_DEVICE inline float rtty_follow(float A, float Em, float Es) { return cw_follow(A, Em + Es); }
// em <- max(m, em - em / 256)
PSDR_HOST_DEVICE inline float rtty_peak(float em, float m) {
    const float d = fmaf(em, -0.00390625f, em);
    return m > d ? m : d;
}
// ... and a peak stays at 1/16 of the other at least: a tone that was not sent for seconds is sliced 12 dB under the other
PSDR_HOST_DEVICE inline float rtty_held(float mine, float other) {
    const float f = other * 0.0625f;
    return mine > f ? mine : f;
}
// T and Nn follow with weight 1/256
PSDR_HOST_DEVICE inline float rtty_slow(float T, float t) { return fmaf(t - T, 0.00390625f, T); }
// the bit, behind the peaks' update: mark iff m es >= s em - each tone sliced at its own half
PSDR_HOST_DEVICE inline int rtty_mark(float m, float s, float em, float es) { return m * es >= s * em ? 1 : 0; }
PSDR_HOST_DEVICE inline bool rtty_present(bool full, float T, float Nn, float ratio) { return full && tone_finite(T) && T > 0.f && T >= ratio * Nn; }
PSDR_HOST_DEVICE inline float rtty_quality(float T, float Nn) {
    if (Nn == 0.f) return 0.f;
    const float q = T / Nn;
    return tone_finite(q) ? q : 0.f;
}
// One hop of the framing: mark is the line (1 mark, 0 space).  Returns the character the hop appends, 0 for none; a stop bit
// that reads space counts one framing error
PSDR_HOST_DEVICE inline uint32_t rtty_frame_step(RttyFrame &f, int mark, int u, int usos, const uint8_t (*baudot)[32], uint32_t &errors) {
    uint32_t out = 0;
    if (!f.busy && !mark && !f.sp) f.busy = 1, f.k = 0, f.i = 0, f.code = 0;  // space directly behind mark: t0 = 16 (this hop)
    if (f.busy) {
        const int c = u / 2 + f.i * u;  // the sample point behind t0, in 1/16 hop
        if (c < 16 * (f.k + 1)) {       // (16 k <= c holds: the points are more than a hop apart)
            if (f.i == 0) {
                if (mark) f.busy = 0;  // a false start
                else f.i = 1;
            } else if (f.i <= 5) {
                f.code |= mark << (f.i - 1);
                f.i++;
            } else {
                if (mark) {
                    if (f.code == RTTY_CODE_LTRS) f.figs = 0;
                    else if (f.code == RTTY_CODE_FIGS) f.figs = 1;
                    else out = baudot[f.figs][f.code];
                    if (f.code == RTTY_CODE_SPACE && usos) f.figs = 0;
                } else {
                    errors++;
                }
                f.busy = 0;
            }
        }
        f.k++;
    }
    f.sp = !mark;
    return out;
}
// the record behind D complete hops
PSDR_HOST_DEVICE inline RttyRec rtty_record(uint64_t D, uint64_t nchars, uint32_t errors, int p, float em, float es, float T, float Nn, int present, float lscale) {
    if (D == 0) return RttyRec{0u, 0u, 0.f, 0.f, 0.f, 0};
    return RttyRec{(uint32_t)nchars, errors, (float)(20 * (p - RTTY_P0)), (em > es ? em : es) * lscale, rtty_quality(T, Nn), present};
}
// hop b's order-dependent part behind the pairs' arg-max: q is the lowest candidate with the largest A, Aq and Ap the followers of
// q and of the followed pair; E the hop's 32 energies are read at the new p.  One definition for the host and the kernel's wave
struct RttyScalars {
    uint64_t nchars;
    float em, es, T, Nn;
    uint32_t errors;
    int p, present;
    RttyFrame f;
};
PSDR_HOST_DEVICE inline int rtty_pair(int p, int q, float Aq, float Ap) { return cw_moves(Aq, Ap) ? q : p; }
PSDR_HOST_DEVICE inline uint32_t rtty_scalar_step(RttyScalars &z, const RttyEntry &e, uint64_t b, float m, float s, const uint8_t (*baudot)[32]) {
    const float pm = rtty_peak(z.em, m), ps = rtty_peak(z.es, s);
    z.em = rtty_held(pm, ps), z.es = rtty_held(ps, pm);
    const int bit = rtty_mark(m, s, z.em, z.es);
    const float t = m > s ? m : s, n = m > s ? s : m;
    z.T = rtty_slow(z.T, t), z.Nn = rtty_slow(z.Nn, n);
    z.present = rtty_present(b + 1 >= (uint64_t)RTTY_FILL, z.T, z.Nn, e.ratio) ? 1 : 0;
    return rtty_frame_step(z.f, z.present ? bit : 1, e.u, e.usos, baudot, z.errors);
}

// ---- the stream ---------------------------------------------------------------------------------------------------------------
// S[b][k] from the kept correlations: hops b - wn + 1 .. b, ascending; hops before the start count as 0.  row(hb): C of hop hb
template <class Row>
PSDR_HOST_DEVICE inline ToneC rtty_window(uint64_t b, int wn, Row row) {
    ToneC S = {0.f, 0.f};
    for (int j = 0; j < wn; j++) {
        const int64_t hb = (int64_t)b - wn + 1 + j;
        if (hb >= 0) rtty_window_step(S, row((uint64_t)hb));
    }
    return S;
}
// A client's batch on the host, as k_audio_rtty runs it: rows[nframes * h] and flags[nframes] are read, st and text carried,
// rec[nframes] written
inline void rtty_stream(const RttyTables &t, const RttyEntry &e, const float *rows, const int *flags, int h, int nframes, RttyState &st, uint8_t *text, RttyRec *rec) {
    const int H = t.H;
    const uint64_t pos0 = st.pos, L = (uint64_t)nframes * (uint64_t)h, b0 = pos0 / H, b1 = (pos0 + L) / H;
    RttyScalars z = {st.nchars, st.em, st.es, st.T, st.Nn, st.errors, pos0 == 0 ? RTTY_P0 : st.p, st.present, st.f};
    auto emit = [&](uint64_t D) {  // the frames at whose end D hops are complete
        const int lo = cw_first_frame(D, pos0, h, H), hi = std::min(nframes, cw_first_frame(D + 1, pos0, h, H));
        for (int f = lo; f < hi; f++) rec[f] = rtty_record(D, z.nchars, z.errors, z.p, z.em, z.es, z.T, z.Nn, z.present, e.lscale);
    };
    emit(b0);
    float x[RTTY_HMAX];
    for (uint64_t b = b0; b < b1; b++) {
        for (int n = 0; n < H; n++) x[n] = cw_sample(b * H + n, pos0, b0, H, st.part, rows, flags, h);
        for (int k = 0; k < RTTY_LANES; k++) st.ring[b % RTTY_WMAX][k] = rtty_corr(&t.t, e.inc[k], ToneC{e.rot[k][0], e.rot[k][1]}, b, x, H);
        float E[RTTY_LANES];
        for (int k = 0; k < RTTY_LANES; k++) E[k] = rtty_energy(rtty_window(b, e.wn, [&](uint64_t hb) { return st.ring[hb % RTTY_WMAX][k]; }));
        int q = -1;  // the lowest candidate with the largest A
        for (int j = 0; j < RTTY_PAIRS; j++) {
            st.A[j] = rtty_follow(st.A[j], E[2 * j], E[2 * j + 1]);
            if ((e.cand >> j & 1) && (q < 0 || tone_bits(st.A[j]) > tone_bits(st.A[q]))) q = j;
        }
        z.p = rtty_pair(z.p, q, st.A[q], st.A[z.p]);
        const uint32_t out = rtty_scalar_step(z, e, b, E[2 * z.p], E[2 * z.p + 1], t.baudot);
        if (out) text[z.nchars++ % RTTY_TEXT] = (uint8_t)out;
        emit(b + 1);
    }
    float part[RTTY_HMAX] = {};
    for (uint64_t u = b1 * H; u < pos0 + L; u++) part[u - b1 * H] = cw_sample(u, pos0, b0, H, st.part, rows, flags, h);
    memcpy(st.part, part, sizeof(part));
    st.pos = pos0 + L, st.nchars = z.nchars, st.em = z.em, st.es = z.es, st.T = z.T, st.Nn = z.Nn;
    st.errors = z.errors, st.p = z.p, st.present = z.present, st.f = z.f;
}

// ---- the call -----------------------------------------------------------------------------------------------------------------
// psdr_client_set_rtty_decoder's refusals, in the order they are looked for; cfg == null switches it off (an IQ client may)
enum RttyVerdict { RTTY_OK, RTTY_BAD_ID, RTTY_INACTIVE, RTTY_IQ, RTTY_BAD_MARK, RTTY_BAD_SHIFT, RTTY_BAD_BAUD, RTTY_BAD_USOS, RTTY_BAD_SEARCH, RTTY_BAD_SNR, RTTY_BAD_RATE, RTTY_BAD_BAND };
inline RttyVerdict rtty_check(const AudioSlot *slots, size_t S, int id, const psdr_rtty_config *cfg, int audio_rate) {
    if (id < 0 || (size_t)id >= S) return RTTY_BAD_ID;
    if (!slots[id].active) return RTTY_INACTIVE;
    if (!cfg) return RTTY_OK;
    if (slots[id].mode == PSDR_IQ) return RTTY_IQ;
    if (!cw_inside(cfg->mark_hz, RTTY_MARK_MIN, RTTY_MARK_MAX)) return RTTY_BAD_MARK;
    if (!cw_inside(std::fabs(cfg->shift_hz), RTTY_SHIFT_MIN, RTTY_SHIFT_MAX)) return RTTY_BAD_SHIFT;
    if (!cw_inside(cfg->baud, RTTY_BAUD_MIN, RTTY_BAUD_MAX)) return RTTY_BAD_BAUD;
    if (cfg->usos != 0 && cfg->usos != 1) return RTTY_BAD_USOS;
    if (!cw_inside(cfg->search_hz, RTTY_SEARCH_MIN, RTTY_SEARCH_MAX)) return RTTY_BAD_SEARCH;
    if (!cw_inside(cfg->snr_db, RTTY_SNR_MIN, RTTY_SNR_MAX)) return RTTY_BAD_SNR;
    if (audio_rate < RTTY_RATE_MIN || audio_rate > RTTY_RATE_MAX) return RTTY_BAD_RATE;
    const double space = cfg->mark_hz + cfg->shift_hz, hi = std::max(cfg->mark_hz, space), lo = std::min(cfg->mark_hz, space);
    if (hi + RTTY_EDGE > RTTY_TOP * audio_rate || lo - RTTY_EDGE < RTTY_BOTTOM) return RTTY_BAD_BAND;
    return RTTY_OK;
}
// ... and what an accepted call does to the slot: switching it ON - from off, or again - starts the state from zero at the
// client's next listed batch (also while paused)
inline void rtty_apply(AudioSlot &s, const psdr_rtty_config *cfg, int audio_rate) {
    s.rtty_on = cfg ? 1 : 0;
    if (!cfg) return;
    const double rate = (double)audio_rate;
    s.rtty_wn = rtty_wn_of(cfg->baud, rate), s.rtty_u = rtty_u_of(cfg->baud, rate), s.rtty_usos = cfg->usos;
    s.rtty_cand = rtty_candidates(cfg->search_hz);
    s.rtty_ratio = tone_ratio(cfg->snr_db);
    const double span = (double)s.rtty_wn * rtty_hop(rate);
    s.rtty_lscale = (float)(4.0 / (span * span));
    for (int j = 0; j < RTTY_PAIRS; j++) {
        tone_inc_rot(cfg->mark_hz + rtty_pair_hz(j), rate, s.rtty_inc[2 * j], s.rtty_rot[2 * j]);
        tone_inc_rot(cfg->mark_hz + cfg->shift_hz + rtty_pair_hz(j), rate, s.rtty_inc[2 * j + 1], s.rtty_rot[2 * j + 1]);
    }
    s.rtty_fresh = true;
}
// psdr_rtty_defaults: 2125 Hz where the pairs of 2125 and 2295 Hz stay under 0.45 audio_rate, else 915 Hz
inline bool rtty_defaults(double audio_rate, psdr_rtty_config *out) {
    if (!out || !(audio_rate >= RTTY_RATE_MIN && audio_rate <= RTTY_RATE_MAX)) return false;
    const bool room = RTTY_MARK_DEFAULT + RTTY_SHIFT_DEFAULT + RTTY_EDGE < RTTY_TOP * audio_rate;
    out->mark_hz = room ? RTTY_MARK_DEFAULT : RTTY_MARK_LOW, out->shift_hz = RTTY_SHIFT_DEFAULT, out->baud = RTTY_BAUD_DEFAULT;
    out->usos = 1, out->search_hz = RTTY_SEARCH_DEFAULT, out->snr_db = RTTY_SNR_DEFAULT;
    return true;
}
inline void rtty_entry(RttyEntry &e, int slot, const AudioSlot &s) {
    e.slot = slot, e.wn = s.rtty_wn, e.u = s.rtty_u, e.usos = s.rtty_usos;
    e.ratio = s.rtty_ratio, e.lscale = s.rtty_lscale, e.cand = s.rtty_cand, e.pad = 0;
    memcpy(e.inc, s.rtty_inc, sizeof(e.inc));
    memcpy(e.rot, s.rtty_rot, sizeof(e.rot));
}

// ---- the batch ----------------------------------------------------------------------------------------------------------------
struct RttyPlan {
    int n = 0;                 // table[0, n): the batch's RTTY clients, in slot order
    std::vector<size_t> zero;  // slots whose state and text start this batch from zero
    bool any() const { return n > 0; }  // no such client in the batch: nothing is uploaded, zeroed or launched
};
// One batch, behind demod_plan(): cw_plan with other fields.  Of the clients the batch demodulated the ones with the decoder on
// whose kind wrote audio rows are listed; the state starts from zero when the call switched it on since the client's last listed
// batch, on a mode change and on a retune.  An IQ client and a paused one keep setting, state and a pending fresh start.
// b_rtty_on: the last batch ran with the decoder for this client (psdr_read_rtty)
inline RttyPlan rtty_plan(AudioSlot *slots, size_t S, uint64_t demod_seq, RttyEntry *table) {
    RttyPlan p;
    for (size_t i = 0; i < S; i++) {
        AudioSlot &s = slots[i];
        if (!s.active || s.paused || s.last_seq != demod_seq) continue;
        s.b_rtty_on = false;
        if (s.b_mode == PSDR_IQ || !s.rtty_on) continue;
        s.b_rtty_on = true;
        const int m = (int)std::floor(s.b_mid);
        if (s.rtty_fresh || s.rtty_mode != s.b_mode || s.rtty_l != s.b_l || s.rtty_r != s.b_r || s.rtty_m != m) p.zero.push_back(i);
        s.rtty_fresh = false;
        s.rtty_mode = s.b_mode, s.rtty_l = s.b_l, s.rtty_r = s.b_r, s.rtty_m = m;
        rtty_entry(table[p.n++], (int)i, s);
    }
    return p;
}

}  // namespace psdr

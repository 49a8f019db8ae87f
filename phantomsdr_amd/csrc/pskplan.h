// pskplan.h - the per-client PSK31 decoder (include/psdr.h: psdr_client_set_psk_decoder), everything of it that is not a launch:
// the ONE definition of the hop correlation, the symbol window, the symbol clock, the differential detection, the carrier follower,
// the presence, the varicode machine and its table, the records and the stream's bookkeeping (k_audio_psk in psk.h and the host
// tests run this text), the tables, the argument validation, the defaults and psk_plan(), which walks the audio slots behind
// demod_plan() and says who is listed in the batch and whose state starts from zero.  Plain C++17 (no HIP):
// tests/test_psk_host.py builds it with the host compiler.
//
// The rule is written out in include/psdr.h.  Phases, seeds and the per-sample rotation are toneplan.h's functions; the lanes are
// the client's own (they follow carrier_hz and baud), so increments and rotations travel in the batch's table, as rttyplan.h's do,
// and the context's tables hold the two seed tables and the varicode table by code.  The hop and its correlation are rttyplan.h's,
// the frames of a hop, the sample of a stream and the move of a follower cwplan.h's.  Every f32 operation is an explicit fmaf, a
// lone multiply, a lone add or the one division of `quality`, so contraction has nothing to fuse; clock and varicode are integer
// arithmetic.
#pragma once
#include "rttyplan.h"

namespace psdr {

constexpr int PSK_LANES = PSDR_PSK_LANES;  // 16 lanes baud / 8 apart
constexpr int PSK_P0 = 8;                  // the lane on the configured carrier, where the follower starts
constexpr int PSK_GROUP = 16;              // hops the kernel correlates at once, four per wave
constexpr int PSK_HMAX = RTTY_HMAX;        // the longest hop
constexpr int PSK_WMAX = 32;               // hops of correlations the state keeps: the symbol window is 8 to 32 of them
constexpr int PSK_BINS = 16;               // timing bins of the symbol clock
constexpr int PSK_FILL = 32;               // sample points before the presence is read: one time constant of the coherence
constexpr int PSK_TEXT = 1024;             // characters the device keeps per slot
constexpr int PSK_SR_BITS = 12;            // a shift register longer than this without 00 holds no character
constexpr int PSK_RATE_MIN = RTTY_RATE_MIN, PSK_RATE_MAX = RTTY_RATE_MAX;
constexpr double PSK_CARRIER_MIN = 300.0, PSK_CARRIER_MAX = 3000.0, PSK_CARRIER_DEFAULT = 1000.0;
constexpr double PSK_BAUD_31 = 31.25, PSK_BAUD_63 = 62.5;
constexpr double PSK_SEARCH_LANES = 3.0;   // the default search: three lanes to either side
constexpr double PSK_QUALITY_DEFAULT = PSDR_PSK_QUALITY_DEFAULT;
constexpr double PSK_TOP = 0.45, PSK_BOTTOM = 100.0;  // every lane stays under 0.45 audio_rate and above 100 Hz

inline double psk_lane_hz(int j, double baud) { return (j - PSK_P0) * baud / 8.0; }
// the symbol window in hops, and the symbol length in 1/16 hop: both rounded to nearest, in double
inline int psk_wn_of(double baud, double audio_rate) { return (int)std::floor(audio_rate / (baud * rtty_hop(audio_rate)) + 0.5); }
inline int psk_u_of(double baud, double audio_rate) { return (int)std::floor(16.0 * audio_rate / (baud * rtty_hop(audio_rate)) + 0.5); }
inline uint32_t psk_candidates(double search_hz, double baud) {
    uint32_t m = 1u << PSK_P0;
    for (int j = 0; j < PSK_LANES; j++)
        if (std::fabs(psk_lane_hz(j, baud)) <= search_hz) m |= 1u << j;
    return m;
}

// G3PLX's varicode by character: the code's bits, the first one sent on top.  No code holds 00, each begins and ends in 1, every
// such string of up to 9 bits is used and 40 of the 55 of 10 bits (tests/test_psk_host.py holds the table to that and to the anchors)
static const uint16_t PSK_VARICODE[128] = {
    0x2ab, 0x2db, 0x2ed, 0x377, 0x2eb, 0x35f, 0x2ef, 0x2fd, 0x2ff, 0x0ef, 0x01d, 0x36f, 0x2dd, 0x01f, 0x375, 0x3ab,  // NUL .. SI
    0x2f7, 0x2f5, 0x3ad, 0x3af, 0x35b, 0x36b, 0x36d, 0x357, 0x37b, 0x37d, 0x3b7, 0x355, 0x35d, 0x3bb, 0x2fb, 0x37f,  // DLE .. US
    0x001, 0x1ff, 0x15f, 0x1f5, 0x1db, 0x2d5, 0x2bb, 0x17f, 0x0fb, 0x0f7, 0x16f, 0x1df, 0x075, 0x035, 0x057, 0x1af,  // space .. /
    0x0b7, 0x0bd, 0x0ed, 0x0ff, 0x177, 0x15b, 0x16b, 0x1ad, 0x1ab, 0x1b7, 0x0f5, 0x1bd, 0x1ed, 0x055, 0x1d7, 0x2af,  // 0 .. ?
    0x2bd, 0x07d, 0x0eb, 0x0ad, 0x0b5, 0x077, 0x0db, 0x0fd, 0x155, 0x07f, 0x1fd, 0x17d, 0x0d7, 0x0bb, 0x0dd, 0x0ab,  // @ .. O
    0x0d5, 0x1dd, 0x0af, 0x06f, 0x06d, 0x157, 0x1b5, 0x15d, 0x175, 0x17b, 0x2ad, 0x1f7, 0x1ef, 0x1fb, 0x2bf, 0x16d,  // P .. _
    0x2df, 0x00b, 0x05f, 0x02f, 0x02d, 0x003, 0x03d, 0x05b, 0x02b, 0x00d, 0x1eb, 0x0bf, 0x01b, 0x03b, 0x00f, 0x007,  // ` .. o
    0x03f, 0x1bf, 0x015, 0x017, 0x005, 0x037, 0x07b, 0x06b, 0x0df, 0x05d, 0x1d5, 0x2b7, 0x1bb, 0x2b5, 0x2d7, 0x3b5,  // p .. DEL
};

// The tables of the context: the seed tables (of t, inc, rot, h, nb and lscale are not used) and the varicode by code: the
// character + 1, 0 for a code that is none
struct PskTables {
    ToneTables t;
    uint8_t vari[1024];
    int H, pad;
};
inline void psk_tables(PskTables &c, double audio_rate) {
    memset(&c, 0, sizeof(c));
    tone_seed_tables(c.t);
    for (int ch = 0; ch < 128; ch++) c.vari[PSK_VARICODE[ch]] = (uint8_t)(ch + 1);
    c.H = rtty_hop(audio_rate);
}
// One entry of the batch's table: the client's window, symbol length, candidates and lanes
struct PskEntry {
    int slot, wn, u;
    uint32_t cand;            // the lanes that may be followed
    float quality, lscale;    // lscale = 4 / (wn H)^2: level = the follower of E_p at the sample points, times lscale
    float df;                 // baud / 8, exact in f32: offset_hz = (p - 8) df
    int pad;
    uint32_t inc[PSK_LANES];
    float rot[PSK_LANES][2];
};
// What a client carries from batch to batch.  All zero is the start; p is set to PSK_P0 with the first batch (pos == 0 says so)
struct PskState {
    float part[PSK_HMAX];               // the unfinished hop's samples, part[0, pos % H)
    ToneC ring[PSK_WMAX][PSK_LANES];    // C of hop b in row b % 32
    ToneC prev[PSK_LANES];              // S at the last sample point
    float Qre[PSK_LANES];               // the followers of Re d^2
    float G[PSK_BINS];                  // the timing bins' followers
    uint64_t pos, nchars;
    float quality, level;
    uint32_t errors, sr;
    int p, present, c, age, nsp, pad;
};
// One frame's record
struct PskRec {
    uint32_t nchars, errors;
    float offset_hz, level, quality;
    int present;
};
static_assert(sizeof(PskEntry) == 224 && sizeof(PskState) == 4664 && sizeof(PskRec) == 24 && sizeof(PskTables) == sizeof(ToneTables) + 1032,
              "the device tables' layout");

// ---- the hop ------------------------------------------------------------------------------------------------------------------
// C[b][j] is rtty_corr, a term of the window's sum rtty_window_step, E = |S|^2 rtty_energy.
// the followers of the clock and of the detection have weight 1/32
PSDR_HOST_DEVICE inline float psk_follow(float A, float v) { return fmaf(v - A, 0.03125f, A); }
PSDR_HOST_DEVICE inline float psk_clean(float v) { return tone_finite(v) ? v : 0.f; }
// what the wave and the host carry besides the per-lane followers
struct PskScalars {
    uint64_t nchars;
    float quality, level;
    uint32_t errors, sr;
    int p, present, c, age, nsp;
};
// what the clock follows: the sum of the candidates' energies, j ascending.  (The followed lane's alone would do for a signal that
// is followed - but idle reversals are two steady tones baud / 2 to either side, a lane near one of them sees a steady carrier
// whose E has no dips, the bins level out, the sample points drift off the symbols and the true lane reads nothing: the follower
// would hold the false lane until text comes.)  E(j): lane j's energy
template <class Energy>
PSDR_HOST_DEVICE inline float psk_clock_energy(uint32_t cand, Energy E) {
    float T = 0.f;
    for (int j = 0; j < PSK_LANES; j++)
        if (cand >> j & 1) T = T + E(j);
    return T;
}
// The clock, part 1: the hop advances c by 16 modulo u (u >= 128); its timing bin
PSDR_HOST_DEVICE inline int psk_clock_bin(PskScalars &z, int u) {
    z.c += 16;
    if (z.c >= u) z.c -= u;
    return 16 * z.c / u;
}
// ... part 2, behind the bins' arg-max g: the hop is a sample point when the clock is within half a symbol behind
// tau = floor(g u / 16) and three quarters of a symbol have passed since the last one.  (Asking for the hop in which the clock
// crosses tau loses a symbol whenever a bin's update moves the arg-max to a bin the clock has just left; this way a move of up to
// eight bins back or four bins on costs none and doubles none.)
PSDR_HOST_DEVICE inline bool psk_clock_sample(PskScalars &z, const PskEntry &e, int g) {
    z.age = z.age + 16 > 65536 ? 65536 : z.age + 16;
    int d = z.c - g * e.u / 16;
    if (d < 0) d += e.u;
    if (d >= e.u / 2 || z.age < 3 * e.u / 4) return false;
    z.age = 0;
    return true;
}
// A lane at a sample point: d = S conj(prev), prev <- S, the follower of Re d^2; returns Re d, Re d^2 and |d|^2
struct PskD {
    float re, q, w;
};
PSDR_HOST_DEVICE inline PskD psk_lane_step(ToneC S, ToneC &prev, float &Qre) {
    const float dre = fmaf(S.re, prev.re, S.im * prev.im);
    const float dim = fmaf(S.im, prev.re, -(S.re * prev.im));
    prev = S;
    const float q = psk_clean(fmaf(dre, dre, -(dim * dim)));
    const float w = psk_clean(fmaf(dre, dre, dim * dim));
    Qre = psk_follow(Qre, q);
    return PskD{dre, q, w};
}
// M = max(Qre, +0): what the carrier follower compares (a value that is no number reads +0)
PSDR_HOST_DEVICE inline float psk_merit(float Qre) { return Qre > 0.f ? Qre : 0.f; }
// the follower moves to q only when M_q > 2 M_p; the bits of another lane are another line: the register starts over (a lane on
// one of the idle's two tones reads ones, the true lane zeros - behind a move in the idle they would end a character nobody sent)
PSDR_HOST_DEVICE inline void psk_move(PskScalars &z, int q, float Mq, float Mp) {
    if (!cw_moves(Mq, Mp) || q == z.p) return;
    z.p = q, z.sr = 0;
}
// the symbol's own coherence, cos of twice its turn: Re d^2 / |d|^2 as one f32 division, 0 when |d|^2 is 0 or the quotient is not
// finite
PSDR_HOST_DEVICE inline float psk_coherence(float q, float w) {
    if (w == 0.f) return 0.f;
    const float c = q / w;
    return tone_finite(c) ? c : 0.f;
}
PSDR_HOST_DEVICE inline bool psk_present(bool full, float coherence, float quality) { return full && coherence >= quality; }
// One bit of the varicode machine.  Returns the character + 1 the bit completes, 0 for none (NUL is dropped by the caller's + 1
// test); a code that is no character counts one error, as does a register that passes 12 bits without 00 - unless it holds
// ones only, which is the steady carrier behind a transmission and not a fault of the line
PSDR_HOST_DEVICE inline uint32_t psk_bit_step(uint32_t &sr, int bit, const uint8_t *vari, uint32_t &errors) {
    sr = sr << 1 | (uint32_t)bit;
    if ((sr & 3u) == 0u) {
        const uint32_t code = sr >> 2;
        sr = 0;
        if (code == 0) return 0;
        const uint32_t ch = code < 1024u ? vari[code] : 0u;  // (12 bits and a 0: a code of 11 bits is none)
        if (!ch) errors++;
        return ch;
    }
    if (sr >> PSK_SR_BITS) {
        if (sr != (2u << PSK_SR_BITS) - 1u) errors++;
        sr = 0;
    }
    return 0;
}
// A sample point behind the lanes' steps and the carrier's arg-max: Ep and d are the followed lane's (the new p's).  Returns
// the character the symbol appends, 0 for none.  One definition for the host and the kernel's wave
PSDR_HOST_DEVICE inline uint32_t psk_symbol_step(PskScalars &z, const PskEntry &e, float Ep, PskD d, const uint8_t *vari) {
    z.level = psk_follow(z.level, Ep);
    if (z.nsp < PSK_FILL) z.nsp++;
    z.quality = psk_follow(z.quality, psk_coherence(d.q, d.w));
    z.present = psk_present(z.nsp >= PSK_FILL, z.quality, e.quality) ? 1 : 0;
    if (!z.present) {  // an absent signal is a steady carrier: nothing is printed and the register is cleared
        z.sr = 0;
        return 0;
    }
    const uint32_t ch = psk_bit_step(z.sr, d.re >= 0.f ? 1 : 0, vari, z.errors);
    return ch > 1 ? ch - 1 : 0;
}
// the record behind D complete hops
PSDR_HOST_DEVICE inline PskRec psk_record(uint64_t D, const PskScalars &z, float df, float lscale) {
    if (D == 0) return PskRec{0u, 0u, 0.f, 0.f, 0.f, 0};
    return PskRec{(uint32_t)z.nchars, z.errors, (float)(z.p - PSK_P0) * df, z.level * lscale, z.quality, z.present};
}
PSDR_HOST_DEVICE inline PskScalars psk_scalars(const PskState &st) {
    return PskScalars{st.nchars, st.quality, st.level, st.errors, st.sr, st.pos == 0 ? PSK_P0 : st.p, st.present, st.c, st.age, st.nsp};
}
PSDR_HOST_DEVICE inline void psk_keep(PskState &st, const PskScalars &z, uint64_t pos) {
    st.pos = pos, st.nchars = z.nchars, st.quality = z.quality, st.level = z.level, st.errors = z.errors, st.sr = z.sr;
    st.p = z.p, st.present = z.present, st.c = z.c, st.age = z.age, st.nsp = z.nsp;
}

// ---- the stream ---------------------------------------------------------------------------------------------------------------
// A client's batch on the host, as k_audio_psk runs it: rows[nframes * h] and flags[nframes] are read, st and text carried,
// rec[nframes] written
inline void psk_stream(const PskTables &t, const PskEntry &e, const float *rows, const int *flags, int h, int nframes, PskState &st, uint8_t *text, PskRec *rec) {
    const int H = t.H;
    const uint64_t pos0 = st.pos, L = (uint64_t)nframes * (uint64_t)h, b0 = pos0 / H, b1 = (pos0 + L) / H;
    PskScalars z = psk_scalars(st);
    auto emit = [&](uint64_t D) {  // the frames at whose end D hops are complete
        const int lo = cw_first_frame(D, pos0, h, H), hi = std::min(nframes, cw_first_frame(D + 1, pos0, h, H));
        for (int f = lo; f < hi; f++) rec[f] = psk_record(D, z, e.df, e.lscale);
    };
    emit(b0);
    float x[PSK_HMAX];
    for (uint64_t b = b0; b < b1; b++) {
        for (int n = 0; n < H; n++) x[n] = cw_sample(b * H + n, pos0, b0, H, st.part, rows, flags, h);
        for (int j = 0; j < PSK_LANES; j++) st.ring[b % PSK_WMAX][j] = rtty_corr(&t.t, e.inc[j], ToneC{e.rot[j][0], e.rot[j][1]}, b, x, H);
        ToneC S[PSK_LANES];
        for (int j = 0; j < PSK_LANES; j++) S[j] = rtty_window(b, e.wn, [&](uint64_t hb) { return st.ring[hb % PSK_WMAX][j]; });
        const int bin = psk_clock_bin(z, e.u);
        st.G[bin] = psk_follow(st.G[bin], psk_clock_energy(e.cand, [&](int j) { return rtty_energy(S[j]); }));
        int g = 0;  // the lowest bin with the largest G
        for (int i = 1; i < PSK_BINS; i++)
            if (tone_bits(st.G[i]) > tone_bits(st.G[g])) g = i;
        if (psk_clock_sample(z, e, g)) {
            PskD d[PSK_LANES];
            int q = -1;  // the lowest candidate with the largest M
            for (int j = 0; j < PSK_LANES; j++) {
                d[j] = psk_lane_step(S[j], st.prev[j], st.Qre[j]);
                if ((e.cand >> j & 1) && (q < 0 || tone_bits(psk_merit(st.Qre[j])) > tone_bits(psk_merit(st.Qre[q])))) q = j;
            }
            psk_move(z, q, psk_merit(st.Qre[q]), psk_merit(st.Qre[z.p]));
            const uint32_t out = psk_symbol_step(z, e, rtty_energy(S[z.p]), d[z.p], t.vari);
            if (out) text[z.nchars++ % PSK_TEXT] = (uint8_t)out;
        }
        emit(b + 1);
    }
    float part[PSK_HMAX] = {};
    for (uint64_t u = b1 * H; u < pos0 + L; u++) part[u - b1 * H] = cw_sample(u, pos0, b0, H, st.part, rows, flags, h);
    memcpy(st.part, part, sizeof(part));
    psk_keep(st, z, pos0 + L);
}

// ---- the call -----------------------------------------------------------------------------------------------------------------
// psdr_client_set_psk_decoder's refusals, in the order they are looked for; cfg == null switches it off (an IQ client may)
enum PskVerdict { PSK_OK, PSK_BAD_ID, PSK_INACTIVE, PSK_IQ, PSK_BAD_CARRIER, PSK_BAD_BAUD, PSK_BAD_SEARCH, PSK_BAD_QUALITY, PSK_BAD_RATE, PSK_BAD_BAND };
inline PskVerdict psk_check(const AudioSlot *slots, size_t S, int id, const psdr_psk_config *cfg, int audio_rate) {
    if (id < 0 || (size_t)id >= S) return PSK_BAD_ID;
    if (!slots[id].active) return PSK_INACTIVE;
    if (!cfg) return PSK_OK;
    if (slots[id].mode == PSDR_IQ) return PSK_IQ;
    if (!cw_inside(cfg->carrier_hz, PSK_CARRIER_MIN, PSK_CARRIER_MAX)) return PSK_BAD_CARRIER;
    if (!(cfg->baud == PSK_BAUD_31 || cfg->baud == PSK_BAUD_63)) return PSK_BAD_BAUD;
    if (!(std::isfinite(cfg->search_hz) && cfg->search_hz >= 0 && cfg->search_hz < cfg->baud / 2)) return PSK_BAD_SEARCH;
    if (!(std::isfinite(cfg->quality) && cfg->quality > 0 && cfg->quality < 1)) return PSK_BAD_QUALITY;
    if (audio_rate < PSK_RATE_MIN || audio_rate > PSK_RATE_MAX) return PSK_BAD_RATE;
    if (cfg->carrier_hz + psk_lane_hz(PSK_LANES - 1, cfg->baud) > PSK_TOP * audio_rate || cfg->carrier_hz + psk_lane_hz(0, cfg->baud) < PSK_BOTTOM) return PSK_BAD_BAND;
    return PSK_OK;
}
// ... and what an accepted call does to the slot: switching it ON - from off, or again - starts the state from zero at the
// client's next listed batch (also while paused)
inline void psk_apply(AudioSlot &s, const psdr_psk_config *cfg, int audio_rate) {
    s.psk_on = cfg ? 1 : 0;
    if (!cfg) return;
    const double rate = (double)audio_rate;
    s.psk_wn = psk_wn_of(cfg->baud, rate), s.psk_u = psk_u_of(cfg->baud, rate);
    s.psk_cand = psk_candidates(cfg->search_hz, cfg->baud);
    s.psk_quality = (float)cfg->quality, s.psk_df = (float)(cfg->baud / 8.0);
    const double span = (double)s.psk_wn * rtty_hop(rate);
    s.psk_lscale = (float)(4.0 / (span * span));
    for (int j = 0; j < PSK_LANES; j++) tone_inc_rot(cfg->carrier_hz + psk_lane_hz(j, cfg->baud), rate, s.psk_inc[j], s.psk_rot[j]);
    s.psk_fresh = true;
}
// psdr_psk_defaults: 1000 Hz, PSK31, three lanes to either side
inline bool psk_defaults(double audio_rate, psdr_psk_config *out) {
    if (!out || !(audio_rate >= PSK_RATE_MIN && audio_rate <= PSK_RATE_MAX)) return false;
    out->carrier_hz = PSK_CARRIER_DEFAULT, out->baud = PSK_BAUD_31;
    out->search_hz = PSK_SEARCH_LANES * PSK_BAUD_31 / 8.0, out->quality = PSK_QUALITY_DEFAULT;
    return true;
}
inline void psk_entry(PskEntry &e, int slot, const AudioSlot &s) {
    e.slot = slot, e.wn = s.psk_wn, e.u = s.psk_u, e.cand = s.psk_cand;
    e.quality = s.psk_quality, e.lscale = s.psk_lscale, e.df = s.psk_df, e.pad = 0;
    memcpy(e.inc, s.psk_inc, sizeof(e.inc));
    memcpy(e.rot, s.psk_rot, sizeof(e.rot));
}

// ---- the batch ----------------------------------------------------------------------------------------------------------------
struct PskPlan {
    int n = 0;                 // table[0, n): the batch's PSK clients, in slot order
    std::vector<size_t> zero;  // slots whose state and text start this batch from zero
    bool any() const { return n > 0; }  // no such client in the batch: nothing is uploaded, zeroed or launched
};
// One batch, behind demod_plan(): rtty_plan with other fields.  Of the clients the batch demodulated the ones with the decoder on
// whose kind wrote audio rows are listed; the state starts from zero when the call switched it on since the client's last listed
// batch, on a mode change and on a retune.  An IQ client and a paused one keep setting, state and a pending fresh start.
// b_psk_on: the last batch ran with the decoder for this client (psdr_read_psk)
inline PskPlan psk_plan(AudioSlot *slots, size_t S, uint64_t demod_seq, PskEntry *table) {
    PskPlan p;
    for (size_t i = 0; i < S; i++) {
        AudioSlot &s = slots[i];
        if (!s.active || s.paused || s.last_seq != demod_seq) continue;
        s.b_psk_on = false;
        if (s.b_mode == PSDR_IQ || !s.psk_on) continue;
        s.b_psk_on = true;
        const int m = (int)std::floor(s.b_mid);
        if (s.psk_fresh || s.psk_mode != s.b_mode || s.psk_l != s.b_l || s.psk_r != s.b_r || s.psk_m != m) p.zero.push_back(i);
        s.psk_fresh = false;
        s.psk_mode = s.b_mode, s.psk_l = s.b_l, s.psk_r = s.b_r, s.psk_m = m;
        psk_entry(table[p.n++], (int)i, s);
    }
    return p;
}

}  // namespace psdr

// cwplan.h - the per-client CW decoder (include/psdr.h: psdr_client_set_cw_decoder), everything of it that is not a launch: the
// ONE definition of the hop correlation, the lane energies, the pitch follower, the levels, the keying and timing state machine,
// the Morse table, the records and the stream's bookkeeping (k_audio_cw in cw.h and the host tests run this text), the tables, the
// argument validation, the defaults and cw_plan(), which walks the audio slots behind demod_plan() and says who is listed in the
// batch and whose state starts from zero.  Plain C++17 (no HIP): tests/test_cw_host.py builds it with the host compiler.
//
// The rule is written out in include/psdr.h.  Phases, seeds and the per-sample rotation are toneplan.h's functions on a ToneTables
// whose lanes hold the CW pitches; only the block length differs (a hop of H samples, not 256).  Every f32 operation is an explicit
// fmaf, a lone multiply or a lone add, so contraction has nothing to fuse; everything behind the levels is integer arithmetic.
#pragma once
#include "toneplan.h"

namespace psdr {

constexpr int CW_LANES = PSDR_CW_LANES;  // candidate pitches, lane = pitch
constexpr int CW_GROUP = 4;              // hops the kernel correlates at once, one per wave
constexpr int CW_HMAX = 256;             // the longest hop
constexpr int CW_RING = 128;             // the last values of e the floor is ranked over
constexpr int CW_LO_RANK = 16;           // lo: the 16th smallest (0-based) of them, the 12.5 % quantile
constexpr int CW_TEXT = 1024;            // characters the device keeps per slot
constexpr int CW_UTAB = 512;             // entries of the wpm table: u < 512 at every rate
constexpr int CW_TOO_LONG = 256;         // the code of more than 7 elements
constexpr int CW_RATE_MIN = 4000, CW_RATE_MAX = 48000;
constexpr double CW_F0 = 250.0, CW_DF = 25.0;  // lane k listens at 250 + 25 k Hz
constexpr double CW_PITCH_MIN = 300.0, CW_PITCH_MAX = 1800.0, CW_PITCH_DEFAULT = 700.0;
constexpr double CW_SEARCH_MIN = 0.0, CW_SEARCH_MAX = 800.0, CW_SEARCH_DEFAULT = 100.0;
constexpr double CW_WPM_MIN = 10.0, CW_WPM_MAX = 40.0, CW_WPM_DEFAULT = 20.0;
constexpr double CW_SNR_MIN = 6.0, CW_SNR_MAX = 40.0, CW_SNR_DEFAULT = 22.0;

// a hop lasts 4 to 8 ms
inline int cw_hop(double audio_rate) { return audio_rate < 8000 ? 32 : audio_rate < 16000 ? 64 : audio_rate < 32000 ? 128 : 256; }
inline double cw_lane_hz(int k) { return CW_F0 + CW_DF * k; }
// the dot length in 1/16 hop at `wpm`: 1.2 / wpm seconds, rounded to nearest
inline int cw_u_of(double wpm, double audio_rate) { return (int)std::floor(19.2 * audio_rate / (cw_hop(audio_rate) * wpm) + 0.5); }
// the lane nearest to pitch_hz (a tie goes up)
inline int cw_nearest(double pitch_hz) {
    const int k = (int)std::floor((pitch_hz - CW_F0) / CW_DF + 0.5);
    return k < 0 ? 0 : k >= CW_LANES ? CW_LANES - 1 : k;
}
inline uint64_t cw_candidates(double pitch_hz, double search_hz) {
    uint64_t m = 1ull << cw_nearest(pitch_hz);
    for (int k = 0; k < CW_LANES; k++)
        if (std::fabs(cw_lane_hz(k) - pitch_hz) <= search_hz) m |= 1ull << k;
    return m;
}

// ITU-R M.1677-1: letters, figures and the punctuation . , : ? ' - / ( ) " = + @
struct CwSign {
    char ch;
    const char *key;
};
static const CwSign CW_SIGNS[] = {
    {'A', ".-"},     {'B', "-..."},   {'C', "-.-."},   {'D', "-.."},    {'E', "."},      {'F', "..-."},   {'G', "--."},    {'H', "...."},
    {'I', ".."},     {'J', ".---"},   {'K', "-.-"},    {'L', ".-.."},   {'M', "--"},     {'N', "-."},     {'O', "---"},    {'P', ".--."},
    {'Q', "--.-"},   {'R', ".-."},    {'S', "..."},    {'T', "-"},      {'U', "..-"},    {'V', "...-"},   {'W', ".--"},    {'X', "-..-"},
    {'Y', "-.--"},   {'Z', "--.."},   {'1', ".----"},  {'2', "..---"},  {'3', "...--"},  {'4', "....-"},  {'5', "....."},  {'6', "-...."},
    {'7', "--..."},  {'8', "---.."},  {'9', "----."},  {'0', "-----"},  {'.', ".-.-.-"}, {',', "--..--"}, {':', "---..."}, {'?', "..--.."},
    {'\'', ".----."}, {'-', "-....-"}, {'/', "-..-."},  {'(', "-.--."},  {')', "-.--.-"}, {'"', ".-..-."}, {'=', "-...-"},  {'+', ".-.-."},
    {'@', ".--.-."}};
constexpr int CW_NSIGNS = (int)(sizeof(CW_SIGNS) / sizeof(CW_SIGNS[0]));
// the code of a keying: it starts at 1 and is shifted left per element, the low bit 1 for a dah
inline int cw_code_of(const char *key) {
    int code = 1;
    for (; *key; key++) code = (code << 1) | (*key == '-' ? 1 : 0);
    return code;
}

// The tables of the plan, computed in double and rounded once.  t: the seed tables, and inc / rot of the 64 lanes (h, nb and lscale
// of it are not used); wpm[u] = 1.2 audio_rate / (H u / 16); hz: the lanes; morse: character by code, '*' where there is none;
// lscale = 1 / H^2: level = hi lscale, the squared amplitude of a steady tone
struct CwTables {
    ToneTables t;
    float wpm[CW_UTAB];
    float hz[CW_LANES];
    uint8_t morse[256];
    int H, umin, umax;  // the dot length's bounds: 40 and 10 WPM
    float lscale;
};
inline void cw_tables(CwTables &c, double audio_rate) {
    memset(&c, 0, sizeof(c));
    tone_seed_tables(c.t);
    for (int k = 0; k < CW_LANES; k++) {
        tone_lane(c.t, k, cw_lane_hz(k), audio_rate);
        c.hz[k] = (float)cw_lane_hz(k);
    }
    c.H = cw_hop(audio_rate);
    for (int u = 1; u < CW_UTAB; u++) c.wpm[u] = (float)(19.2 * audio_rate / ((double)c.H * u));
    memset(c.morse, '*', sizeof(c.morse));
    for (int j = 0; j < CW_NSIGNS; j++) c.morse[cw_code_of(CW_SIGNS[j].key)] = (uint8_t)CW_SIGNS[j].ch;
    c.umin = cw_u_of(CW_WPM_MAX, audio_rate), c.umax = cw_u_of(CW_WPM_MIN, audio_rate);
    c.lscale = (float)(1.0 / ((double)c.H * c.H));
}
// One entry of the batch's table
struct CwEntry {
    int slot, p0, u0, track;  // the lane the follower starts at, the dot length it starts from, track_speed
    float ratio;
    int pad;
    uint64_t cand;  // the lanes that may be followed
};
// the keying and timing state, in hops; u in 1/16 hop.  code 0: no element pending; sp: a character is out and its space is not
struct CwKey {
    int u, key, pend, run, code, sp;
};
// What a client carries from batch to batch.  All zero is the start; lane and k.u are set from the entry with the first batch
// (pos == 0 says so)
struct CwState {
    float part[CW_HMAX];     // the unfinished hop's samples, part[0, pos % H)
    ToneC cprev[CW_LANES];   // C of the hop before
    float A[CW_LANES];       // the followers
    float ring[CW_RING];     // e of hop b at b % 128
    uint64_t pos, nchars;
    float hi;
    int lane;
    CwKey k;
};
// One frame's record
struct CwRec {
    uint32_t nchars;
    float wpm, pitch_hz, level;
    int key, pad;
};
static_assert(sizeof(CwEntry) == 32 && sizeof(CwState) == 2352 && sizeof(CwRec) == 24 && sizeof(CwKey) == 24 &&
                  sizeof(CwTables) == sizeof(ToneTables) + 2048 + 256 + 256 + 16,
              "the device tables' layout");

// ---- the hop ------------------------------------------------------------------------------------------------------------------
// C[b][k] over the hop's H samples: toneplan.h's seed and step, the phase of stream position b H
PSDR_HOST_DEVICE inline ToneC cw_corr(const ToneTables *t, int k, uint64_t b, const float *x, int H) {
    ToneC w = tone_seed(t, tone_phase(t->inc[k], b * (uint64_t)H));
    const ToneC rot = {t->rot[k][0], t->rot[k][1]};
    ToneC acc = {0.f, 0.f};
    for (int n = 0; n < H; n++) tone_step(acc, w, rot, x[n]);
    return acc;
}
// E = |C + Cprev|^2; an energy that is not finite enters as 0 (it would stay in the followers and in hi for ever)
PSDR_HOST_DEVICE inline float cw_energy(ToneC c, ToneC cp) {
    const ToneC s = {c.re + cp.re, c.im + cp.im};
    const float E = tone_power(s);
    return tone_finite(E) ? E : 0.f;
}
// A follows E with weight 1/64
PSDR_HOST_DEVICE inline float cw_follow(float A, float E) { return fmaf(E - A, 0.015625f, A); }
// the follower moves to q only when A_q > 2 A_p
PSDR_HOST_DEVICE inline bool cw_moves(float Aq, float Ap) { return Aq > 2.f * Ap; }
// hi <- max(e, hi - hi / 128)
PSDR_HOST_DEVICE inline float cw_hi(float hi, float e) {
    const float d = fmaf(hi, -0.0078125f, hi);
    return e > d ? e : d;
}
PSDR_HOST_DEVICE inline bool cw_present(bool full, float hi, float lo, float ratio) { return full && tone_finite(hi) && hi > 0.f && hi >= ratio * lo; }
PSDR_HOST_DEVICE inline int cw_raw(bool present, float e, float hi) { return (present && e >= 0.25f * hi) ? 1 : 0; }
PSDR_HOST_DEVICE inline int cw_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
// a mark of len hops ends: dit or dah, the code, and with track the dot length a quarter of the way (floor division: >> 2 on
// the signed difference, / 3 on a length that is not negative)
PSDR_HOST_DEVICE inline void cw_mark_end(CwKey &k, int len, int track, int umin, int umax) {
    const int dah = len * 16 >= 2 * k.u ? 1 : 0;
    if (k.code == 0) k.code = 1;
    k.code = k.code >= 128 ? CW_TOO_LONG : ((k.code << 1) | dah);
    if (!track) return;
    const int target = dah ? 16 * len / 3 : 16 * len;
    k.u = cw_clamp(k.u + ((target - k.u) >> 2), umin, umax);
}
// One hop of the keying: raw is taken once it has held g = max(1, u / 64) hops, the run it starts counted from its first hop.
// Returns the characters the hop appends, at most two: the first in bits 0..7, the second in bits 8..15, 0 for none
PSDR_HOST_DEVICE inline uint32_t cw_key_step(CwKey &k, int raw, int track, int umin, int umax, const uint8_t *morse) {
    uint32_t out = 0;
    if (k.run < (1 << 26)) k.run++;  // (a silence of days: the count stands still, far beyond 5 u)
    if (raw != k.key) {
        k.pend++;
        const int g = k.u / 64 > 1 ? k.u / 64 : 1;
        if (k.pend >= g) {
            if (k.key) cw_mark_end(k, k.run - k.pend, track, umin, umax);
            k.key = raw, k.run = k.pend, k.pend = 0;
        }
    } else {
        k.pend = 0;
    }
    if (!k.key) {
        const int len16 = (k.run - k.pend) * 16;  // (hops that may belong to the next mark do not count)
        if (k.code != 0 && len16 >= 2 * k.u) {
            out = k.code >= CW_TOO_LONG ? (uint32_t)'*' : (uint32_t)morse[k.code];
            k.code = 0, k.sp = 1;
        }
        if (k.sp && len16 >= 5 * k.u) {
            out = out ? out | ((uint32_t)' ' << 8) : (uint32_t)' ';
            k.sp = 0;
        }
    }
    return out;
}
// the record behind D complete hops
PSDR_HOST_DEVICE inline CwRec cw_record(const CwTables *t, uint64_t D, uint64_t nchars, const CwKey &k, int lane, float hi) {
    if (D == 0) return CwRec{0u, 0.f, t->hz[lane], 0.f, 0, 0};
    return CwRec{(uint32_t)nchars, t->wpm[k.u], t->hz[lane], hi * t->lscale, k.key, 0};
}
// ---- the stream ---------------------------------------------------------------------------------------------------------------
// the first frame of a batch (frames of h samples from stream position pos0 on) at whose last sample D hops are complete
PSDR_HOST_DEVICE inline int cw_first_frame(uint64_t D, uint64_t pos0, int h, int H) {
    const int64_t d = (int64_t)(D * (uint64_t)H) - (int64_t)pos0;
    return d <= 0 ? 0 : ((int)d + h - 1) / h - 1;
}
// sample t of the stream during a batch that starts at pos0 with the carried partial hop (whose first sample is H b0)
PSDR_HOST_DEVICE inline float cw_sample(uint64_t t, uint64_t pos0, uint64_t b0, int H, const float *part, const float *rows, const int *flags, int h) {
    if (t < pos0) return part[t - b0 * (uint64_t)H];
    const uint32_t o = (uint32_t)(t - pos0);
    return flags[o / (uint32_t)h] ? 0.f : rows[o];
}
// lo on the host (the kernel counts over the lanes): the value of rank 16 among the ring's 128, ordered as unsigned integers on the
// bit pattern (the energies are >= +0), ties by the lower index
inline float cw_lo(const float *ring) {
    for (int i = 0; i < CW_RING; i++) {
        int rank = 0;
        for (int j = 0; j < CW_RING; j++) rank += tone_bits(ring[j]) < tone_bits(ring[i]) || (tone_bits(ring[j]) == tone_bits(ring[i]) && j < i);
        if (rank == CW_LO_RANK) return ring[i];
    }
    return 0.f;
}
// hop b's order-dependent part on the host, from the hop's 64 correlations; text: the slot's ring of CW_TEXT bytes
inline void cw_hop_step(const CwTables &t, const CwEntry &e, uint64_t b, const ToneC *C, CwState &st, uint8_t *text) {
    float E[CW_LANES];
    for (int k = 0; k < CW_LANES; k++) {
        E[k] = cw_energy(C[k], st.cprev[k]);
        st.cprev[k] = C[k];
        st.A[k] = cw_follow(st.A[k], E[k]);
    }
    int q = -1;  // the lowest candidate with the largest A
    for (int k = 0; k < CW_LANES; k++)
        if ((e.cand >> k & 1) && (q < 0 || tone_bits(st.A[k]) > tone_bits(st.A[q]))) q = k;
    if (cw_moves(st.A[q], st.A[st.lane])) st.lane = q;
    const float en = E[st.lane];
    st.hi = cw_hi(st.hi, en);
    st.ring[b % CW_RING] = en;
    const bool full = b + 1 >= CW_RING;
    const float lo = full ? cw_lo(st.ring) : 0.f;
    const int raw = cw_raw(cw_present(full, st.hi, lo, e.ratio), en, st.hi);
    for (uint32_t out = cw_key_step(st.k, raw, e.track, t.umin, t.umax, t.morse); out; out >>= 8) text[st.nchars++ % CW_TEXT] = (uint8_t)out;
}
// A client's batch on the host, as k_audio_cw runs it: rows[nframes * h] and flags[nframes] are read, st and text carried,
// rec[nframes] written
inline void cw_stream(const CwTables &t, const CwEntry &e, const float *rows, const int *flags, int h, int nframes, CwState &st, uint8_t *text, CwRec *rec) {
    const int H = t.H;
    const uint64_t pos0 = st.pos, L = (uint64_t)nframes * (uint64_t)h, b0 = pos0 / H, b1 = (pos0 + L) / H;
    if (pos0 == 0) st.lane = e.p0, st.k.u = e.u0;
    auto emit = [&](uint64_t D) {  // the frames at whose end D hops are complete
        const int lo = cw_first_frame(D, pos0, h, H), hi = std::min(nframes, cw_first_frame(D + 1, pos0, h, H));
        for (int f = lo; f < hi; f++) rec[f] = cw_record(&t, D, st.nchars, st.k, st.lane, st.hi);
    };
    emit(b0);
    float x[CW_HMAX];
    ToneC C[CW_LANES];
    for (uint64_t b = b0; b < b1; b++) {
        for (int n = 0; n < H; n++) x[n] = cw_sample(b * H + n, pos0, b0, H, st.part, rows, flags, h);
        for (int k = 0; k < CW_LANES; k++) C[k] = cw_corr(&t.t, k, b, x, H);
        cw_hop_step(t, e, b, C, st, text);
        emit(b + 1);
    }
    float part[CW_HMAX] = {};
    for (uint64_t u = b1 * H; u < pos0 + L; u++) part[u - b1 * H] = cw_sample(u, pos0, b0, H, st.part, rows, flags, h);
    memcpy(st.part, part, sizeof(part));
    st.pos = pos0 + L;
}

// ---- the call -----------------------------------------------------------------------------------------------------------------
// psdr_client_set_cw_decoder's refusals, in the order they are looked for; cfg == null switches it off (an IQ client may)
enum CwVerdict { CW_OK, CW_BAD_ID, CW_INACTIVE, CW_IQ, CW_BAD_PITCH, CW_BAD_SEARCH, CW_BAD_WPM, CW_BAD_TRACK, CW_BAD_SNR, CW_BAD_RATE };
inline bool cw_inside(double v, double lo, double hi) { return std::isfinite(v) && v >= lo && v <= hi; }
inline CwVerdict cw_check(const AudioSlot *slots, size_t S, int id, const psdr_cw_config *cfg, int audio_rate) {
    if (id < 0 || (size_t)id >= S) return CW_BAD_ID;
    if (!slots[id].active) return CW_INACTIVE;
    if (!cfg) return CW_OK;
    if (slots[id].mode == PSDR_IQ) return CW_IQ;
    if (!cw_inside(cfg->pitch_hz, CW_PITCH_MIN, CW_PITCH_MAX)) return CW_BAD_PITCH;
    if (!cw_inside(cfg->search_hz, CW_SEARCH_MIN, CW_SEARCH_MAX)) return CW_BAD_SEARCH;
    if (!cw_inside(cfg->wpm, CW_WPM_MIN, CW_WPM_MAX)) return CW_BAD_WPM;
    if (cfg->track_speed != 0 && cfg->track_speed != 1) return CW_BAD_TRACK;
    if (!cw_inside(cfg->snr_db, CW_SNR_MIN, CW_SNR_MAX)) return CW_BAD_SNR;
    if (audio_rate < CW_RATE_MIN || audio_rate > CW_RATE_MAX) return CW_BAD_RATE;
    return CW_OK;
}
// ... and what an accepted call does to the slot: switching it ON - from off, or again - starts the state from zero at the
// client's next listed batch (also while paused)
inline void cw_apply(AudioSlot &s, const psdr_cw_config *cfg, int audio_rate) {
    s.cw_on = cfg ? 1 : 0;
    if (!cfg) return;
    s.cw_p0 = cw_nearest(cfg->pitch_hz), s.cw_cand = cw_candidates(cfg->pitch_hz, cfg->search_hz);
    s.cw_u0 = cw_u_of(cfg->wpm, (double)audio_rate), s.cw_track = cfg->track_speed;
    s.cw_ratio = tone_ratio(cfg->snr_db);
    s.cw_fresh = true;
}
// psdr_cw_defaults
inline bool cw_defaults(double audio_rate, psdr_cw_config *out) {
    if (!out || !(audio_rate >= CW_RATE_MIN && audio_rate <= CW_RATE_MAX)) return false;
    out->pitch_hz = CW_PITCH_DEFAULT, out->search_hz = CW_SEARCH_DEFAULT, out->wpm = CW_WPM_DEFAULT;
    out->track_speed = 1, out->snr_db = CW_SNR_DEFAULT;
    return true;
}

// ---- the batch ----------------------------------------------------------------------------------------------------------------
struct CwPlan {
    int n = 0;                 // table[0, n): the batch's CW clients, in slot order
    std::vector<size_t> zero;  // slots whose state and text start this batch from zero
    bool any() const { return n > 0; }  // no such client in the batch: nothing is uploaded, zeroed or launched
};
// One batch, behind demod_plan(): tone_plan with other fields.  Of the clients the batch demodulated the ones with the decoder on
// whose kind wrote audio rows are listed; the state starts from zero when the call switched it on since the client's last listed
// batch, on a mode change and on a retune.  An IQ client and a paused one keep setting, state and a pending fresh start.
// b_cw_on: the last batch ran with the decoder for this client (psdr_read_cw)
inline CwPlan cw_plan(AudioSlot *slots, size_t S, uint64_t demod_seq, CwEntry *table) {
    CwPlan p;
    for (size_t i = 0; i < S; i++) {
        AudioSlot &s = slots[i];
        if (!s.active || s.paused || s.last_seq != demod_seq) continue;
        s.b_cw_on = false;
        if (s.b_mode == PSDR_IQ || !s.cw_on) continue;
        s.b_cw_on = true;
        const int m = (int)std::floor(s.b_mid);
        if (s.cw_fresh || s.cw_mode != s.b_mode || s.cw_l != s.b_l || s.cw_r != s.b_r || s.cw_m != m) p.zero.push_back(i);
        s.cw_fresh = false;
        s.cw_mode = s.b_mode, s.cw_l = s.b_l, s.cw_r = s.b_r, s.cw_m = m;
        table[p.n++] = CwEntry{(int)i, s.cw_p0, s.cw_u0, s.cw_track, s.cw_ratio, 0, s.cw_cand};
    }
    return p;
}

}  // namespace psdr

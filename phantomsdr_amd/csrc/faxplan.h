// faxplan.h - the per-client radiofax decoder (include/psdr.h: psdr_client_set_fax_decoder), everything of it that is not a launch:
// the ONE definition of the discriminator, the line and column of a sample, the pixel, the tone blocks, the start / phasing / image
// machine, the phasing search's decision, the records and the stream's bookkeeping (k_audio_fax in fax.h and the host tests run
// this text), the tables, the argument validation, the defaults and fax_plan(), which walks the audio slots behind demod_plan() and
// says who is listed in the batch and whose state starts from zero.  Plain C++17 (no HIP): tests/test_fax_host.py builds it with
// the host compiler.
//
// The rule is written out in include/psdr.h.  Phases, seeds and the per-sample rotation are toneplan.h's functions, the hop is
// rttyplan.h's, the frames of a hop cwplan.h's.  Every f32 operation is an explicit fmaf, a lone multiply, a lone add or one of the
// stated divisions (the angle's quotient, the pixel's mean, a block's rho and mean), so contraction has nothing to fuse; line,
// column, counters, machine and phasing search are integer arithmetic.
#pragma once
#include "rttyplan.h"

namespace psdr {

constexpr int FAX_IDLE = 0, FAX_PHASING = 1, FAX_IMAGE = 2;  // the machine's states, as records and meta hold them
constexpr int FAX_HMAX = RTTY_HMAX;     // the longest hop
constexpr int FAX_ZT = 80;              // samples of z the state keeps: the boxcar reaches K - 1 <= 59 back
constexpr int FAX_YT = 16;              // samples of y the state keeps: the delay D <= 15
constexpr int FAX_WIDTH_MIN = 256, FAX_WIDTH_MAX = 2048, FAX_WIDTH_DEFAULT = 1024;
constexpr int FAX_PIXEL_MAX = 64;       // samples per pixel: 1 to 64
constexpr int FAX_RING_MIN = 64;        // lines the ring holds at least
constexpr int FAX_PHASING_MAX = 80;     // lines of phasing without a complete run before the image is taken as it comes
constexpr int FAX_RATE_MIN = RTTY_RATE_MIN, FAX_RATE_MAX = RTTY_RATE_MAX;
constexpr double FAX_TONE_MIN = 300.0, FAX_TONE_MAX = 3400.0, FAX_SHIFT_MIN = 200.0, FAX_SHIFT_MAX = 1600.0;
constexpr double FAX_BLACK_DEFAULT = 1500.0, FAX_WHITE_DEFAULT = 2300.0, FAX_LPM_DEFAULT = 120.0;
constexpr double FAX_SLANT_MAX = 2000.0, FAX_TOP = 0.45, FAX_GUARD = 300.0;
constexpr double FAX_TONE_HZ[3] = {300.0, 450.0, 675.0};  // start (IOC 576), stop, start (IOC 288)
constexpr float FAX_HALF_PI = 1.57079637f;

// K, D, NB and Lq of the rule, in double
inline int fax_k_of(double centre, double audio_rate) {
    const int k = (int)std::floor(audio_rate / (2.0 * centre) + 0.5);
    return k < 2 ? 2 : k;
}
inline int fax_d_of(double audio_rate) {
    const int d = (int)std::floor(audio_rate / 3200.0);
    return d < 1 ? 1 : d;
}
inline int fax_nb_of(double audio_rate) { return (int)std::floor(audio_rate / (8.0 * rtty_hop(audio_rate)) + 0.5); }
inline uint64_t fax_lq_of(double lpm, double slant_ppm, double audio_rate) {
    return (uint64_t)std::floor(65536.0 * 60.0 * audio_rate / lpm * (1.0 + slant_ppm * 1e-6) + 0.5);
}
// lines the ring holds: 2 more than the largest batch (max_samples of the stream) can complete, 64 at least
inline int fax_ring_of(uint64_t Lq, uint64_t max_samples) {
    const uint64_t r = 2 + (max_samples * 65536u) / Lq + 1;
    return r < (uint64_t)FAX_RING_MIN ? FAX_RING_MIN : (int)r;
}
// ... and of any client the call accepts in this context: what the context's first fax client allocates per slot
inline int fax_ring_max(double audio_rate, uint64_t max_samples) { return fax_ring_of(fax_lq_of(240.0, -FAX_SLANT_MAX, audio_rate), max_samples); }

// The tables of the context: the seed tables (of t, inc, rot, h, nb and lscale are not used) and the hop
struct FaxTables {
    ToneTables t;
    int H, pad;
};
inline void fax_tables(FaxTables &c, double audio_rate) {
    memset(&c, 0, sizeof(c));
    tone_seed_tables(c.t);
    c.H = rtty_hop(audio_rate);
}
// (One entry of the batch's table, FaxEntry, is demodplan.h's: the slot keeps it as the table holds it)
// One frame's record
struct FaxRec {
    uint32_t nlines;
    int state;
    uint32_t image;
    int ioc;
    float offset_hz, tone_quality;
};
// The machine: what the work-group and the host carry as plain values.  All zero is the start; fax_start() sets what is not zero
// with the first batch (pos == 0 says so)
struct FaxScalars {
    uint64_t nlines;   // kept lines
    uint64_t lstart;   // the line being built covers 65536 t + Lq in [lstart, lstart + Lq)
    float psum, F, quality;
    int pcnt, pcol;    // the unfinished pixel: its samples' sum, their count, its column (-1: none)
    ToneC S[3];        // the block's sums of the hops' correlations
    float SQ, SM;
    int nhop, cnt[3];
    int state, ioc;
    uint32_t image;
    int skip;          // the line being built is a partial one (before the first origin, behind a move): it is not looked at
    int run, prevc, plines, ilines;
    int rrow;          // nlines % R: the ring's row of the next kept line
};
// What a client carries from batch to batch
struct FaxState {
    ToneC zt[FAX_ZT];            // z[pos - 80 + i]
    ToneC yt[FAX_YT];            // y[pos - 16 + i]
    float vpart[FAX_HMAX];       // the unfinished hop's v, vpart[0, pos % H)
    uint8_t line[FAX_WIDTH_MAX]; // the line being built
    uint64_t pos;
    FaxScalars z;
    FaxRec last;                 // the record behind the last complete hop
};
static_assert(sizeof(FaxEntry) == 128 && sizeof(FaxRec) == 24 && sizeof(FaxScalars) == 120 && sizeof(FaxState) == 3224 && sizeof(FaxTables) == sizeof(ToneTables) + 8,
              "the device tables' layout");

// ---- the discriminator --------------------------------------------------------------------------------------------------------
// w of sample t: the seed at the exact phase of the hop's first sample, then one rotation per sample
PSDR_HOST_DEVICE inline ToneC fax_w(const ToneTables *t, uint32_t inc, ToneC rot, uint64_t at, int H) {
    const int n = (int)(at & (uint64_t)(H - 1));  // (H is a power of two)
    ToneC w = tone_seed(t, tone_phase(inc, at - (uint64_t)n));
    for (int i = 0; i < n; i++) w = tone_cmul(w, rot);
    return w;
}
PSDR_HOST_DEVICE inline ToneC fax_z(float x, ToneC w) { return ToneC{x * w.re, -x * w.im}; }
// y[t] = sum_{i < K} z[t - i], i ascending; Z(i): z[t - i]
template <class Zs>
PSDR_HOST_DEVICE inline ToneC fax_y(int K, Zs Z) {
    ToneC y = {0.f, 0.f};
    for (int i = 0; i < K; i++) {
        const ToneC z = Z(i);
        y.re = y.re + z.re, y.im = y.im + z.im;
    }
    return y;
}
// the angle of d in (-pi/2, pi/2): ONE division, of the smaller part by the larger, so that the quotient lies in [-1, 1] - a
// clamped tangent cannot reach the +-pi/2 a shift of 1600 Hz needs at a rate that is a multiple of 3200 -, then
// Abramowitz and Stegun's 4.4.49, an odd polynomial of degree 17; re <= 0 or a part that is not finite saturates by the sign of im
PSDR_HOST_DEVICE inline float fax_angle(float re, float im) {
    const float sat = im > 0.f ? FAX_HALF_PI : im < 0.f ? -FAX_HALF_PI : 0.f;
    if (!(tone_finite(re) && tone_finite(im)) || !(re > 0.f)) return sat;
    const bool swap = fabsf(im) > re;
    float q = swap ? re / im : im / re;
    q = q > 1.f ? 1.f : q < -1.f ? -1.f : q;
    const float s = q * q;
    float p = fmaf(0.0028662257f, s, -0.0161657367f);
    p = fmaf(p, s, 0.0429096138f);
    p = fmaf(p, s, -0.0752896400f);
    p = fmaf(p, s, 0.1065626393f);
    p = fmaf(p, s, -0.1420889944f);
    p = fmaf(p, s, 0.1999355085f);
    p = fmaf(p, s, -0.3333314528f);
    p = fmaf(p, s, 1.0f);
    const float a = q * p;
    return swap ? sat + -a : a;
}
// v[t] from y[t] and y[t - D]
PSDR_HOST_DEVICE inline float fax_v(ToneC y, ToneC yd, float s) {
    const float dre = fmaf(y.re, yd.re, y.im * yd.im);
    const float dim = fmaf(y.im, yd.re, -(y.re * yd.im));
    const float v = fmaf(fax_angle(dre, dim), s, 0.5f);
    return v < 0.f ? 0.f : v > 1.f ? 1.f : v;
}
// ---- line, column, pixel ------------------------------------------------------------------------------------------------------
PSDR_HOST_DEVICE inline uint64_t fax_tq(uint64_t t, uint64_t Lq) { return 65536u * t + Lq; }
// floor((tq - lstart) width / Lq), exactly: the f32 quotient of a numerator below 2^43 and an Lq below 2^32 is off by less than
// 0.001 of a column, so one step either way sets it right (a 64-bit division would cost the kernel its registers)
PSDR_HOST_DEVICE inline int fax_col(uint64_t tq, uint64_t lstart, uint64_t Lq, int width) {
    const uint64_t num = (tq - lstart) * (uint64_t)width;
    uint32_t q = (uint32_t)((float)num / (float)Lq);
    if ((uint64_t)q * Lq > num)
        q--;
    else if ((uint64_t)(q + 1u) * Lq <= num)
        q++;
    return (int)q < width ? (int)q : width - 1;  // (q < width whenever the sample lies in the line)
}
// floor(a Lq / width) for a column a < 2048 and Lq < 2^32, in 32-bit steps
PSDR_HOST_DEVICE inline uint64_t fax_col_start(int a, uint64_t Lq, int width) {
    const uint32_t l = (uint32_t)Lq, w = (uint32_t)width;
    return (uint64_t)a * (uint64_t)(l / w) + (uint64_t)((uint32_t)a * (l % w) / w);
}
// the first sample behind the line being built
PSDR_HOST_DEVICE inline uint64_t fax_line_stop(uint64_t lstart) { return (lstart + 65535u) >> 16; }
PSDR_HOST_DEVICE inline uint8_t fax_byte(float sum, int cnt) {
    const float p = sum / (float)cnt;
    const int b = (int)fmaf(255.f, p, 0.5f);
    return (uint8_t)(b > 255 ? 255 : b);
}
// the start: the line grid stands at origin0 (the samples before it are a partial line), FREE reads an image from sample 0
PSDR_HOST_DEVICE inline void fax_start(FaxScalars &z, const FaxEntry &e) {
    z.pcol = -1, z.prevc = -1;
    z.state = e.mode == PSDR_FAX_FREE ? FAX_IMAGE : FAX_IDLE;
    z.lstart = e.origin0 ? e.origin0 : e.Lq;
    z.skip = e.origin0 ? 1 : 0;
}
PSDR_HOST_DEVICE inline FaxRec fax_record(const FaxScalars &z, const FaxEntry &e) {
    return FaxRec{(uint32_t)z.nlines, z.state, z.image, z.ioc, e.shift * z.F, z.quality};
}
// ---- tones --------------------------------------------------------------------------------------------------------------------
// one hop's part: r[0..5] the three correlations of v - 0.5, r[6] = Q, r[7] = M; V(n): the hop's v
template <class Vs>
PSDR_HOST_DEVICE inline ToneC fax_tone_corr(const ToneTables *t, uint32_t inc, ToneC rot, uint64_t b, int H, Vs V) {
    ToneC w = tone_seed(t, tone_phase(inc, b * (uint64_t)H));
    ToneC acc = {0.f, 0.f};
    for (int n = 0; n < H; n++) tone_step(acc, w, rot, V(n) + -0.5f);
    return acc;
}
template <class Vs>
PSDR_HOST_DEVICE inline void fax_tone_qm(int H, Vs V, float &Q, float &M) {
    Q = 0.f, M = 0.f;
    for (int n = 0; n < H; n++) {
        const float u = V(n) + -0.5f;
        Q = fmaf(u, u, Q);
        M = M + u;
    }
}
PSDR_HOST_DEVICE inline void fax_clear_counters(FaxScalars &z) { z.cnt[0] = z.cnt[1] = z.cnt[2] = 0; }
// a hop's end in PSDR_FAX_AUTO: the block's sums and, with its last hop, the decision, the counters and the machine
PSDR_HOST_DEVICE inline void fax_hop_step(FaxScalars &z, const FaxEntry &e, const float *r) {
    for (int k = 0; k < 3; k++) z.S[k].re = z.S[k].re + r[2 * k], z.S[k].im = z.S[k].im + r[2 * k + 1];
    z.SQ = z.SQ + r[6], z.SM = z.SM + r[7];
    if (++z.nhop < e.NB) return;
    const float den = e.nbh * z.SQ;
    float top = 0.f;  // the largest rho and the lowest tone that has it (rho >= +0)
    int best = 0;
    for (int k = 0; k < 3; k++) {
        const float q = (2.f * fmaf(z.S[k].re, z.S[k].re, z.S[k].im * z.S[k].im)) / den;
        const float rho = tone_finite(q) ? q : 0.f;
        if (rho > top) top = rho, best = k;
    }
    z.quality = top;
    const int hit = top >= e.ratio ? best : -1;
    for (int k = 0; k < 3; k++) {
        const int c = z.cnt[k] + (k == hit ? 1 : -1);
        z.cnt[k] = c < 0 ? 0 : c > 2 * e.start_blocks ? 2 * e.start_blocks : c;
    }
    if (hit >= 0) z.F = fmaf(z.SM / e.nbh - z.F, 0.125f, z.F);
    if (z.cnt[1] >= e.start_blocks) {
        z.state = FAX_IDLE;
        fax_clear_counters(z);
    } else if (z.state == FAX_IDLE && (z.cnt[0] >= e.start_blocks || z.cnt[2] >= e.start_blocks)) {
        z.ioc = z.cnt[0] >= e.start_blocks ? 576 : 288;
        z.state = FAX_PHASING, z.image++;
        z.run = 0, z.prevc = -1, z.plines = 0, z.ilines = 0;
        fax_clear_counters(z);
    }
    for (int k = 0; k < 3; k++) z.S[k] = ToneC{0.f, 0.f};
    z.SQ = 0.f, z.SM = 0.f, z.nhop = 0;
}
// ---- a completed line ---------------------------------------------------------------------------------------------------------
// in PHASING, behind the search (dev: the largest window sum in the pulse's measure, c its lowest column, total: the whole line in
// that measure): returns how far the origin moves, in 1/65536 sample (0: it stays)
PSDR_HOST_DEVICE inline uint64_t fax_phase_step(FaxScalars &z, const FaxEntry &e, int dev, int c, int total) {
    const bool valid = dev >= 192 * e.wp && total - dev <= 64 * (e.width - e.wp);
    if (valid) {
        int d = c > z.prevc ? c - z.prevc : z.prevc - c;
        if (d > e.width - d) d = e.width - d;
        z.run = (z.prevc >= 0 && d <= e.width / 64) ? z.run + 1 : 1;
        z.prevc = c;
    } else {
        z.run = 0, z.prevc = -1;
    }
    z.plines++;
    if (z.run >= e.phase_lines) {
        z.state = FAX_IMAGE;
        const int a = c + e.wp / 2;
        return fax_col_start(a >= e.width ? a - e.width : a, e.Lq, e.width);
    }
    if (z.plines >= FAX_PHASING_MAX) z.state = FAX_IMAGE;
    return 0;
}
// in IMAGE, behind the line's copy into ring row nlines % R: its meta, and the count
PSDR_HOST_DEVICE inline uint32_t fax_keep(FaxScalars &z, const FaxEntry &e) {
    const uint32_t meta = z.image << 8 | (uint32_t)z.state;
    z.nlines++, z.ilines++;
    z.rrow = z.rrow + 1 == e.R ? 0 : z.rrow + 1;
    if (e.max_lines && z.ilines >= e.max_lines) z.state = FAX_IDLE;
    return meta;
}
// the grid behind a completed line: the next line, or - behind a move - the partial line in front of the new origin
PSDR_HOST_DEVICE inline void fax_next_line(FaxScalars &z, const FaxEntry &e, uint64_t move) {
    z.lstart += move ? move : e.Lq;
    if (move) z.skip = 1;
}
// the phasing search on the host (the work-group does the same with its threads): the line's measure, the largest circular window
// sum and its lowest column
inline void fax_search(const uint8_t *pix, int width, int wp, int &dev, int &c, int &total) {
    int sum = 0;
    for (int i = 0; i < width; i++) sum += pix[i];
    const bool dark = 2 * sum >= 255 * width;  // a bright line: the pulse is dark
    dev = -1, c = 0;
    for (int j = 0; j < width; j++) {
        int win = 0;
        for (int i = 0; i < wp; i++) win += pix[(j + i) % width];
        const int d = dark ? 255 * wp - win : win;
        if (d > dev) dev = d, c = j;
    }
    total = dark ? 255 * width - sum : sum;
}

// ---- the stream ---------------------------------------------------------------------------------------------------------------
// A client's batch on the host, sample by sample: rows[nframes * h] and flags[nframes] are read, st, ring[R * width] and meta[R]
// carried, rec[nframes] written
inline void fax_stream(const FaxTables &t, const FaxEntry &e, const float *rows, const int *flags, int h, int nframes, FaxState &st, uint8_t *ring, uint32_t *meta,
                       FaxRec *rec) {
    const int H = t.H;
    const uint64_t pos0 = st.pos, L = (uint64_t)nframes * (uint64_t)h, b0 = pos0 / H;
    FaxScalars z = st.z;
    if (pos0 == 0) fax_start(z, e), st.last = fax_record(z, e);
    auto emit = [&](uint64_t D) {
        const int lo = cw_first_frame(D, pos0, h, H), hi = std::min(nframes, cw_first_frame(D + 1, pos0, h, H));
        for (int f = lo; f < hi; f++) rec[f] = st.last;
    };
    emit(b0);
    const ToneC rot = {e.rot[0], e.rot[1]};
    std::vector<ToneC> zs(FAX_ZT + L), ys(FAX_YT + L);  // zs[i] = z[pos0 - 80 + i], ys[i] = y[pos0 - 16 + i]
    memcpy(zs.data(), st.zt, sizeof(st.zt));
    memcpy(ys.data(), st.yt, sizeof(st.yt));
    float vh[FAX_HMAX];
    memcpy(vh, st.vpart, sizeof(vh));
    for (uint64_t u = 0; u < L; u++) {
        const uint64_t at = pos0 + u;
        const float x = flags[u / (uint64_t)h] ? 0.f : rows[u];
        const ToneC *zp = &(zs[FAX_ZT + u] = fax_z(x, fax_w(&t.t, e.inc, rot, at, H)));
        const ToneC y = ys[FAX_YT + u] = fax_y(e.K, [&](int i) { return zp[-i]; });
        const float v = fax_v(y, ys[FAX_YT + u - e.D], e.s);
        // the line and the pixel
        const uint64_t tq = fax_tq(at, e.Lq);
        while (tq >= z.lstart + e.Lq) {
            if (z.pcnt) st.line[z.pcol] = fax_byte(z.psum, z.pcnt);
            z.pcnt = 0, z.psum = 0.f, z.pcol = -1;
            uint64_t move = 0;
            if (z.skip) {
                z.skip = 0;
            } else if (z.state == FAX_PHASING) {
                int dev, c, total;
                fax_search(st.line, e.width, e.wp, dev, c, total);
                move = fax_phase_step(z, e, dev, c, total);
            } else if (z.state == FAX_IMAGE) {
                const size_t r = (size_t)z.rrow;
                memcpy(ring + r * e.width, st.line, e.width);
                meta[r] = fax_keep(z, e);
            }
            fax_next_line(z, e, move);
        }
        const int col = fax_col(tq, z.lstart, e.Lq, e.width);
        if (col != z.pcol) {
            if (z.pcnt) st.line[z.pcol] = fax_byte(z.psum, z.pcnt);
            z.pcol = col, z.psum = 0.f, z.pcnt = 0;
        }
        z.psum = z.psum + v, z.pcnt++;
        // the hop
        const int n = (int)(at % H);
        vh[n] = v;
        if (n == H - 1) {
            const uint64_t b = at / H;
            if (e.mode == PSDR_FAX_AUTO) {
                float r[8];
                for (int k = 0; k < 3; k++) {
                    const ToneC c = fax_tone_corr(&t.t, e.tinc[k], ToneC{e.trot[k][0], e.trot[k][1]}, b, H, [&](int i) { return vh[i]; });
                    r[2 * k] = c.re, r[2 * k + 1] = c.im;
                }
                fax_tone_qm(H, [&](int i) { return vh[i]; }, r[6], r[7]);
                fax_hop_step(z, e, r);
            }
            st.last = fax_record(z, e);
            emit(b + 1);
        }
    }
    memcpy(st.zt, zs.data() + L, sizeof(st.zt));
    memcpy(st.yt, ys.data() + L, sizeof(st.yt));
    const int left = (int)((pos0 + L) % H);
    for (int i = 0; i < FAX_HMAX; i++) st.vpart[i] = i < left ? vh[i] : 0.f;
    st.z = z, st.pos = pos0 + L;
}

// ---- the call -----------------------------------------------------------------------------------------------------------------
// psdr_client_set_fax_decoder's refusals, in the order they are looked for; cfg == null switches it off (an IQ client may)
enum FaxVerdict { FAX_OK, FAX_BAD_ID, FAX_INACTIVE, FAX_IQ, FAX_BAD_MODE, FAX_BAD_TONES, FAX_BAD_LPM, FAX_BAD_WIDTH, FAX_BAD_SLANT, FAX_BAD_PHASE_COL, FAX_BAD_RATIO,
                  FAX_BAD_START, FAX_BAD_PHASE_LINES, FAX_BAD_MAX_LINES, FAX_BAD_RATE, FAX_BAD_BAND, FAX_BAD_PIXEL };
inline FaxVerdict fax_check(const AudioSlot *slots, size_t S, int id, const psdr_fax_config *cfg, int audio_rate) {
    if (id < 0 || (size_t)id >= S) return FAX_BAD_ID;
    if (!slots[id].active) return FAX_INACTIVE;
    if (!cfg) return FAX_OK;
    if (slots[id].mode == PSDR_IQ) return FAX_IQ;
    if (cfg->mode != PSDR_FAX_AUTO && cfg->mode != PSDR_FAX_FREE) return FAX_BAD_MODE;
    if (!cw_inside(cfg->black_hz, FAX_TONE_MIN, FAX_TONE_MAX) || !cw_inside(cfg->white_hz, FAX_TONE_MIN, FAX_TONE_MAX) ||
        !cw_inside(std::fabs(cfg->white_hz - cfg->black_hz), FAX_SHIFT_MIN, FAX_SHIFT_MAX))
        return FAX_BAD_TONES;
    if (!(cfg->lpm == 60.0 || cfg->lpm == 90.0 || cfg->lpm == 120.0 || cfg->lpm == 240.0)) return FAX_BAD_LPM;
    if (cfg->width < FAX_WIDTH_MIN || cfg->width > FAX_WIDTH_MAX) return FAX_BAD_WIDTH;
    if (!cw_inside(cfg->slant_ppm, -FAX_SLANT_MAX, FAX_SLANT_MAX)) return FAX_BAD_SLANT;
    if (cfg->phase_col < 0 || cfg->phase_col >= cfg->width) return FAX_BAD_PHASE_COL;
    if (!(std::isfinite(cfg->tone_ratio) && cfg->tone_ratio > 0 && cfg->tone_ratio < 1)) return FAX_BAD_RATIO;
    if (cfg->start_blocks < 2 || cfg->start_blocks > 64) return FAX_BAD_START;
    if (cfg->phase_lines < 2 || cfg->phase_lines > 32) return FAX_BAD_PHASE_LINES;
    if (cfg->max_lines < 0) return FAX_BAD_MAX_LINES;
    if (audio_rate < FAX_RATE_MIN || audio_rate > FAX_RATE_MAX) return FAX_BAD_RATE;
    if (std::max(cfg->black_hz, cfg->white_hz) + FAX_GUARD > FAX_TOP * audio_rate) return FAX_BAD_BAND;
    const uint64_t Lq = fax_lq_of(cfg->lpm, cfg->slant_ppm, (double)audio_rate), px = 65536u * (uint64_t)cfg->width;
    if (Lq < px || Lq > FAX_PIXEL_MAX * px) return FAX_BAD_PIXEL;
    return FAX_OK;
}
// ... and what an accepted call does to the slot: switching it ON - from off, or again - starts the state from zero at the
// client's next listed batch (also while paused).  max_samples: the samples of the context's largest batch
inline void fax_apply(AudioSlot &s, const psdr_fax_config *cfg, int audio_rate, uint64_t max_samples) {
    s.fax_on = cfg ? 1 : 0;
    if (!cfg) return;
    const double rate = (double)audio_rate, centre = (cfg->black_hz + cfg->white_hz) / 2.0, shift = cfg->white_hz - cfg->black_hz;
    FaxEntry &e = s.fax;
    memset(&e, 0, sizeof(e));
    e.mode = cfg->mode, e.width = cfg->width, e.K = fax_k_of(centre, rate), e.D = fax_d_of(rate), e.NB = fax_nb_of(rate);
    e.start_blocks = cfg->start_blocks, e.phase_lines = cfg->phase_lines, e.max_lines = cfg->max_lines;
    e.wp = std::max(1, cfg->width / 20);
    e.Lq = fax_lq_of(cfg->lpm, cfg->slant_ppm, rate);
    e.origin0 = (uint64_t)cfg->phase_col * e.Lq / (uint64_t)cfg->width;
    e.R = fax_ring_of(e.Lq, max_samples);
    tone_inc_rot(centre, rate, e.inc, e.rot);
    for (int k = 0; k < 3; k++) tone_inc_rot(FAX_TONE_HZ[k], rate, e.tinc[k], e.trot[k]);
    e.s = (float)(rate / (2.0 * M_PI * e.D * shift));
    e.ratio = (float)cfg->tone_ratio, e.shift = (float)shift, e.nbh = (float)(e.NB * rtty_hop(rate));
    s.fax_fresh = true;
}
// psdr_fax_defaults: 120 lines per minute, 1500 / 2300 Hz, 1024 pixels; below 5778 Hz the tones do not fit and the call says so
inline bool fax_defaults(double audio_rate, psdr_fax_config *out) {
    if (!out || !(audio_rate >= FAX_RATE_MIN && audio_rate <= FAX_RATE_MAX)) return false;
    out->mode = PSDR_FAX_AUTO, out->black_hz = FAX_BLACK_DEFAULT, out->white_hz = FAX_WHITE_DEFAULT, out->lpm = FAX_LPM_DEFAULT;
    out->width = FAX_WIDTH_DEFAULT, out->slant_ppm = 0.0, out->phase_col = 0, out->tone_ratio = PSDR_FAX_TONE_RATIO_DEFAULT;
    out->start_blocks = 8, out->phase_lines = 4, out->max_lines = 0;
    return true;
}

// ---- the batch ----------------------------------------------------------------------------------------------------------------
struct FaxPlan {
    int n = 0;                 // table[0, n): the batch's fax clients, in slot order
    std::vector<size_t> zero;  // slots whose state starts this batch from zero
    bool any() const { return n > 0; }  // no such client in the batch: nothing is uploaded, zeroed or launched
};
// One batch, behind demod_plan(): psk_plan with other fields
inline FaxPlan fax_plan(AudioSlot *slots, size_t S, uint64_t demod_seq, FaxEntry *table) {
    FaxPlan p;
    for (size_t i = 0; i < S; i++) {
        AudioSlot &s = slots[i];
        if (!s.active || s.paused || s.last_seq != demod_seq) continue;
        s.b_fax_on = false;
        if (s.b_mode == PSDR_IQ || !s.fax_on) continue;
        s.b_fax_on = true;
        const int m = (int)std::floor(s.b_mid);
        if (s.fax_fresh || s.fax_mode != s.b_mode || s.fax_l != s.b_l || s.fax_r != s.b_r || s.fax_m != m) p.zero.push_back(i);
        s.fax_fresh = false;
        s.fax_mode = s.b_mode, s.fax_l = s.b_l, s.fax_r = s.b_r, s.fax_m = m;
        table[p.n] = s.fax;
        table[p.n++].slot = (int)i;
    }
    return p;
}

}  // namespace psdr

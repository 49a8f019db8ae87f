// createplan.h - what psdr_create decides, resolved in pure functions of the config and a few facts: which configs it
// accepts (create_check), the split M = M1 * M2 and everything that hangs off it (shape_plan), every create-time buffer
// (buffer_plan), the twiddle tables (twiddle_plan), the audio clients' inverse DFT (idft_plan) and the band regions of
// psdr_set_band_layout (band_plan).  Plain host C++17 (no HIP, no getenv, no allocation): context.hip adopts the plans,
// tests/test_create_plan.py prints them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/psdr.h"
#include "demodplan.h"
#include "forwardplan.h"
#include "layout.h"
#include "types.h"

namespace psdr {

// an answer of the C-ABI: the code and what psdr_last_error() says
struct PlanStatus {
    int code = PSDR_OK;
    std::string msg;
};
inline PlanStatus plan_fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return PlanStatus{code, buf};
}

// every argument rejection of psdr_create that needs no device, in the order they are answered
inline PlanStatus create_check(const psdr_config &g) {
    const size_t N = g.fft_size;
    if (N == 0 || (N & (N - 1))) return plan_fail(PSDR_ERR_INVALID, "fft_size must be a power of two");
    const size_t M = g.is_real ? N / 2 : N;
    if (ilog2(M) < 12 || ilog2(M) > 22)
        return plan_fail(PSDR_ERR_UNSUPPORTED, "fft_size %zu unsupported: complex transform length must be 2^12..2^22", N);
    if (g.downsample_levels < 1 || ((M >> (g.downsample_levels - 1)) < 1))
        return plan_fail(PSDR_ERR_INVALID, "downsample_levels %d invalid", g.downsample_levels);
    if (g.audio_fft_size < 0 || (g.audio_fft_size % 4) != 0)
        return plan_fail(PSDR_ERR_INVALID, "audio_fft_size must be a non-negative multiple of 4");
    if (g.input_format < PSDR_FMT_U8 || g.input_format > PSDR_FMT_F64) return plan_fail(PSDR_ERR_INVALID, "unknown input_format %d", g.input_format);
    if (g.max_batch < 1) return plan_fail(PSDR_ERR_INVALID, "max_batch must be >= 1");
    if (g.waterfall_size < 0) return plan_fail(PSDR_ERR_INVALID, "waterfall_size must be >= 0");
    return {};
}

// the run-time knobs (ctx.h) as facts: psdr_create reads the environment once and fills this
struct CreateEnv {
    bool real_split_2048x1024 = false;  // PSDR_REAL_SPLIT=2048x1024: round 4's split of 2^22-point real frames
    bool real_3pass = false;            // PSDR_REAL_3PASS: the three-pass real path
    int seg_len = 0;                    // PSDR_SEG_LEN (0: unset)
    bool demod_chain = true;            // PSDR_DEMOD_CHAIN
    int demod_chain_k = 0;              // PSDR_DEMOD_K (0: unset)
    int log2M2 = 0;                     // PSDR_LOG2M2 of a tuning build (0: unset)
    int num_cus = 256;
};

constexpr unsigned TICKET_SLOTS = 64;
// tile widths: T = min(16384/L, other dimension)
inline int pick_T(int L, int other) { return std::min(16384 / L, other); }

struct ShapePlan {
    size_t N = 0, M = 0, R = 0;  // R = fft_result_size: N (IQ) or N/2 (real), src/spectrumserver.cpp:99-105
    bool is_real = false;
    int log2M1 = 0, log2M2 = 0, M1 = 0, M2 = 0, T1 = 0, T2 = 0;
    int size_log2 = 0, levels = 0, max_batch = 1, n = 0;
    size_t spec_stride = 0, q_len = 0, q_stride = 0, qt_stride = 0, p_stride = 0;
    bool real_fused = false;
    int tile_ch = 16, LT = 0, tiled_lt = -1;
    int min_waterfall_fft = 0, skip_num = 1, log2UB = 0;
    RecMap recmap{};
    SpecLayout lay{};
    SegFacts seg;  // (fused real input only)
    TailFacts tail;
};
// of a config create_check accepts
inline ShapePlan shape_plan(const psdr_config &g, const CreateEnv &env) {
    ShapePlan s;
    s.N = g.fft_size;
    s.is_real = g.is_real != 0;
    s.M = s.R = s.is_real ? s.N / 2 : s.N;
    const int m = ilog2(s.M);
    s.log2M2 = m / 2;
    // 2^22-point real frames (a 2^21-point packed transform): 1024 x 2048 - the first pass is then the 16-column kernel
    // of the 2^20 / 2^21-point shapes (128-byte raw rows and Y rows: 5.3 TB/s against the 8-column 2048-point kernel's
    // 4.1), the second pass walks tiles of FOUR (row, mirror row) couples of 2048-point rows (k_fft_pass2_real<2048, 8, 16>).
    if (s.is_real && m == 21 && !env.real_split_2048x1024) s.log2M2 = 11;
    if (env.log2M2) s.log2M2 = env.log2M2;
    s.log2M1 = m - s.log2M2;
    s.M1 = 1 << s.log2M1, s.M2 = 1 << s.log2M2;
    s.T1 = pick_T(s.M1, s.M2), s.T2 = pick_T(s.M2, s.M1);
    s.size_log2 = (int)std::lround(std::log2((double)s.N)) + g.brightness_offset;
    s.levels = g.downsample_levels;
    s.max_batch = g.max_batch;
    s.n = g.audio_fft_size;
    s.spec_stride = s.is_real ? s.M + 2 : s.N;
    for (int i = 0; i < s.levels; i++) s.q_len += s.R >> i;
    s.q_stride = (s.q_len + 127) & ~(size_t)127;
    s.real_fused = s.is_real && !env.real_3pass &&
                   ((s.M2 == 1024 && s.T2 == 16 && (s.M1 == 1024 || s.M1 == 2048)) || (s.M2 == 2048 && s.T2 == 8 && s.M1 == 1024 && s.T1 == 16));
    if (s.real_fused) {
        const int cp = s.T2 / 2;  // (row, mirror row) couples per tile: 8 (octet records, levels 0..3) or 4 (quartets, levels 0..2)
        s.tile_ch = cp;           // RecMap mode 2
        s.LT = s.tiled_lt = ilog2((size_t)cp);
        s.recmap.l2tpr = ilog2((size_t)(s.M1 / cp));
        s.recmap.l2rows = s.log2M2;
        s.recmap.mapped = 2;
        s.recmap.pair = cp == 4 ? 1 : 0;  // quartets: a column's two records side by side
        s.lay.mode = 2;
        s.lay.l2cp = s.LT;
        s.seg.G = s.M1 / s.T2, s.seg.num_cus = env.num_cus, s.seg.seg_len_env = env.seg_len;
    } else if (s.is_real) {
        s.LT = 8;  // the untangle kernel finishes levels 0..8 (4 bins per lane, 64 lanes)
    } else {
        s.tile_ch = s.T2 >= 16 ? 16 : 8;
        s.LT = s.tiled_lt = s.T2 >= 16 ? 4 : 3;
        s.recmap.l2tpr = ilog2((size_t)(s.M1 / s.tile_ch));
        s.recmap.l2gpt = ilog2((size_t)(s.T2 / s.tile_ch));
        s.recmap.l2rows = s.log2M2;
        s.recmap.mapped = 1;
        if (s.M2 == 1024 && s.T2 == 16) s.lay.mode = 1;  // k_fft_pass2<1024, 16, true, *> writes tile-major lines
    }
    if (s.tiled_lt >= 0) s.qt_stride = 2 * s.R;  // R/CH records of 2*CH bytes
    if (s.lay.mode) s.lay.m1 = s.M1, s.lay.l2m1 = s.log2M1, s.lay.L = s.M2, s.lay.l2L = s.log2M2;
    s.p_stride = std::max<size_t>(s.R >> s.LT, 64);
    s.skip_num = std::max(g.skip_num, 1);
    s.min_waterfall_fft = g.waterfall_size > 0 ? g.waterfall_size : (int)(s.R >> (s.levels - 1));
    if (s.is_real) s.log2UB = std::min(10, ilog2(s.N));
    TailFacts &t = s.tail;
    t.R = s.R, t.levels = s.levels, t.LT = s.LT, t.log2M2 = s.log2M2, t.M2 = s.M2, t.real_fused = s.real_fused;
    t.mapped = s.recmap.mapped, t.l2gpt = s.recmap.l2gpt, t.pair = s.recmap.pair;
    return s;
}

// ---- the audio clients' inverse DFT of n points (demod.h) ------------------------------------------------------------------
// fixed: the compile-time plans 360 = 8*9*5 and 720 = 8*9*10; wave: one wave per item, no work-group barriers; lds: one
// work-group per item (k_demod_idft) with both buffers and the twiddles in LDS while 24 n bytes fit 144 KiB (lds_mode 0), the
// buffers alone while 16 n do (1), else in the per-work-group global scratch (2)
enum IdftKind { IDFT_NONE, IDFT_FIXED360, IDFT_FIXED720, IDFT_WAVE, IDFT_LDS };
struct IdftPlan {
    PlanStatus st;
    int n = 0;
    IdftKind kind = IDFT_NONE;
    int nstages = 0, radix[PSDR_MAX_STAGES] = {};
    int lds_mode = 0, idft_threads = 256;
    size_t idft_lds = 0;
};
inline IdftPlan idft_plan(int n) {
    IdftPlan p;
    p.n = n;
    if (n <= 0) return p;
    // factorise n, grouping prime factors into radices <= 16 (fewer barriers)
    int m = n, cur = 1, ns = 0;
    auto close = [&] {
        if (cur > 1 && ns < PSDR_MAX_STAGES) p.radix[ns] = cur;
        ns += cur > 1;
    };
    auto take = [&](int f) {  // the next prime factor, in ascending order
        if (cur * f > 16) close(), cur = 1;
        cur *= f;
    };
    for (int f = 2; (long long)f * f <= m; f++)
        for (; m % f == 0; m /= f) take(f);
    if (m > 1) take(m);
    close();
    if (ns > PSDR_MAX_STAGES) {
        p.st = plan_fail(PSDR_ERR_UNSUPPORTED, "audio_fft_size %d has too many factors", n);
        return p;
    }
    p.nstages = ns;
    const size_t cap = 144 * 1024;
    p.lds_mode = (size_t)n * 24 <= cap ? 0 : ((size_t)n * 16 <= cap ? 1 : 2);
    p.idft_lds = p.lds_mode == 2 ? 0 : (size_t)n * (p.lds_mode ? 16 : 24);
    p.idft_threads = n <= 512 ? 128 : 256;
    p.kind = n == 360 ? IDFT_FIXED360 : (n == 720 ? IDFT_FIXED720 : (n <= 512 ? IDFT_WAVE : IDFT_LDS));
    return p;
}
// Stage tables of the generic-radix Stockham: output o = s*(n/R) + i of a stage with radix R and p = product of the earlier
// radices reads x[i + q*n/R] and writes y[j + s*p], j = (i - i%p)*R + i%p, with twiddle exponent q*e1,
// e1 = (i%p + s*p)*n/(p*R).  An entry as the kernels read it (an int4; ctx.h ties the size); out[nstages * n]
struct IdftEntry {
    int i, j, e1, pad;
};
inline void idft_stage_table(const IdftPlan &p, IdftEntry *out) {
    const int n = p.n;
    int pp = 1;
    for (int st = 0; st < p.nstages; st++) {
        const int R = p.radix[st], tlen = n / R, step = n / (pp * R);
        for (int o = 0; o < n; o++) {
            const int s = o / tlen, i = o - s * tlen, k = i % pp, j = (i - k) * R + k;
            const long long e1 = ((long long)(k + s * pp) * step) % n;
            out[(size_t)st * n + o] = IdftEntry{i, j + s * pp, (int)e1, 0};
        }
        pp *= R;
    }
}

// ---- the twiddle tables: exp(sign * 2 pi i * (j*mult) / period), j < count ----------------------------------------------------
struct Twiddles {
    size_t count = 0, mult = 1, period = 1;  // count 0: the table does not exist
    int sign = -1;
};
struct TwiddlePlan {
    Twiddles Wl1, Wl2;  // the passes' stage tables; Wl2.count 0: M2 == M1, it shares Wl1
    Twiddles TB;        // inter-pass twiddle W_M^e = W_M1^{e >> log2M2} * W_M^{e & (M2-1)}: the first factor is the pass-1 stage
                        // table, the second has M2 entries
    Twiddles UA, UB;    // real input: the untangle's W_N^{h << log2UB}, W_N^{l}
    Twiddles UG;        // fused real input: W_N^{CP g}, the tile's factor
    Twiddles Wn;        // the audio IDFT's
};
inline TwiddlePlan twiddle_plan(const ShapePlan &s) {
    TwiddlePlan t;
    t.Wl1 = {(size_t)s.M1, 1, (size_t)s.M1, -1};
    if (s.M2 != s.M1) t.Wl2 = {(size_t)s.M2, 1, (size_t)s.M2, -1};
    t.TB = {(size_t)s.M2, 1, s.M, -1};
    if (s.is_real) {
        const size_t UB = (size_t)1 << s.log2UB;
        t.UA = {s.N / UB + 1, UB, s.N, -1};
        t.UB = {UB, 1, s.N, -1};
        if (s.real_fused) t.UG = {(size_t)(s.M1 / s.T2), (size_t)(s.T2 / 2), s.N, -1};
    }
    if (s.n > 0) t.Wn = {(size_t)s.n, 1, (size_t)s.n, +1};
    return t;
}
// a table's values, generated in double (x: cos, y: sin - a float2)
struct Twiddle {
    float x, y;
};
inline std::vector<Twiddle> make_twiddles(const Twiddles &t) {
    std::vector<Twiddle> w(t.count);
    for (size_t j = 0; j < t.count; j++) {
        const double a = (double)t.sign * 2.0 * M_PI * (double)((j * t.mult) % t.period) / (double)t.period;
        w[j] = Twiddle{(float)std::cos(a), (float)std::sin(a)};
    }
    return w;
}

// ---- every allocation of psdr_create: elements (0: the context has no such buffer) and whether they start as zeroes ---------
struct Buf {
    size_t count = 0;
    bool zero = false;
};
struct BufferPlan {
    Buf tickets{TICKET_SLOTS * 8, true};  // (each of the two passes')
    Buf Y, Z;         // Z: the three-pass real path's second array, or one frame of k-order staging for psdr_read_spectrum /
                      // psdr_get_output_buffer where the spectrum is not in natural order, or nothing
    size_t seg_cap = 0;            // fused real input: segments the seam buffers and the flags hold (in hand-off mode any
    Buf seamP, seamC, segflag;     // segment may fall back to a seam); P [segment][M2][couples per tile], C [segment][M2];
                                   // flags, then the two result sets' fallback marks
    Buf spec, q, qt, pscr;         // of each result set (pscr: each of its two)
    Buf stage, h_out, h_q;         // level 1
    size_t slots = 0;              // audio client slots (0: audio_fft_size 0, none of the buffers below)
    Buf ypost, pwr, audio, nan;    // pwr, audio, nan: of each of the two result sets
    Buf real_prev, bb_tail, bb_last, ssb_mark, gscratch;  // gscratch: lds_mode 2 only
    size_t client_ring = 0;        // bytes of a slot of the client parameter ring
    size_t wslots = 0, wf_sent_off = 0, wf_ring = 0;  // waterfall client slots; a ring slot [WfClient x W][int x F]
};
inline BufferPlan buffer_plan(const ShapePlan &s, const psdr_config &g) {
    BufferPlan b;
    const size_t F = (size_t)s.max_batch;
    b.Y = {F * s.M, false};
    b.Z = {s.is_real && !s.real_fused ? F * s.M : (s.lay.mode ? s.M + 2 : 0), false};
    if (s.real_fused) {
        const size_t cap = b.seg_cap = seg_cap(s.seg, s.max_batch);
        b.seamP = {cap * (size_t)s.M2 * (size_t)(s.T2 / 2), false};
        b.seamC = {cap * (size_t)s.M2, false};
        b.segflag = {3 * cap, true};
    }
    b.spec = {F * s.spec_stride, true};
    b.q = {F * s.q_stride, true};
    if (s.tiled_lt >= 0) b.qt = {F * s.qt_stride, true};
    b.pscr = {F * s.p_stride, false};
    b.stage = {s.is_real ? s.N : 2 * s.N, false};
    b.h_out = {s.is_real ? s.N / 2 + 1 : s.N + (size_t)g.additional_size, false};
    b.h_q = {s.q_len, false};
    if (s.n > 0) {
        const size_t S = b.slots = (size_t)std::max(1, g.max_clients), n = (size_t)s.n;
        b.ypost = {S * F * n, false};
        b.pwr = b.nan = {S * F, true};
        b.audio = {S * F * (n / 2), true};
        b.real_prev = b.bb_tail = {2 * S * (n / 2), true};
        b.bb_last = {2 * S, true};
        b.ssb_mark = {S, true};
        if (idft_plan(s.n).lds_mode == 2) b.gscratch = {S * F * 2 * n, false};
        b.client_ring = client_ring_bytes(S);
    }
    b.wslots = (size_t)std::max(1, g.max_waterfall_clients);
    b.wf_sent_off = (b.wslots * sizeof(WfClient) + 63) & ~(size_t)63;
    b.wf_ring = b.wf_sent_off + F * sizeof(int);
    return b;
}

// ---- band regions (psdr_set_band_layout; layout.h: SpecLayout mode 3) -------------------------------------------------------
struct BandPlan {
    PlanStatus st;
    int H = 0, Lb = 0, Lw = 0;  // halo columns per band, a band's own columns, the lines of a tile in a region
    size_t frame_stride = 0;    // bins from frame to frame INSIDE a region
    size_t region = 0;          // bins of one band's region: all frames of a batch
    SpecLayout lay{};           // `lay` as mode 3
};
// lay: the context's layout now (a banded context may be banded again)
inline BandPlan band_plan(const ShapePlan &s, const SpecLayout &lay, int nbands, uint32_t halo_bins, int max_batch) {
    BandPlan b;
    if (s.is_real || lay.mode == 0 || lay.mode == 2 || (s.M1 != 1024 && s.M1 != 2048) || s.M2 != 1024)
        b.st = plan_fail(PSDR_ERR_UNSUPPORTED, "banded spectrum: 2^20- and 2^21-point IQ frames only (use psdr_pack_band)");
    else if (nbands < 1 || nbands > 16 || (nbands & (nbands - 1)))
        b.st = plan_fail(PSDR_ERR_INVALID, "nbands %d: a power of two <= 16", nbands);
    else if (halo_bins > (uint32_t)s.M)
        b.st = plan_fail(PSDR_ERR_INVALID, "halo of %u bins", halo_bins);
    if (b.st.code) return b;
    b.H = (int)((halo_bins + (uint32_t)s.M1 - 1) >> s.log2M1), b.Lb = s.M2 / nbands, b.Lw = b.Lb + b.H;
    // k_band_halo repeats the first H columns of band b+1 behind band b: they must be band b+1's OWN columns (a halo
    // longer than a band would reach into band b+2's, which band b+1's region only holds as its own halo - written
    // by the same launch)
    if (b.H > b.Lb) {
        b.st = plan_fail(PSDR_ERR_INVALID, "halo of %u bins = %d columns of %d bins exceeds a band of %d columns (%d bands)", halo_bins, b.H, s.M1,
                         b.Lb, nbands);
        return b;
    }
    b.frame_stride = (size_t)s.M1 * b.Lw;
    b.region = (size_t)max_batch * b.frame_stride;
    b.lay = lay;
    b.lay.mode = 3;
    b.lay.l2Lb = ilog2((size_t)b.Lb);
    b.lay.Lw = b.Lw;
    b.lay.band_stride = b.region;
    b.lay.c2_0 = 0;
    return b;
}

}  // namespace psdr

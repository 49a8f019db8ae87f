// ctx.h - internal: the context behind the C-ABI (include/psdr.h) and what the translation units of libpsdr_hip.so
// share.  context.hip (lifetime, Level 1, ingest ring, instrumentation), pass1.hip / pass2.hip (the FFT pass
// launchers), forward.hip (the frame loop: passes + pyramid tails, spectrum / pyramid read-back, band layout,
// waterfall), demod.hip (audio clients + demodulation), fetch.hip (the served end: results to host memory), postchain.hip
// (DC blocker / AGC / int16), wire.hip (packets).  What the host decides sits in plain C++17 headers of pure functions, one per
// decision - createplan.h (what psdr_create accepts, the shape, the buffers, the twiddles, the audio IDFT, the band regions),
// forwardplan.h, demodplan.h, fetchplan.h, postplan.h and the per-feature plans.  What a context allocates has one owner each (owned.h); what only some
// contexts need - an optional per-client feature's buffers and tables - sits in one struct per feature that exists whole or
// not at all (psdr_ctx: `iq` .. `agc_prof`; RingTable: a batch's table beside the client parameter ring).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/psdr.h"
#include "agcplan.h"
#include "anbplan.h"
#include "audiofilterplan.h"
#include "blankerplan.h"
#include "butterfly.h"
#include "createplan.h"
#include "cwplan.h"
#include "rttyplan.h"
#include "pskplan.h"
#include "faxplan.h"
#include "demodplan.h"
#include "fetchplan.h"
#include "forwardplan.h"
#include "noiseplan.h"
#include "nrplan.h"
#include "owned.h"
#include "postplan.h"
#include "quantize.h"
#include "scanplan.h"
#include "squelchplan.h"
#include "toneplan.h"
#include "types.h"

// sets psdr_last_error() of the calling thread and returns `code`
int psdr_fail(int code, const char *fmt, ...);
#define fail psdr_fail
#define HIPCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(PSDR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                \
    } while (0)
// ... for calls that return the library's own status (the owners of owned.h)
#define PSDRCHK(expr)         \
    do {                      \
        int rc_ = (expr);     \
        if (rc_) return rc_;  \
    } while (0)

// Run-time knobs of the PRODUCT library (documented in DESIGN.md): PSDR_SEG_LEN (tiles per chain segment of the fused
// real-input pass), PSDR_DEMOD_CHAIN / PSDR_DEMOD_K (one-kernel demodulation and its frames per chain), PSDR_REAL_3PASS
// (the three-pass real path).  Every other A/B switch of the tuning rounds is read only by a -DPSDR_TUNING_BUILD
// library (tools/build_variants.py tuning=PSDR_TUNING_BUILD), never by the one that ships.
inline const char *psdr_tuning_env(const char *name) {
#ifdef PSDR_TUNING_BUILD
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

namespace psdr {

enum KernelId { K_PASS1, K_PASS2, K_UNTANGLE, K_TAIL, K_IDFT, K_OLA, K_WFALL, K_POST, K_SEAM, K_BAND, K_WFHOLD, K_WFCARRY, K_SQUELCH, K_NB_SCAN, K_NB_APPLY, K_AUDIO_FILTER, K_AUDIO_NR, K_AUDIO_NB, K_SCAN_TRACE, K_SCAN_FLOOR, K_SCAN_HOT, K_SCAN_MARK, K_SCAN_EMIT, K_AUDIO_TONE, K_AUDIO_CW, K_AUDIO_RTTY, K_AUDIO_PSK, K_AUDIO_FAX, K_COUNT };
extern const char *kKernelNames[K_COUNT];

struct PendingEvent {
    Event a, b;
    int kid;
};

// Small host->device parameter blocks (client lists) are double-buffered K deep so a new
// batch can be enqueued without waiting for the previous one to drain.
struct ParamRing {
    static constexpr int K = 8;
    HostBuf<unsigned char> h;
    DevBuf<unsigned char> d;
    size_t slot_bytes = 0;
    Event ev[K];
    bool used[K] = {};
    int idx = 0;
    int init(size_t bytes) {
        slot_bytes = (bytes + 255) & ~(size_t)255;
        PSDRCHK(h.alloc(slot_bytes * K));
        PSDRCHK(d.alloc(slot_bytes * K));
        for (Event &e : ev) PSDRCHK(e.create());
        return PSDR_OK;
    }
    // returns the slot to fill (waits only if the ring wrapped onto a still-busy slot); -1: HIP error
    int acquire() {
        idx = (idx + 1) % K;
        if (used[idx] && hipEventSynchronize(ev[idx]) != hipSuccess) return -1;
        return idx;
    }
    // hands the slot acquire() has just returned back, unused
    void unacquire() { idx = (idx + K - 1) % K; }
    void *host(int i) { return h + slot_bytes * i; }
    void *dev(int i) { return d + slot_bytes * i; }
    hipError_t release(int i, hipStream_t s) {
        const hipError_t e = hipEventRecord(ev[i], s);
        used[i] = e == hipSuccess;
        return e;
    }
};
// A batch's table of S entries of T that travels beside a ParamRing: one host and one device image [ParamRing::K][S], image i
// with the discipline of the ring's slot i (filled once the slot is acquired, read by the kernels the slot's event covers).
template <typename T>
struct RingTable {
    HostBuf<T> h;
    DevBuf<T> d;
    size_t S = 0;
    static size_t bytes(size_t entries) { return entries * ParamRing::K * sizeof(T); }  // (of one image)
    int alloc(size_t entries) {
        PSDRCHK(h.alloc(entries * ParamRing::K));
        PSDRCHK(d.alloc(entries * ParamRing::K, true));
        S = entries;
        return PSDR_OK;
    }
    explicit operator bool() const { return (bool)d; }
    T *host(int ring) const { return h + (size_t)ring * S; }
    T *dev(int ring) const { return d + (size_t)ring * S; }
    // the first `count` entries of the slot's host image to its device image
    hipError_t upload(int ring, size_t count, hipStream_t s) const {
        return hipMemcpyAsync(dev(ring), host(ring), count * sizeof(T), hipMemcpyHostToDevice, s);
    }
};

// the client parameter ring's slot: demodplan.h (host-only: it spells sizeof(int4) as a number)
static_assert(sizeof(int4) == NOTCH_ENTRY, "a slot's manual notches are one int4 (DemodArgs::notch_man)");
// the segment table's entry: forwardplan.h (host-only: it spells uint4 as four unsigneds)
static_assert(sizeof(uint4) == sizeof(SegEntry), "a segment table entry is one uint4 (Pass2Args::segtab, SeamArgs::segtab)");

// the audio IDFT's stage table entry and a twiddle: createplan.h (host-only: it spells int4 as four ints, float2 as two floats)
static_assert(sizeof(int4) == sizeof(IdftEntry), "a stage table entry is one int4 (DemodArgs::stage_tab)");
static_assert(sizeof(float2) == sizeof(Twiddle), "a twiddle is one float2");

}  // namespace psdr
using namespace psdr;

// What psdr_create resolves (createplan.h: shape_plan, idft_plan) it copies into the fields below in one place (context.hip:
// adopt); `lay`, `spec_stride`, `nbands` and `band_H` start from the plan and move with psdr_set_band_layout.
struct psdr_ctx {
    psdr_config cfg;
    ShapePlan shape;  // the plan itself, as created (band_plan reads it)
    int device = 0;
    int num_cus = 256;
    size_t N = 0, M = 0, R = 0;
    int M1 = 0, M2 = 0, log2M1 = 0, log2M2 = 0;
    int T1 = 0, T2 = 0;
    bool is_real = false;
    // real input, N/2 = 1024*1024 or 2048*1024 points: pass 2 untangles, normalises, takes the power
    // and builds pyramid levels 0..3 itself (k_fft_pass2_real); smaller real transforms keep the
    // three-pass form (pass 1, pass 2, k_untangle_real)
    bool real_fused = false;
    SpecLayout lay{};                // device layout of the spectrum (natural unless real_fused)
    int nbands = 0, band_H = 0;      // psdr_set_band_layout: band regions (SpecLayout mode 3), halo columns per band
    SegFacts seg_facts;              // what the chain segments are planned from (forwardplan.h); seg_len_env: PSDR_SEG_LEN, read at create
    float *d_seamP = nullptr, *d_seamC = nullptr;  // views: seam_pool[cur_set][0 / 1]
    DevBuf<float> seam_pool[2][2];
    size_t seg_cap = 0;  // segments the seam buffers (seamP, seamC) and the flags hold: seg_cap(seg_facts, max_batch)
    // chain segments of the fused real second pass for a batch of `nframes` frames (forwardplan.h; forward.hip: seg_plan)
    struct SegPlan {
        int nframes = 0;
        unsigned nsegs = 0;
        bool handoff = false;  // all but a frame's top segment get their carried row through memory inside the launch
        DevBuf<uint4> d_tab;
    };
    std::vector<SegPlan> seg_plans;  // one per batch size seen
    DevBuf<unsigned> d_segflag;      // [seg_cap] epoch of the launch that last published the segment's carry-out; behind it
                                     // [2][seg_cap] the fallback marks of the two result sets (fft_pass.h: segmark)
    unsigned seg_epoch = 0;
    int size_log2 = 0;
    int levels = 0;
    size_t spec_stride = 0;  // complex elements per frame
    size_t q_len = 0, q_stride = 0;
    int LT = 0;  // pyramid levels finished inside the fused kernel
    TailPlan tails;  // ... and who finishes the others (forwardplan.h), resolved at create
    size_t p_stride = 0;
    int max_batch = 1;
    int min_waterfall_fft = 0;  // input.waterfall_size (src/spectrumserver.cpp:56)
    std::set<const void *> lds_attr_done;  // kernels whose dynamic-LDS limit was raised on this device
    // Two streams: the FFT passes run on `stream`; everything that only consumes a finished
    // batch (pyramid tail, demodulation, waterfall gather) runs on `side`, so it overlaps
    // the next batch's pass 1 (its work-groups fit next to the persistent FFT work-groups).
    hipStream_t stream = nullptr, side = nullptr;  // views: own_stream / own_side, or the caller's (psdr_set_stream)
    Stream own_stream, own_side;
    DevBuf<cf> d_Y;  // the inter-pass array, max_batch frames of M complex values
    // TileQueue counters: a ring of TICKET_SLOTS launches x 8 counters per pass; half the ring is
    // re-zeroed (in stream order) whenever the other half starts being used
    DevBuf<unsigned> d_tickets[2];
    unsigned ticket_pos[2] = {0, 0};
    bool input_on_main = false;  // level-1 H2D staging was enqueued on the main stream
    Event ev_in;
    Event ev_fft_done, ev_side_done;
    bool side_pending = false;
    // Result buffers (spectrum, pyramid, level powers) exist twice: batch b+1 is produced
    // into the other set while the side stream still consumes batch b, so the FFT stream only
    // ever waits for the consumers of batch b-1.  d_spec/d_q/d_qt/d_pscr are views of the set of
    // the LAST processed batch (forward.hip: select_set).
    // (forward.hip: enqueue_tails - what the tail kernels of the batch just transformed need)
    bool tails_pending = false;
    const struct SegPlan *tails_plan = nullptr;
    int tails_nframes = 0;
    int cur_set = 0;
    bool alt_sets = false;  // alternate the sets also on a caller's stream (a group's root: the peers read batch b's spectrum while b + 1 is transformed)
    DevBuf<cf> spec_pool[2];
    DevBuf<int8_t> q_pool[2], qt_pool[2];
    DevBuf<float> pscr_pool[2][2];
    Event ev_set_done[2];
    bool set_pending[2] = {false, false};

    DevBuf<cf> d_Wl1, own_Wl2, d_TB;
    cf *d_Wl2 = nullptr;  // view: d_Wl1 when M2 == M1, else own_Wl2
    DevBuf<cf> d_UA, d_UB, d_UG;
    cf wdelta = {1.f, 0.f};  // W_N^1
    DevBuf<unsigned long long> d_trace;  // PSDR_TRACE tuning builds: per pass [8][16] phase stamps + [256][8] work-group timeline
    int log2UB = 0;
    DevBuf<cf> d_Z;
    cf *d_spec = nullptr;
    int8_t *d_q = nullptr;   // level-major pyramid (the reference's layout)
    int8_t *d_qt = nullptr;  // tiled records of levels 0..LT (IQ fused epilogue), quantize.h
    size_t qt_stride = 0;
    int tiled_lt = -1, tile_ch = 16;
    RecMap recmap{};  // order of the tiled records and of the level-LT scratch
    std::vector<char> q_untiled;  // per frame: level-major copy of the tiled levels is current
    float *d_pscr[2] = {nullptr, nullptr};

    // level 1
    DevBuf<float> d_stage;
    HostBuf<cf> h_out;
    HostBuf<int8_t> h_q;
    bool loaded = false, executed = false, out_valid = false, q_valid = false;
    int last_nframes = 0;

    // audio clients
    std::mutex mtx;
    std::vector<AudioSlot> aslots;
    int n = 0;  // audio_fft_size
    int nstages = 0;
    int radix[PSDR_MAX_STAGES];
    int lds_mode = 0;
    IdftKind idft_kind = IDFT_NONE;  // which kernels transform (createplan.h): demod.hip switches on it
    bool demod_chain = true;  // PSDR_DEMOD_CHAIN=0: the two-kernel path (k_demod_idft_fixed + k_demod_ola) for n = 360 / 720 too
    int demod_chain_k = 0;    // PSDR_DEMOD_K: frames per chain (0: 8, 4 when there are few clients)
    size_t idft_lds = 0;
    DevBuf<int4> d_stage_tab;
    int idft_threads = 256;
    DevBuf<cf> d_Wn, d_ypost, d_gscratch, d_bb_tail, d_bb_last;
    // post-demodulation chain (postchain.h), allocated by psdr_set_post_chain
    bool post_on = false;
    bool post_ready = false;   // the chain's buffers, events and streams exist (psdr_set_post_chain's one-time set-up went through)
    int opt_pc_streams = 0;    // PSDR_OPT_POST_CHAIN_STREAMS: 0 = creation order (deterministic), 1 = chosen by measurement
    int opt_pc_pcm16 = 0;      // PSDR_OPT_POST_CHAIN_PCM16: the chain's PCM as int16 rows (half the bytes to the host)
    bool pcm_is16 = false;     // ... of the last chain batch (what a fetch / psdr_read_pcm finds in the PCM buffer)
    int opt_pc_agc = 1;        // PSDR_OPT_POST_CHAIN_AGC: 1 = chunk maxima + k_pc_agc where it applies, 0 = the five-kernel form
    PostArgs post{};  // (passed to kernels by value: raw pointers, views of what `pc` owns)
    // The chain is a pipeline across batches (round 5), in the order of a batch's data:
    //   side     index, gather (behind the demodulation)
    //   pc_s[0]  moving averages (sequential), history
    //   pc_s[2]  look-ahead peak, w_t, gain recurrence (sequential), int16 output
    // (pc_s[1] is created and left idle: postchain.hip says why.)  The two sequential kernels (1.5 - 2 ms per 512 frames each, whatever the client count)
    // are what a stream must not share: rounds 3-4 had the moving averages AND the six short kernels of their stage on
    // one stream - longer than the step it hid behind (3.2 ms against 2.6).  What the stages hand on rotates over PC_SETS
    // sets, so a batch's chain may take up to two steps longer than a step.
    static constexpr int PC_SETS = 3;
    Stream pc_s[3];
    // what psdr_set_post_chain's one-time set-up creates: built whole, then moved in
    struct PostChain {
        Event ev[4][PC_SETS];  // [stage][set]: the stage's kernels of the batch that used the set are done
        DevBuf<float> x[PC_SETS], m1[PC_SETS], v1[PC_SETS];
        DevBuf<float> p[PC_SETS], s[PC_SETS], sm[PC_SETS];  // prefix maxima then g_t / w_t / sub-block maxima
        DevBuf<int> fstart[PC_SETS], len[PC_SETS];
        // the AGC in one kernel behind chunk maxima (postchain.h k_pc_cm / k_pc_cscan / k_pc_agc): per set like P / S
        DevBuf<float> cm[PC_SETS], cp[PC_SETS], cs[PC_SETS];
        DevBuf<int> falive[PC_SETS];
        DevBuf<int32_t> pcm_pool[2];  // post.pcm is a view of the last batch's
        DevBuf<int32_t> pcm_dump;     // PostArgs' pointers of the same names
        DevBuf<float> dc_s1, dc_s2, agc_gain;
        DevBuf<int> agc_n0;
    } pc;
    bool post_direct = false;  // the last chain batch's moving averages read d_audio themselves (k_pc_ma2 DIRECT)
    psdr::PcPlan post_plan;    // the chain's form (postplan.h), resolved by postchain.hip pc_replan whenever one of its facts changes
    uint64_t chain_seq = 0;
    bool chain_pending = false;
    // Results of the LAST demodulation batch: d_audio / d_pwr / d_nan point into one of TWO sets that alternate from batch to
    // batch, so that the copies of batch b to the host (psdr_fetch_begin) run beside the demodulation of batch b + 1 instead
    // of holding it up (256 clients: 96 MB per step, 1.7 ms on the link - longer than the demodulation it follows)
    float *d_pwr = nullptr, *d_audio = nullptr;  // views: pwr_pool / audio_pool / nan_pool [out_set]
    int *d_nan = nullptr;
    DevBuf<float> d_real_prev;
    DevBuf<float> audio_pool[2], pwr_pool[2];
    DevBuf<int> nan_pool[2];
    int out_set = 0, pcm_set = 0;
    // Optional per-client features.  Each struct below owns everything its feature allocates, and the context has it from the
    // first client that uses the feature (demod.hip: first_use, under mtx): built whole from the context's sizes and then moved
    // in - all of it or none - and kept.  A context that never sees such a client allocates nothing.  alloc(): non-zero if an
    // allocation failed (psdr_last_error() says why); bytes(): the size the failure message names.
    // PSDR_IQ clients' rows [slot][max_batch][n/2] complex64: two pools that alternate with out_set like audio_pool
    struct IqRows {
        DevBuf<cf> pool[2];
        static size_t bytes(const psdr_ctx &c) { return c.aslots.size() * (size_t)c.max_batch * ((size_t)c.n / 2) * sizeof(cf); }  // (of one pool)
        int alloc(const psdr_ctx &c) { return pool[0].alloc(bytes(c) / sizeof(cf)) || pool[1].alloc(bytes(c) / sizeof(cf)); }
        explicit operator bool() const { return (bool)pool[1]; }
    } iq;
    cf *d_iq = nullptr;  // view: the last batch's pool (null until the context's first IQ client)
    // PSDR_SAM clients (demod.h): the carrier tail [2][slots][n/2] beside bb_tail, and the carrier records [slot][max_batch]
    // (level, offset_hz) in two pools that alternate with out_set
    struct Sam {
        DevBuf<cf> car_tail, pool[2];
        static size_t bytes(const psdr_ctx &c) { return 2 * c.aslots.size() * ((size_t)c.n / 2 + (size_t)c.max_batch) * sizeof(cf); }
        int alloc(const psdr_ctx &c) {
            const size_t S = c.aslots.size(), recs = S * (size_t)c.max_batch;
            return car_tail.alloc(2 * S * ((size_t)c.n / 2), true) || pool[0].alloc(recs, true) || pool[1].alloc(recs, true);
        }
        explicit operator bool() const { return (bool)pool[1]; }
    } sam;
    cf *d_car = nullptr;  // view: the last batch's records (null until the context's first SAM client)
    // a family's own tail [2][slots][n/2] - ft: tuned USB / LSB clients (demod.h); sb: sideband SAM clients, the tail of their
    // clipped baseband
    struct Tails {
        DevBuf<cf> tail;
        static size_t bytes(const psdr_ctx &c) { return 2 * c.aslots.size() * ((size_t)c.n / 2) * sizeof(cf); }
        int alloc(const psdr_ctx &c) { return tail.alloc(bytes(c) / sizeof(cf), true); }
        explicit operator bool() const { return (bool)tail; }
    } ft, sb;
    int opt_fine_tune = 0;  // PSDR_OPT_FINE_TUNE: the flag psdr_client_add hands a new client
    int opt_sam_sideband = PSDR_SAM_BOTH;  // PSDR_OPT_SAM_SIDEBAND: the value psdr_client_add hands a new client
    // auto-notch (demod.h: k_notch_detect): per slot the power sums acc [slots][n], the frame counter and the table of the two
    // automatic entries (DemodArgs::notch_auto).  Manual notches travel in the client ring and need no allocation.
    struct Notch {
        DevBuf<float> acc;
        DevBuf<int> cnt;
        DevBuf<int4> tab;
        static size_t bytes(const psdr_ctx &c) { return c.aslots.size() * ((size_t)c.n * sizeof(float) + sizeof(int) + sizeof(int4)); }
        int alloc(const psdr_ctx &c) {
            const size_t S = c.aslots.size();
            return acc.alloc(S * (size_t)c.n, true) || cnt.alloc(S, true) || tab.alloc(S, true);
        }
        explicit operator bool() const { return (bool)tab; }
    } notch;
    int opt_auto_notch = 0;  // PSDR_OPT_AUTO_NOTCH: the value psdr_client_add hands a new client
    const void *dbg_notch_man = nullptr, *dbg_notch_auto = nullptr;  // DemodArgs::notch_man / notch_auto of the last batch (psdr_debug_notch_ptrs)
    // squelch (squelch.h: k_squelch): the frames' open flags [slots][max_batch] in two sets that alternate with out_set like
    // nan_pool, the post chain's drop flags [slots][max_batch] (written and read on `side` within one batch: one set), the
    // gates' state [slots] and the batch's table (squelchplan.h) - a RingTable beside client_ring: the manual notches' way is
    // closed, the client ring's layout is pinned.
    struct Squelch {
        DevBuf<int> pool[2], drop;
        DevBuf<SquelchState> state;
        RingTable<SquelchEntry> tab;
        static size_t bytes(const psdr_ctx &c) {
            const size_t S = c.aslots.size();
            return 3 * S * (size_t)c.max_batch * sizeof(int) + S * sizeof(SquelchState) + RingTable<SquelchEntry>::bytes(S);
        }
        int alloc(const psdr_ctx &c) {
            const size_t S = c.aslots.size(), rows = S * (size_t)c.max_batch;
            return pool[0].alloc(rows, true) || pool[1].alloc(rows, true) || drop.alloc(rows, true) || state.alloc(S, true) || tab.alloc(S);
        }
        explicit operator bool() const { return (bool)tab; }
    } squelch;
    int *d_sq = nullptr;  // view: the last batch's open flags (null until the context's first squelch client)
    // noise floor (noise.h: k_noise_floor): per slot the power sums acc [slots][n] and the ring's record, the frames' noise power
    // W [slots][max_batch] in two sets that alternate with out_set like the squelch flags, and the batch's table (noiseplan.h),
    // a RingTable beside client_ring
    struct NoiseFloor {
        DevBuf<float> acc, pool[2];
        DevBuf<NoiseState> state;
        RingTable<NoiseEntry> tab;
        static size_t bytes(const psdr_ctx &c) {
            const size_t S = c.aslots.size();
            return S * (((size_t)c.n + 2 * (size_t)c.max_batch) * sizeof(float) + sizeof(NoiseState)) + RingTable<NoiseEntry>::bytes(S);
        }
        int alloc(const psdr_ctx &c) {
            const size_t S = c.aslots.size(), rows = S * (size_t)c.max_batch;
            return acc.alloc(S * (size_t)c.n, true) || state.alloc(S, true) || pool[0].alloc(rows, true) || pool[1].alloc(rows, true) || tab.alloc(S);
        }
        explicit operator bool() const { return (bool)tab; }
    } noise;
    float *d_nf = nullptr;  // view: the last batch's W rows (null until the context's first noise-floor client)
    // audio filter (audiofilter.h: k_audio_filter): the sections' carried state [slots][2 sections][2] and the batch's table
    // (audiofilterplan.h), a RingTable beside client_ring
    struct AudioFilter {
        DevBuf<float> state;
        RingTable<AfEntry> tab;
        static size_t bytes(const psdr_ctx &c) {
            return c.aslots.size() * 2 * PSDR_AUDIO_FILTER_SECTIONS * sizeof(float) + RingTable<AfEntry>::bytes(c.aslots.size());
        }
        int alloc(const psdr_ctx &c) { return state.alloc(c.aslots.size() * 2 * PSDR_AUDIO_FILTER_SECTIONS, true) || tab.alloc(c.aslots.size()); }
        explicit operator bool() const { return (bool)tab; }
    } af;
    // noise reduction (nr.h: k_audio_nr): the clients' carried state [slots], the window and twiddle tables and the batch's table
    // (nrplan.h), a RingTable beside client_ring
    struct NoiseReduction {
        DevBuf<NrState> state;
        DevBuf<NrTables> plan;
        RingTable<NrEntry> tab;
        static size_t bytes(const psdr_ctx &c) { return c.aslots.size() * sizeof(NrState) + sizeof(NrTables) + RingTable<NrEntry>::bytes(c.aslots.size()); }
        int alloc(const psdr_ctx &c) {
            if (state.alloc(c.aslots.size(), true) || plan.alloc(1) || tab.alloc(c.aslots.size())) return 1;
            NrTables t;
            nr_tables(t);
            const hipError_t e = hipMemcpy(plan.get(), &t, sizeof(t), hipMemcpyHostToDevice);
            return e == hipSuccess ? 0 : psdr_fail(PSDR_ERR_HIP, "noise reduction tables: %s", hipGetErrorString(e));
        }
        explicit operator bool() const { return (bool)tab; }
    } nr;
    int opt_nr = 0;  // PSDR_OPT_NOISE_REDUCTION: the preset (0: none) a client gets at psdr_client_add
    // audio blanker (anb.h: k_audio_nb): the clients' carried state [slots] and the batch's table (anbplan.h), a RingTable beside
    // client_ring
    struct AudioBlanker {
        DevBuf<AnbState> state;
        RingTable<AnbEntry> tab;
        static size_t bytes(const psdr_ctx &c) { return c.aslots.size() * sizeof(AnbState) + RingTable<AnbEntry>::bytes(c.aslots.size()); }
        int alloc(const psdr_ctx &c) { return state.alloc(c.aslots.size(), true) || tab.alloc(c.aslots.size()); }
        explicit operator bool() const { return (bool)tab; }
    } anb;
    int opt_anb = 0;  // PSDR_OPT_AUDIO_BLANKER: the preset (0: none) a client gets at psdr_client_add
    // tone decoder (tone.h: k_audio_tone): the clients' carried state [slots] and history ring [slots][ring][64], the plan's
    // tables for the context's audio_rate, the frames' records [slots][max_batch] and the chain's drop flags [slots][max_batch]
    // (both written and read on `side` within one batch or behind a drain: one set), and the batch's table (toneplan.h), a
    // RingTable beside client_ring
    struct ToneDecoder {
        DevBuf<ToneState> state;
        DevBuf<ToneC> hist;
        DevBuf<ToneTables> plan;
        DevBuf<ToneRec> rec;
        DevBuf<int> drop;
        RingTable<ToneEntry> tab;
        int ring = 0;  // rows of a slot's history ring
        static size_t ring_rows(const psdr_ctx &c) { return (size_t)tone_ring(tone_nb((double)c.cfg.audio_rate)); }
        static size_t bytes(const psdr_ctx &c) {
            const size_t S = c.aslots.size();
            return S * (sizeof(ToneState) + ring_rows(c) * TONE_LANES * sizeof(ToneC) + (size_t)c.max_batch * (sizeof(ToneRec) + sizeof(int))) + sizeof(ToneTables) +
                   RingTable<ToneEntry>::bytes(S);
        }
        int alloc(const psdr_ctx &c) {
            const size_t S = c.aslots.size(), rows = S * (size_t)c.max_batch;
            ring = (int)ring_rows(c);
            if (state.alloc(S, true) || hist.alloc(S * (size_t)ring * TONE_LANES, true) || plan.alloc(1) || rec.alloc(rows, true) || drop.alloc(rows, true) || tab.alloc(S))
                return 1;
            std::vector<ToneTables> t(1);
            tone_tables(t[0], (double)c.cfg.audio_rate);
            const hipError_t e = hipMemcpy(plan.get(), t.data(), sizeof(ToneTables), hipMemcpyHostToDevice);
            return e == hipSuccess ? 0 : psdr_fail(PSDR_ERR_HIP, "tone decoder tables: %s", hipGetErrorString(e));
        }
        explicit operator bool() const { return (bool)tab; }
    } tone;
    // CW decoder (cw.h: k_audio_cw): the clients' carried state [slots] and text ring [slots][1024], the plan's tables for the
    // context's audio_rate, the frames' records [slots][max_batch] (written and read on `side` within one batch or behind a
    // drain: one set), and the batch's table (cwplan.h), a RingTable beside client_ring
    struct CwDecoder {
        DevBuf<CwState> state;
        DevBuf<uint8_t> text;
        DevBuf<CwTables> plan;
        DevBuf<CwRec> rec;
        RingTable<CwEntry> tab;
        static size_t bytes(const psdr_ctx &c) {
            const size_t S = c.aslots.size();
            return S * (sizeof(CwState) + CW_TEXT + (size_t)c.max_batch * sizeof(CwRec)) + sizeof(CwTables) + RingTable<CwEntry>::bytes(S);
        }
        int alloc(const psdr_ctx &c) {
            const size_t S = c.aslots.size();
            if (state.alloc(S, true) || text.alloc(S * CW_TEXT, true) || plan.alloc(1) || rec.alloc(S * (size_t)c.max_batch, true) || tab.alloc(S)) return 1;
            std::vector<CwTables> t(1);
            cw_tables(t[0], (double)c.cfg.audio_rate);
            const hipError_t e = hipMemcpy(plan.get(), t.data(), sizeof(CwTables), hipMemcpyHostToDevice);
            return e == hipSuccess ? 0 : psdr_fail(PSDR_ERR_HIP, "CW decoder tables: %s", hipGetErrorString(e));
        }
        explicit operator bool() const { return (bool)tab; }
    } cw;
    // RTTY decoder (rtty.h: k_audio_rtty): the clients' carried state [slots] and text ring [slots][1024], the seed and code
    // tables for the context's audio_rate, the frames' records [slots][max_batch] (written and read on `side` within one batch or
    // behind a drain: one set), and the batch's table (rttyplan.h), a RingTable beside client_ring
    struct RttyDecoder {
        DevBuf<RttyState> state;
        DevBuf<uint8_t> text;
        DevBuf<RttyTables> plan;
        DevBuf<RttyRec> rec;
        RingTable<RttyEntry> tab;
        static size_t bytes(const psdr_ctx &c) {
            const size_t S = c.aslots.size();
            return S * (sizeof(RttyState) + RTTY_TEXT + (size_t)c.max_batch * sizeof(RttyRec)) + sizeof(RttyTables) + RingTable<RttyEntry>::bytes(S);
        }
        int alloc(const psdr_ctx &c) {
            const size_t S = c.aslots.size();
            if (state.alloc(S, true) || text.alloc(S * RTTY_TEXT, true) || plan.alloc(1) || rec.alloc(S * (size_t)c.max_batch, true) || tab.alloc(S)) return 1;
            std::vector<RttyTables> t(1);
            rtty_tables(t[0], (double)c.cfg.audio_rate);
            const hipError_t e = hipMemcpy(plan.get(), t.data(), sizeof(RttyTables), hipMemcpyHostToDevice);
            return e == hipSuccess ? 0 : psdr_fail(PSDR_ERR_HIP, "RTTY decoder tables: %s", hipGetErrorString(e));
        }
        explicit operator bool() const { return (bool)tab; }
    } rtty;
    // PSK31 decoder (psk.h: k_audio_psk): the clients' carried state [slots] and text ring [slots][1024], the seed tables and the
    // varicode by code for the context's audio_rate, the frames' records [slots][max_batch] (written and read on `side` within one
    // batch or behind a drain: one set), and the batch's table (pskplan.h), a RingTable beside client_ring
    struct PskDecoder {
        DevBuf<PskState> state;
        DevBuf<uint8_t> text;
        DevBuf<PskTables> plan;
        DevBuf<PskRec> rec;
        RingTable<PskEntry> tab;
        static size_t bytes(const psdr_ctx &c) {
            const size_t S = c.aslots.size();
            return S * (sizeof(PskState) + PSK_TEXT + (size_t)c.max_batch * sizeof(PskRec)) + sizeof(PskTables) + RingTable<PskEntry>::bytes(S);
        }
        int alloc(const psdr_ctx &c) {
            const size_t S = c.aslots.size();
            if (state.alloc(S, true) || text.alloc(S * PSK_TEXT, true) || plan.alloc(1) || rec.alloc(S * (size_t)c.max_batch, true) || tab.alloc(S)) return 1;
            std::vector<PskTables> t(1);
            psk_tables(t[0], (double)c.cfg.audio_rate);
            const hipError_t e = hipMemcpy(plan.get(), t.data(), sizeof(PskTables), hipMemcpyHostToDevice);
            return e == hipSuccess ? 0 : psdr_fail(PSDR_ERR_HIP, "PSK decoder tables: %s", hipGetErrorString(e));
        }
        explicit operator bool() const { return (bool)tab; }
    } psk;
    // Radiofax decoder (fax.h: k_audio_fax): the clients' carried state [slots], the line rings [slots][rmax][2048] and their meta
    // [slots][rmax] - rmax the lines the context's largest batch can complete at 240 lines per minute, 64 at least -, the seed
    // tables for the context's audio_rate, the frames' records [slots][max_batch] (written and read on `side` within one batch or
    // behind a drain: one set), and the batch's table (faxplan.h), a RingTable beside client_ring
    struct FaxDecoder {
        DevBuf<FaxState> state;
        DevBuf<uint8_t> ring;
        DevBuf<uint32_t> meta;
        DevBuf<FaxTables> plan;
        DevBuf<FaxRec> rec;
        RingTable<FaxEntry> tab;
        int rmax = 0;
        static uint64_t max_samples(const psdr_ctx &c) { return (uint64_t)c.max_batch * (uint64_t)(c.n / 2); }
        static size_t bytes(const psdr_ctx &c) {
            const size_t S = c.aslots.size(), R = (size_t)fax_ring_max((double)c.cfg.audio_rate, max_samples(c));
            return S * (sizeof(FaxState) + R * (FAX_WIDTH_MAX + sizeof(uint32_t)) + (size_t)c.max_batch * sizeof(FaxRec)) + sizeof(FaxTables) + RingTable<FaxEntry>::bytes(S);
        }
        int alloc(const psdr_ctx &c) {
            const size_t S = c.aslots.size();
            rmax = fax_ring_max((double)c.cfg.audio_rate, max_samples(c));
            if (state.alloc(S, true) || ring.alloc(S * (size_t)rmax * FAX_WIDTH_MAX, true) || meta.alloc(S * (size_t)rmax, true) || plan.alloc(1) ||
                rec.alloc(S * (size_t)c.max_batch, true) || tab.alloc(S))
                return 1;
            std::vector<FaxTables> t(1);
            fax_tables(t[0], (double)c.cfg.audio_rate);
            const hipError_t e = hipMemcpy(plan.get(), t.data(), sizeof(FaxTables), hipMemcpyHostToDevice);
            return e == hipSuccess ? 0 : psdr_fail(PSDR_ERR_HIP, "fax decoder tables: %s", hipGetErrorString(e));
        }
        explicit operator bool() const { return (bool)tab; }
    } fax;
    // AGC profiles (agcplan.h; postchain.h: k_pc_want_prof and the PcWithProfiles kernels): the batch's table, a RingTable beside
    // client_ring.  The chain's carried state is the context's own: a profile adds none
    struct AgcProfiles {
        RingTable<AgcEntry> tab;
        static size_t bytes(const psdr_ctx &c) { return RingTable<AgcEntry>::bytes(c.aslots.size()); }
        int alloc(const psdr_ctx &c) { return tab.alloc(c.aslots.size()); }
        explicit operator bool() const { return (bool)tab; }
    } agc_prof;
    DevBuf<unsigned> d_ssb_mark;  // [slots] DemodArgs::ssb_mark (demod.h): USB / LSB batches that need the frame-ordered NaN guard
    ParamRing client_ring;
    int last_demod_frames = 0;
    uint64_t demod_seq = 0;  // number of demodulation batches so far (AudioSlot::last_seq)
    // psdr_fetch_begin / _end / psdr_fetch_batch: the served end of the path (src/signal.cpp:283-291, src/audio.cpp:26-44,
    // src/waterfall.cpp:44-51 hand HOST buffers to the encoders).  A ring of pinned host sets, [slot][frame][...] each; a fetch is
    // enqueued on `fetch_stream` behind the kernels that produce the batch's results and runs beside the next batch's passes;
    // the device buffers it reads exist once, so the next batch's WRITERS (demodulation, waterfall gather, the chain's
    // output kernel) wait for `done` of the newest fetch in stream order (fetch_guard).  fetch.hip; what a fetch copies and the
    // ring's arithmetic: fetchplan.h.
    struct FetchSet {
        HostBuf<float> audio, pwr;
        HostBuf<int32_t> nan, pcm;
        HostBuf<int8_t> wf;
        size_t wf_cap = 0;
        // rows that only some slots have: [slot - at.lo][max_batch][...] of the at.n slots from the lowest to the highest that
        // have them (fetchplan.h span_of), in a buffer that holds `cap` slots and only grows
        template <typename T>
        struct Span {
            HostBuf<T> buf;
            size_t cap = 0;
            FetchSpan at;
        };
        Span<cf> iq;          // PSDR_FETCH_IQ: the IQ rows [..][n/2] of the slots that were IQ
        size_t iq_bytes = 0;  // ... and the bytes the fetch's IQ copy moved
        Span<cf> car;         // the carrier records of the slots that were SAM
        Span<int32_t> sq;     // the squelch flags of the slots that ran with squelch
        Span<float> nf;       // the noise power rows of the slots that ran with the noise floor (noiseplan.h: noise_fetch_span)
        std::vector<char> nf_on;  // ... per audio slot: the batch ran with it (psdr_fetched_noise: 0 for every frame otherwise)
        Event done;                      // every copy of the fetch on the first copy stream has landed
        Event ev_pcm;                    // ... and the PCM (its own copy stream: it waits for the post chain, up to two steps late)
        bool has_pcm = false;
        bool pcm16 = false;              // its PCM rows are int16 (PSDR_OPT_POST_CHAIN_PCM16 at that batch)
        Event ev_wf;                     // ... the waterfall rows (first in the copy stream: d_wfout exists once)
        Event ev_audio;                  // ... pwr, NaN flags, float audio and the spans' rows (what the demodulation of batch b + 2 overwrites)
        bool inflight = false;
        unsigned what = 0;     // PSDR_FETCH_* bits the copies covered
        int frames = 0;        // frames of the demodulation batch (0: none was fetched)
        uint64_t seq = 0;      // its demod_seq
        std::vector<FetchWin> win;     // per audio slot: the window the batch was demodulated with
        std::vector<FetchSlot> slots;  // ... and what psdr_fetch_begin planned the copies from (kept for its capacity)
        std::vector<WfSlot> wfm;       // per waterfall slot: what psdr_waterfall_batch gathered (out_off, nsent, b_*)
    } fset[PSDR_FETCH_SETS];
    uint64_t slot_births = 0;      // psdr_client_add calls so far (AudioSlot::born)
    int fetch_fill = 0;            // the set the next psdr_fetch_begin fills (a ring: the oldest in flight is fetch_fill - fetch_inflight)
    int fetch_inflight = 0;        // fetches begun and not yet ended
    int fetch_cur = -1;            // the set psdr_fetched_* read: completed by the last psdr_fetch_end
    Stream fetch_stream, fetch_stream_pcm;
    Event ev_fetch_src;
    // what the next WRITER of a device-side result buffer waits for (stream-ordered): the newest fetch that read it
    // (views of a FetchSet's events)
    hipEvent_t guard_wf = nullptr, guard_audio[2] = {nullptr, nullptr}, guard_pcm[2] = {nullptr, nullptr};

    // waterfall clients
    std::vector<WfSlot> wslots;
    ParamRing wf_ring;  // [WfClient x W][int x F]
    size_t wf_sent_off = 0;
    DevBuf<int8_t> d_wfout;
    size_t wfout_cap = 0;
    // waterfall detectors (psdr_waterfall_set_detector): the carry is the reduction of the frames of the current RUN of
    // psdr_waterfall_batch calls that lie behind the run's last sent frame - what the next sent row's window holds of
    // earlier batches.  Allocated by the first batch with a non-sample client; touched on `side` only.
    int opt_wf_det = PSDR_WF_SAMPLE;   // PSDR_OPT_WATERFALL_DETECTOR: what psdr_waterfall_add hands a new client
    DevBuf<int8_t> d_wf_peak;
    DevBuf<uint32_t> d_wf_sum;
    WfCarryLayout wf_lay;              // which bytes of a frame's record buffers the carry mirrors (forwardplan.h)
    WfCarry wf_carry;                  // the run the carry belongs to
    // band scan (scan.h; psdr_scan_set): the trace [R] of 1/256 counts, the hot bins' mask and the start words [R / 64], the
    // segments' quartiles and floors [R / 256], the list with its head, and the scratch of the run index (the starts in front of
    // every mask word) - sized for level 0, allocated by the first psdr_scan_set that switches the scan on, all or none, and
    // kept.  Touched on `side` only.  scan_on / scan_cfg: under mtx; scan_st: the run of frames the trace belongs to (scanplan.h)
    struct BandScan {
        DevBuf<uint16_t> trace;
        DevBuf<uint64_t> hot, starts;
        DevBuf<uint32_t> Q, F, base;
        DevBuf<ScanRun> list;
        DevBuf<ScanHead> head;
        static size_t bytes(const psdr_ctx &c) { return scan_bytes(c.R); }
        int alloc(const psdr_ctx &c) {
            const size_t R = c.R;
            return trace.alloc(R, true) || hot.alloc(R / 64, true) || starts.alloc(R / 64, true) || Q.alloc(R / SCAN_SEG, true) ||
                   F.alloc(R / SCAN_SEG, true) || base.alloc(R / 64, true) || list.alloc(SCAN_CAP, true) || head.alloc(1, true);
        }
        explicit operator bool() const { return (bool)head; }
    } scan;
    bool scan_on = false;
    psdr_scan_config scan_cfg{};
    ScanState scan_st;

    // streaming ingest ring (psdr_ring_*)
    struct IngestRing {
        static constexpr int NEV = 16;
        DevBuf<unsigned char> d;     // nhalves + 1 slots (the last mirrors slot 0: a frame window may end there)
        int nhalves = 0;
        size_t hb = 0;
        Stream copy;
        std::vector<Event> ev_written;        // per slot: its last H2D copy
        std::vector<char> ever_written;
        std::vector<uint64_t> reader_seq;     // per slot: the last psdr_process_ring call that read it
        Event ev_read[NEV];                   // pass 1 of process call seq % NEV has consumed its halves
        uint64_t seq = 0;
    } ring;
    // impulse blanker on the ring (blanker.h, in front of pass 1): the block maxima [max_batch + 1][N/2/256], the ring of
    // reference levels [max_batch + 2] (blankerplan.h: NbState::rpos), the blocks' masks [..][8], the work list and the counts
    // [max_batch + 1] with the list's length behind them - all of it allocated by the first psdr_ring_set_blanker(on = 1), or
    // none, and kept.  Frame-loop thread only, like the ring.
    struct Blanker {
        bool on = false;
        float kf = 1.f;
        int guard = 0;
        NbState st;
        int rcap = 0;
        DevBuf<float> d_bmax, d_R;
        DevBuf<unsigned> d_mask, d_list, d_count;
        uint64_t last_first = 0;  // the halves the LAST psdr_process_ring blanked (psdr_ring_read_blanker), and where their R sits
        int last_n = 0, last_r0 = 0;
    } nb;

    // instrumentation
    bool profiling = false;   // psdr_set_profiling mode 1: hipEvent brackets around every launch
    bool kclock = false;      // mode 2: device-clock stamps inside the two FFT passes (fft_pass.h kclk_*)
    static constexpr unsigned KCLK_SLOTS = 8192;  // launches per pass that can be stamped between two resets
    DevBuf<unsigned long long> d_kclk;            // [2 passes][KCLK_SLOTS][begin, end]
    unsigned kclk_pos[2] = {0, 0}, kclk_done[2] = {0, 0};
    double wall_clock_khz = 100000.0;
    std::vector<PendingEvent> pending;
    std::vector<Event> pool;
    double k_ms[K_COUNT] = {0};
    int64_t k_n[K_COUNT] = {0};
    std::vector<float> k_samples[K_COUNT];  // per-launch durations in us since the last reset (bounded)
    Event t0, t1;
};

namespace psdr {

struct ProfScope {
    psdr_ctx *c;
    int kid;
    Event a, b;
    hipStream_t st;
    ProfScope(psdr_ctx *c_, int kid_, hipStream_t st_ = nullptr) : c(c_), kid(kid_), st(st_ ? st_ : c_->stream) {
        if (!c->profiling) return;
        auto get = [&](Event &e) {
            if (!c->pool.empty()) {
                e = std::move(c->pool.back());
                c->pool.pop_back();
            } else {
                (void)e.create_timing();
            }
        };
        get(a);
        get(b);
        if (!a || !b || hipEventRecord(a, st) != hipSuccess) give_back();  // no timing for this launch
    }
    ~ProfScope() {
        if (!c->profiling || !a) return;
        if (hipEventRecord(b, st) == hipSuccess)
            c->pending.push_back({std::move(a), std::move(b), kid});
        else
            give_back();
    }
    void give_back() {
        if (a) c->pool.push_back(std::move(a));
        if (b) c->pool.push_back(std::move(b));
    }
};

// persistent launch: as many work-groups as the CUs hold (LDS-limited), a multiple of 8 (XCD
// round-robin of the TileQueue), or one per tile when there are fewer tiles than that
inline unsigned persistent_grid(psdr_ctx *c, unsigned blocks, size_t lds) {
    unsigned cap = ((unsigned)c->num_cus * (unsigned)std::max<size_t>(1, 160 * 1024 / lds)) & ~7u;
    // post chain on: one to three CUs per XCD stay free of the passes' work-groups - the home of the chain's recurrence waves
    // (postchain.hip: they allocate a whole SIMD's registers each, or ask for more LDS than a pass leaves, so they land
    // THERE and nowhere else; beside a pass's eight waves and the other consumers a recurrence runs 1.9 - 2.8 ms per 512
    // frames, longer than the step).  0.5 % of the plain step per CU and XCD.
    unsigned reserve = c->post_on ? (unsigned)c->post_plan.reserve : 0u;
    if (const char *e = psdr_tuning_env("PSDR_GRID_RESERVE")) reserve = (unsigned)atoi(e) & ~7u;  // (tuning build)
    if (lds * 2 > 160 * 1024 && cap >= reserve + 8u) cap -= reserve;
    return blocks <= cap ? blocks : std::max(cap, 8u);
}

// context.hip
int drain(psdr_ctx *c);
// what was just enqueued on `side` reads the current result set: the next drain and the set's next writer wait for it
int side_done(psdr_ctx *c);
// postchain.hip: resolves post_plan again (after a drain: psdr_set_post_chain, the chain's options, psdr_set_stream)
void pc_replan(psdr_ctx *c);
// demod.hip: PSDR_ERR_INVALID unless `id` is an audio slot with a client (under mtx)
int check_slot(psdr_ctx *c, int id);
// fetch.hip: the next writer of a device-side result buffer on stream `st` waits for the fetch that read it (ev may be null)
int fetch_guard_wait(psdr_ctx *c, hipStream_t st, hipEvent_t ev);
void resolve_pending(psdr_ctx *c);
void resolve_kclock(psdr_ctx *c);
int reset_kclock(psdr_ctx *c);
// forward.hip
void select_set(psdr_ctx *c, int set);
int seg_plan(psdr_ctx *c, int nframes, const psdr_ctx::SegPlan **out);  // (built and uploaded on first use of a batch size)
int process_frames(psdr_ctx *c, const void *d_halves, int nframes, int fmt, hipEvent_t ev_raw_consumed = nullptr);
int set_wf_default_detector(psdr_ctx *c, int detector);  // PSDR_OPT_WATERFALL_DETECTOR
// blanker.hip: the blanker's kernels for the halves this psdr_process_ring call reads first, on c->stream
int blanker_enqueue(psdr_ctx *c, uint64_t first_half, int nframes);
// pass1.hip / pass2.hip (Pass1Args / Pass2Args: fft_pass.h)
struct Pass1Args;
struct Pass2Args;
int launch_pass1(psdr_ctx *c, int L, int T, int sb, const Pass1Args &a, unsigned blocks, bool pair);
int launch_pass2(psdr_ctx *c, int L, int T, bool fused, const Pass2Args &a, unsigned blocks);
int launch_pass2_band(psdr_ctx *c, const Pass2Args &a, unsigned blocks);
int launch_pass2_real(psdr_ctx *c, const Pass2Args &a);
// postchain.hip: the chain's kernels for the batch demod_impl has just enqueued; *last_user = the last stream that reads
// the client parameter block; d_drop: the flags [slots][max_batch] of the frames that stay out of the clients' streams - the
// batch's NaN flags themselves, or (a batch with squelch clients) k_squelch's merged drop flags; d_agc: the batch's table of AGC
// profiles [slots], uploaded on `side`, or null (no client of the batch has one)
int post_chain_enqueue(psdr_ctx *c, const ClientParams *d_clients, const int *d_slot_ci, int nact, int npaused, int nframes,
                       const int *d_drop, const AgcEntry *d_agc, hipStream_t *last_user);

}  // namespace psdr

// scan.hip - the band scan: the kernels behind scan.h and the calls of include/psdr.h (psdr_scan_set, psdr_scan_batch and the
// three read calls).  Five launches per psdr_scan_batch on the side stream: k_scan_trace folds the batch's frames into the trace,
// k_scan_floor selects every segment's quartile, k_scan_hot writes the floors and the hot bins' mask, k_scan_mark (one work-group)
// finds the start words, numbers the runs and clears the list, k_scan_emit writes every run's first, end and peak key.
#include "ctx.h"
#include "scan.h"

namespace psdr {

// ---- k_scan_trace -----------------------------------------------------------------------------------------------------------
// NW dwords as one load or store (NW = 8: two 16-byte pieces)
template <int NW>
struct ScanWords {
    typedef uint32_t type __attribute__((ext_vector_type(NW)));
};
// PER int8 values -> u = q + 128 each: the sign bit flipped, as the waterfall detectors take them
template <int PER>
__device__ __forceinline__ void scan_load_u(const int8_t *p, uint32_t (&u)[PER]) {
    if constexpr (PER >= 8) {
        const typename ScanWords<PER / 4>::type v = *reinterpret_cast<const typename ScanWords<PER / 4>::type *>(p);
#pragma unroll
        for (int k = 0; k < PER; k++) u[k] = ((v[k / 4] >> (8 * (k % 4))) & 0xFFu) ^ 0x80u;
    } else if constexpr (PER == 4) {
        const uint32_t v = *reinterpret_cast<const uint32_t *>(p);
#pragma unroll
        for (int k = 0; k < 4; k++) u[k] = ((v >> (8 * k)) & 0xFFu) ^ 0x80u;
    } else if constexpr (PER == 2) {
        const uint32_t v = *reinterpret_cast<const uint16_t *>(p);
        u[0] = (v & 0xFFu) ^ 0x80u, u[1] = (v >> 8) ^ 0x80u;
    } else {
        u[0] = (uint32_t)(uint8_t)*p ^ 0x80u;
    }
}
template <int PER>
__device__ __forceinline__ void scan_load_s(const uint16_t *t, uint32_t (&s)[PER]) {
    if constexpr (PER >= 4) {
        const typename ScanWords<PER / 2>::type v = *reinterpret_cast<const typename ScanWords<PER / 2>::type *>(t);
#pragma unroll
        for (int k = 0; k < PER; k++) s[k] = (v[k / 2] >> (16 * (k % 2))) & 0xFFFFu;
    } else if constexpr (PER == 2) {
        const uint32_t v = *reinterpret_cast<const uint32_t *>(t);
        s[0] = v & 0xFFFFu, s[1] = v >> 16;
    } else {
        s[0] = *t;
    }
}
template <int PER>
__device__ __forceinline__ void scan_store_s(uint16_t *t, const uint32_t (&s)[PER]) {
    if constexpr (PER >= 4) {
        typename ScanWords<PER / 2>::type v;
#pragma unroll
        for (int k = 0; k < PER / 2; k++) v[k] = s[2 * k] | (s[2 * k + 1] << 16);
        *reinterpret_cast<typename ScanWords<PER / 2>::type *>(t) = v;
    } else if constexpr (PER == 2) {
        *reinterpret_cast<uint32_t *>(t) = s[0] | (s[1] << 16);
    } else {
        *t = (uint16_t)s[0];
    }
}
// Lane g owns values [g PER, (g + 1) PER) of the level.  Tiled: they are the level's piece of record g (quantize.h), PER bytes at
// a multiple of PER; level-major: 16 bytes of the level's array.  The loads of a frame do not depend on the trace, so the
// unrolled loop has four frames' loads in flight.
template <int PER>
__global__ __launch_bounds__(256) void k_scan_trace(ScanTraceArgs a) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.lanes) return;
    const int8_t *p = a.src + (a.tiled ? a.map.pos(g) * (size_t)a.rec_bytes + (size_t)a.loff : g * PER);
    uint16_t *t = a.trace + g * PER;
    uint32_t s[PER], u[PER];
    int f = 0;
    if (a.fresh) {
        scan_load_u<PER>(p, u);
#pragma unroll
        for (int k = 0; k < PER; k++) s[k] = scan_first(u[k]);
        p += a.stride, f = 1;
    } else {
        scan_load_s<PER>(t, s);
    }
#pragma unroll 4
    for (; f < a.nframes; f++, p += a.stride) {
        scan_load_u<PER>(p, u);
#pragma unroll
        for (int k = 0; k < PER; k++) s[k] = scan_step(s[k], u[k], a.shift);
    }
    scan_store_s<PER>(t, s);
}

// ---- the evaluation ---------------------------------------------------------------------------------------------------------
// a wave per segment, four adjacent values per lane: 16 rounds of four ballots
__global__ __launch_bounds__(256) void k_scan_floor(ScanEvalArgs a) {
    const int g = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= a.G) return;
    uint32_t x[4];
    scan_load_s<4>(a.trace + (size_t)g * SCAN_SEG + 4 * lane, x);
    const uint32_t q = scan_select(SCAN_RANK, [&](uint32_t prefix, uint32_t mask) {
        int c = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) c += __popcll(__ballot((x[k] & mask) == prefix));
        return c;
    });
    if (lane == 0) a.Q[g] = q;
}
// a wave per mask word, a lane per bin
__global__ __launch_bounds__(256) void k_scan_hot(ScanEvalArgs a) {
    const unsigned w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= a.words) return;
    const int g = (int)(w >> 2);
    const uint32_t F = scan_floor(a.Q, g, a.G);
    const uint64_t m = __ballot(scan_hot(a.trace[(size_t)w * 64 + lane], F, a.threshold));
    if (lane == 0) {
        a.hot[w] = m;
        if ((w & 3) == 0) a.F[g] = F;
    }
}
// One work-group: thread t owns a stretch of adjacent mask words - their start words, then, behind a scan of the threads' counts
// over LDS, the number of starts in front of each.  It also clears the list for k_scan_emit's maxima and writes the total.
__global__ __launch_bounds__(SCAN_MARK_THREADS) void k_scan_mark(ScanEvalArgs a) {
    __shared__ uint32_t part[SCAN_MARK_THREADS];
    const unsigned tid = threadIdx.x;
    const unsigned per = (a.words + SCAN_MARK_THREADS - 1) / SCAN_MARK_THREADS;
    const unsigned w0 = tid * per < a.words ? tid * per : a.words, w1 = w0 + per < a.words ? w0 + per : a.words;
    uint32_t cnt = 0;
    for (unsigned w = w0; w < w1; w++) {
        const uint64_t st = scan_start_word(a.hot[w], w > 0 ? a.hot[w - 1] : 0, w > 1 ? a.hot[w - 2] : 0, a.gap);
        a.starts[w] = st;
        cnt += (uint32_t)scan_popc64(st);
    }
    part[tid] = cnt;
    __syncthreads();
    for (unsigned o = 1; o < SCAN_MARK_THREADS; o <<= 1) {
        const uint32_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t run = part[tid] - cnt;
    for (unsigned w = w0; w < w1; w++) {
        a.base[w] = run;
        run += (uint32_t)scan_popc64(a.starts[w]);  // (this thread's own stores)
    }
    if (tid == SCAN_MARK_THREADS - 1) a.head->total = part[tid];
    for (unsigned i = tid; i < (unsigned)SCAN_CAP; i += SCAN_MARK_THREADS) a.list[i] = ScanRun{0, 0, 0};
}
// A wave per mask word, a lane per bin.  A run's peak is the maximum of its bins' keys, taken by 64-bit atomics into the list's
// entry: every bin of a run takes part at once, however long the run.  Where the wave's bins all belong to one run - the rule in
// a long run - the wave takes its own maximum first and one lane goes to memory.
__global__ __launch_bounds__(256) void k_scan_emit(ScanEvalArgs a) {
    const unsigned w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = threadIdx.x & 63;
    if (w >= a.words) return;
    const uint64_t cur = a.hot[w], p = w > 0 ? a.hot[w - 1] : 0, pp = w > 1 ? a.hot[w - 2] : 0;
    const uint64_t nx = w + 1 < a.words ? a.hot[w + 1] : 0, nnx = w + 2 < a.words ? a.hot[w + 2] : 0;
    if (!cur && (!p || !nx)) return;  // no hot bin here and none on one side: no bin of this word is inside a run
    const uint32_t j = w * 64 + (uint32_t)b;
    const bool hot = (cur >> b) & 1;
    const int below = scan_dist_below(b, cur, p, pp), above = scan_dist_above(b, cur, nx, nnx);
    const uint64_t st = a.starts[w];
    const uint32_t r = scan_run_index(a.base[w], st, b);
    const bool in = scan_inside(hot, below, above, a.gap) && r < (uint32_t)SCAN_CAP;  // (runs past the cap: counted, dropped)
    if (in && ((st >> b) & 1)) a.list[r].first = j;
    if (in && scan_is_end(hot, above, a.gap)) a.list[r].end = j + 1;
    const uint64_t m = __ballot(in);
    if (!m) return;
    unsigned long long key = in ? scan_key(a.trace[j], j) : 0ull;  // (0 is below every key)
    const uint32_t r0 = (uint32_t)__shfl((int)r, __ffsll((unsigned long long)m) - 1);
    if (__ballot(in && r != r0) == 0) {
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const unsigned long long v = __shfl_xor(key, o);
            key = v > key ? v : key;
        }
        if (b == 0) atomicMax(reinterpret_cast<unsigned long long *>(&a.list[r0].key), key);
    } else if (in) {
        atomicMax(reinterpret_cast<unsigned long long *>(&a.list[r].key), key);
    }
}

hipError_t scan_trace_launch(const ScanTraceArgs &a, int per, unsigned blocks, hipStream_t s) {
    switch (per) {
    case 16: hipLaunchKernelGGL(k_scan_trace<16>, dim3(blocks), dim3(256), 0, s, a); break;
    case 8: hipLaunchKernelGGL(k_scan_trace<8>, dim3(blocks), dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL(k_scan_trace<4>, dim3(blocks), dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_scan_trace<2>, dim3(blocks), dim3(256), 0, s, a); break;
    case 1: hipLaunchKernelGGL(k_scan_trace<1>, dim3(blocks), dim3(256), 0, s, a); break;
    default: return hipErrorInvalidValue;  // a missing form is an error, never another path
    }
    return hipGetLastError();
}
hipError_t scan_floor_launch(const ScanEvalArgs &a, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL(k_scan_floor, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t scan_hot_launch(const ScanEvalArgs &a, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL(k_scan_hot, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t scan_mark_launch(const ScanEvalArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_scan_mark, dim3(1), dim3(SCAN_MARK_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t scan_emit_launch(const ScanEvalArgs &a, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL(k_scan_emit, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace psdr

// ---- the calls --------------------------------------------------------------------------------------------------------------
extern "C" int psdr_scan_set(psdr_ctx *c, const psdr_scan_config *cfg) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    if (cfg) {
        const ScanVerdict v = scan_check(c->R, c->levels, *cfg);
        if (v != SCAN_OK) return fail(PSDR_ERR_INVALID, "%s", scan_text(v, c->R, c->levels, *cfg).c_str());
        if (!c->scan) {  // the first on: built whole, then moved in (a failed call leaves the context as it was)
            HIPCHK(hipSetDevice(c->device));
            psdr_ctx::BandScan fresh;
            if (fresh.alloc(*c)) {
                const std::string why = psdr_last_error();
                (void)hipGetLastError();
                return fail(PSDR_ERR_NOMEM, "band scan state (%zu bytes): %s", psdr_ctx::BandScan::bytes(*c), why.c_str());
            }
            c->scan = std::move(fresh);
        }
        c->scan_cfg = *cfg;
    }
    c->scan_on = cfg != nullptr;
    c->scan_st = ScanState();  // the next psdr_scan_batch starts a run; nothing to read until it has evaluated
    return PSDR_OK;
}

extern "C" int psdr_scan_batch(psdr_ctx *c, uint64_t first_frame_num) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    if (!c->scan_on) return fail(PSDR_ERR_STATE, "scan_batch while the band scan is off (psdr_scan_set)");
    if (c->last_nframes < 1) return fail(PSDR_ERR_STATE, "scan_batch before process_batch/execute");
    HIPCHK(hipSetDevice(c->device));
    const psdr_scan_config cfg = c->scan_cfg;
    const int nf = c->last_nframes;
    ScanFacts facts;
    facts.R = c->R, facts.levels = c->levels, facts.tiled_lt = c->tiled_lt, facts.tile_ch = c->tile_ch;
    const ScanLaunch L = scan_launch(facts, cfg.level);
    const ScanStep step = scan_step_plan(c->scan_st, first_frame_num, nf);
    c->scan_st = ScanState();  // (whatever fails below: the next call starts a run)
    ScanTraceArgs ta{};
    ta.src = L.tiled ? c->d_qt : c->d_q + L.qoff;
    ta.stride = L.tiled ? c->qt_stride : c->q_stride;
    ta.trace = c->scan.trace;
    ta.lanes = L.n / (size_t)L.per;
    ta.map = c->recmap;
    ta.rec_bytes = 2 * c->tile_ch, ta.loff = L.loff, ta.tiled = L.tiled ? 1 : 0;
    ta.nframes = nf, ta.fresh = step.fresh ? 1 : 0, ta.shift = cfg.avg_shift;
    ScanEvalArgs ea{};
    ea.trace = c->scan.trace;
    ea.Q = c->scan.Q, ea.F = c->scan.F, ea.hot = c->scan.hot, ea.starts = c->scan.starts, ea.base = c->scan.base;
    ea.list = c->scan.list, ea.head = c->scan.head;
    ea.G = L.G, ea.threshold = cfg.threshold, ea.gap = cfg.gap, ea.words = (unsigned)L.words;
    {
        ProfScope ps(c, K_SCAN_TRACE, c->side);
        HIPCHK(scan_trace_launch(ta, L.per, L.trace_blocks, c->side));
    }
    {
        ProfScope ps(c, K_SCAN_FLOOR, c->side);
        HIPCHK(scan_floor_launch(ea, L.floor_blocks, c->side));
    }
    {
        ProfScope ps(c, K_SCAN_HOT, c->side);
        HIPCHK(scan_hot_launch(ea, L.hot_blocks, c->side));
    }
    {
        ProfScope ps(c, K_SCAN_MARK, c->side);
        HIPCHK(scan_mark_launch(ea, c->side));
    }
    {
        ProfScope ps(c, K_SCAN_EMIT, c->side);
        HIPCHK(scan_emit_launch(ea, L.emit_blocks, c->side));
    }
    c->scan_st = step.after;
    return side_done(c);
}

// the read calls' common start: something was evaluated, and it is at rest
static int scan_at_rest(psdr_ctx *c) {
    if (!c->scan_st.evaluated) return fail(PSDR_ERR_NO_DATA, "no band scan was evaluated yet (psdr_scan_batch)");
    HIPCHK(hipSetDevice(c->device));
    return drain(c);
}
template <typename T>
static int scan_copy(psdr_ctx *c, T *dst, const T *src, size_t count) {
    HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PSDR_OK;
}
extern "C" int psdr_read_signals(psdr_ctx *c, int min_width, psdr_signal *out, int cap, int *n_out, int *total_out, uint64_t *frame_num_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (cap < 0) return fail(PSDR_ERR_INVALID, "read_signals: cap %d is negative", cap);
    std::lock_guard<std::mutex> lk(c->mtx);
    PSDRCHK(scan_at_rest(c));
    ScanHead head;
    PSDRCHK(scan_copy(c, &head, c->scan.head.get(), 1));
    const int kept = scan_kept(head.total), G = (int)((c->R >> c->scan_cfg.level) / SCAN_SEG);
    std::vector<ScanRun> list((size_t)kept);
    std::vector<uint32_t> F((size_t)G);
    if (kept) PSDRCHK(scan_copy(c, list.data(), c->scan.list.get(), (size_t)kept));
    PSDRCHK(scan_copy(c, F.data(), c->scan.F.get(), (size_t)G));
    const int n = scan_filter(list.data(), kept, F.data(), min_width, out, cap);
    if (n_out) *n_out = n;
    if (total_out) *total_out = (int)head.total;
    if (frame_num_out) *frame_num_out = c->scan_st.last_frame;
    return PSDR_OK;
}
extern "C" int psdr_read_scan_floor(psdr_ctx *c, uint32_t *F, int cap, int *nseg_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    PSDRCHK(scan_at_rest(c));
    const int G = (int)((c->R >> c->scan_cfg.level) / SCAN_SEG);
    if (nseg_out) *nseg_out = G;
    if (!F) return PSDR_OK;
    if (cap < G) return fail(PSDR_ERR_INVALID, "output buffer too small (%d < %d segments)", cap, G);
    return scan_copy(c, F, c->scan.F.get(), (size_t)G);
}
extern "C" int psdr_read_scan_trace(psdr_ctx *c, uint16_t *s, size_t cap, size_t *n_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    PSDRCHK(scan_at_rest(c));
    const size_t n = c->R >> c->scan_cfg.level;
    if (n_out) *n_out = n;
    if (!s) return PSDR_OK;
    if (cap < n) return fail(PSDR_ERR_INVALID, "output buffer too small (%zu < %zu bins)", cap, n);
    return scan_copy(c, s, c->scan.trace.get(), n);
}

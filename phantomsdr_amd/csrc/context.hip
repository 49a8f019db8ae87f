// context.hip - lifetime of a context (tables, buffers, streams), Level 1 of the C-ABI (the FFT plug-in: host buffers,
// load_*_input, execute), device-memory helpers, the streaming ingest ring and the instrumentation.  No kernels here.
#include "ctx.h"

static thread_local std::string g_err;
int psdr_fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
extern "C" const char *psdr_last_error(void) { return g_err.c_str(); }
extern "C" int psdr_abi_version(void) { return PSDR_ABI_VERSION; }
extern "C" const char *psdr_version(void) {
#ifdef PSDR_TUNING_BUILD
    return "phantomsdr_amd 0.3 (gfx950, tuning build)";  // reads the A/B knobs of psdr_tuning_env(); not the library that ships
#else
    return "phantomsdr_amd 0.3 (gfx950)";
#endif
}

namespace psdr {
const char *kKernelNames[K_COUNT] = {"fft_pass1",  "fft_pass2", "untangle_real", "pyramid_tail",
                                     "demod_idft", "demod_ola", "waterfall_gather", "post_chain",
                                     "real_seam",  "band_pack",  "waterfall_hold", "waterfall_carry",
                                     "squelch",    "blanker_scan", "blanker_apply",  "audio_filter", "audio_nr", "audio_nb",
                                     "scan_trace", "scan_floor",   "scan_hot",       "scan_mark",    "scan_emit", "audio_tone", "audio_cw", "audio_rtty", "audio_psk", "audio_fax"};

void resolve_pending(psdr_ctx *c) {
    if (c->pending.empty()) return;
    hipStreamSynchronize(c->stream);
    hipStreamSynchronize(c->side);
    for (hipStream_t st : c->pc_s)
        if (st) hipStreamSynchronize(st);
    for (auto &p : c->pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            c->k_ms[p.kid] += ms;
            c->k_n[p.kid] += 1;
            if (c->k_samples[p.kid].size() < 65536) c->k_samples[p.kid].push_back(ms * 1e3f);
        }
        c->pool.push_back(std::move(p.a));
        c->pool.push_back(std::move(p.b));
    }
    c->pending.clear();
}

// mode 2: the stamps of the launches since the last call -> k_ms / k_n / k_samples of the two passes
void resolve_kclock(psdr_ctx *c) {
    if (!c->d_kclk) return;
    bool any = false;
    for (int w = 0; w < 2; w++) any = any || c->kclk_done[w] < std::min(c->kclk_pos[w], psdr_ctx::KCLK_SLOTS);
    if (!any) return;
    hipStreamSynchronize(c->stream);
    std::vector<unsigned long long> h((size_t)2 * psdr_ctx::KCLK_SLOTS * 2);
    if (hipMemcpy(h.data(), c->d_kclk, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return;
    for (int w = 0; w < 2; w++) {
        const int kid = w == 0 ? K_PASS1 : K_PASS2;
        const unsigned end = std::min(c->kclk_pos[w], psdr_ctx::KCLK_SLOTS);
        for (unsigned i = c->kclk_done[w]; i < end; i++) {
            const unsigned long long b = h[((size_t)w * psdr_ctx::KCLK_SLOTS + i) * 2], e = h[((size_t)w * psdr_ctx::KCLK_SLOTS + i) * 2 + 1];
            if (e <= b) continue;  // (never launched / no work-group ran)
            const double us = (double)(e - b) * 1e3 / c->wall_clock_khz;
            c->k_ms[kid] += us * 1e-3;
            c->k_n[kid] += 1;
            if (c->k_samples[kid].size() < 65536) c->k_samples[kid].push_back((float)us);
        }
        c->kclk_done[w] = end;
    }
}
// re-arm the whole ring: begin = ~0, end = 0 (streams drained by the caller)
int reset_kclock(psdr_ctx *c) {
    if (!c->d_kclk) return PSDR_OK;
    std::vector<unsigned long long> h((size_t)2 * psdr_ctx::KCLK_SLOTS * 2);
    for (size_t i = 0; i < h.size(); i += 2) h[i] = ~0ull, h[i + 1] = 0ull;
    HIPCHK(hipMemcpy(c->d_kclk, h.data(), h.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    c->kclk_pos[0] = c->kclk_pos[1] = c->kclk_done[0] = c->kclk_done[1] = 0;
    return PSDR_OK;
}

}  // namespace psdr

namespace {

size_t fmt_bytes(int fmt) {
    switch (fmt) {
    case PSDR_FMT_U8:
    case PSDR_FMT_S8:
        return 1;
    case PSDR_FMT_U16:
    case PSDR_FMT_S16:
        return 2;
    case PSDR_FMT_F32:
        return 4;
    default:
        return 8;
    }
}

// a table of twiddle_plan (a table it leaves out stays unallocated)
int upload(DevBuf<cf> &dst, const Twiddles &t) {
    if (!t.count) return PSDR_OK;
    const std::vector<Twiddle> w = make_twiddles(t);
    PSDRCHK(dst.alloc(w.size()));
    HIPCHK(hipMemcpy(dst, w.data(), w.size() * sizeof(cf), hipMemcpyHostToDevice));
    return PSDR_OK;
}
// a buffer of buffer_plan (one it leaves out stays unallocated)
template <typename B>
int alloc(B &dst, const Buf &b) {
    return b.count ? dst.alloc(b.count) : PSDR_OK;
}
template <typename T>
int alloc(DevBuf<T> &dst, const Buf &b) {
    return b.count ? dst.alloc(b.count, b.zero) : PSDR_OK;
}

// the knobs of ctx.h and the device's size, read once
int read_env(int device, CreateEnv &env) {
    const char *e = getenv("PSDR_REAL_SPLIT");
    env.real_split_2048x1024 = e && strcmp(e, "2048x1024") == 0;
    env.real_3pass = getenv("PSDR_REAL_3PASS") != nullptr;
    if ((e = getenv("PSDR_SEG_LEN"))) env.seg_len = atoi(e);
    if ((e = getenv("PSDR_DEMOD_CHAIN"))) env.demod_chain = atoi(e) != 0;
    if ((e = getenv("PSDR_DEMOD_K"))) env.demod_chain_k = std::max(1, atoi(e));
    if ((e = psdr_tuning_env("PSDR_LOG2M2"))) env.log2M2 = atoi(e);  // tuning: split M = M1 * M2
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    env.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    return PSDR_OK;
}

// the one place the context's create-time fields are assigned
void adopt(psdr_ctx *c, const psdr_config &cfg, const CreateEnv &env, const ShapePlan &s, const IdftPlan &d) {
    c->cfg = cfg;
    c->cfg.skip_num = s.skip_num;
    c->shape = s;
    c->device = cfg.device;
    c->num_cus = env.num_cus;
    c->N = s.N, c->M = s.M, c->R = s.R, c->is_real = s.is_real;
    c->log2M1 = s.log2M1, c->log2M2 = s.log2M2, c->M1 = s.M1, c->M2 = s.M2, c->T1 = s.T1, c->T2 = s.T2;
    c->size_log2 = s.size_log2, c->levels = s.levels, c->max_batch = s.max_batch;
    c->spec_stride = s.spec_stride, c->q_len = s.q_len, c->q_stride = s.q_stride, c->qt_stride = s.qt_stride, c->p_stride = s.p_stride;
    c->real_fused = s.real_fused, c->tile_ch = s.tile_ch, c->LT = s.LT, c->tiled_lt = s.tiled_lt;
    c->min_waterfall_fft = s.min_waterfall_fft, c->log2UB = s.log2UB;
    c->recmap = s.recmap, c->lay = s.lay, c->seg_facts = s.seg;
    c->tails = tails_plan(s.tail);  // the pyramid levels above the tile
    c->n = d.n, c->idft_kind = d.kind, c->nstages = d.nstages;
    std::copy(d.radix, d.radix + PSDR_MAX_STAGES, c->radix);
    c->lds_mode = d.lds_mode, c->idft_lds = d.idft_lds, c->idft_threads = d.idft_threads;
    c->demod_chain = env.demod_chain, c->demod_chain_k = env.demod_chain_k;
}

int build(psdr_ctx *c, const IdftPlan &idft) {
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(c->own_stream.create());
    {
        // the consumers are short kernels that must squeeze in next to the persistent FFT
        // work-groups: give their stream the highest priority (the other way round, and the passes' stream at the
        // highest, measured within +-1 %: docs/history.md section 5)
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        PSDRCHK(c->own_side.create(hi));
    }
    c->stream = c->own_stream;
    c->side = c->own_side;
    // (both passes run on `stream`; the first pass of batch b+1 on a stream of its own beside the second pass of batch b
    // was measured in rounds 1-3 - -12 % at F = 16, nothing from F = 32 on - and taken out in round 5)
    PSDRCHK(c->ev_in.create());
    PSDRCHK(c->ev_fft_done.create());
    PSDRCHK(c->ev_side_done.create());
    PSDRCHK(c->t0.create_timing());
    PSDRCHK(c->t1.create_timing());
    for (int s = 0; s < 2; s++) PSDRCHK(c->ev_set_done[s].create());

    // ---- twiddles.  The Hann window (build_hann_window, src/utils/dsp.cpp:6-11) is evaluated inside pass 1 from these
    // tables; only W_N^1 (odd real samples) is needed on top of them.
    const Twiddle w1 = make_twiddles(Twiddles{2, 1, c->N, -1})[1];
    c->wdelta = make_float2(w1.x, w1.y);
    const TwiddlePlan tw = twiddle_plan(c->shape);
    PSDRCHK(upload(c->d_Wl1, tw.Wl1));
    PSDRCHK(upload(c->own_Wl2, tw.Wl2));
    c->d_Wl2 = tw.Wl2.count ? c->own_Wl2 : c->d_Wl1;
    PSDRCHK(upload(c->d_TB, tw.TB));
    PSDRCHK(upload(c->d_UA, tw.UA));
    PSDRCHK(upload(c->d_UB, tw.UB));
    PSDRCHK(upload(c->d_UG, tw.UG));
    PSDRCHK(upload(c->d_Wn, tw.Wn));
    if (idft.nstages) {
        std::vector<IdftEntry> tab((size_t)idft.nstages * idft.n);
        idft_stage_table(idft, tab.data());
        PSDRCHK(c->d_stage_tab.alloc(tab.size()));
        HIPCHK(hipMemcpy(c->d_stage_tab, tab.data(), tab.size() * sizeof(int4), hipMemcpyHostToDevice));
    }
#ifdef PSDR_TRACE_ON
    PSDRCHK(c->d_trace.alloc(4864, true));
#endif
    // ---- buffers
    const BufferPlan b = buffer_plan(c->shape, c->cfg);
    for (auto &t : c->d_tickets) PSDRCHK(alloc(t, b.tickets));
    PSDRCHK(alloc(c->d_Y, b.Y));
    PSDRCHK(alloc(c->d_Z, b.Z));
    c->seg_cap = b.seg_cap;
    for (int st = 0; st < 2; st++) {  // part of the double-buffered result sets: k_real_seam is a consumer
        PSDRCHK(alloc(c->seam_pool[st][0], b.seamP));
        PSDRCHK(alloc(c->seam_pool[st][1], b.seamC));
    }
    // flags (inside a launch only), then the fallback marks - ONE ARRAY PER RESULT SET: k_real_seam is a consumer, it may
    // run after the next batch's second pass has started writing its own marks
    PSDRCHK(alloc(c->d_segflag, b.segflag));
    for (int s = 0; s < 2; s++) {
        PSDRCHK(alloc(c->spec_pool[s], b.spec));
        PSDRCHK(alloc(c->q_pool[s], b.q));
        PSDRCHK(alloc(c->qt_pool[s], b.qt));
        PSDRCHK(alloc(c->pscr_pool[s][0], b.pscr));
        PSDRCHK(alloc(c->pscr_pool[s][1], b.pscr));
    }
    select_set(c, 0);
    c->q_untiled.assign((size_t)c->max_batch, 0);
    PSDRCHK(alloc(c->d_stage, b.stage));  // level-1 staging
    PSDRCHK(alloc(c->h_out, b.h_out));
    PSDRCHK(alloc(c->h_q, b.h_q));
    // ---- audio clients
    c->aslots.resize(b.slots);
    PSDRCHK(alloc(c->d_ypost, b.ypost));
    for (int k = 0; k < 2; k++) {
        PSDRCHK(alloc(c->pwr_pool[k], b.pwr));
        PSDRCHK(alloc(c->audio_pool[k], b.audio));
        PSDRCHK(alloc(c->nan_pool[k], b.nan));
    }
    c->d_pwr = c->pwr_pool[0], c->d_audio = c->audio_pool[0], c->d_nan = c->nan_pool[0];
    PSDRCHK(alloc(c->d_real_prev, b.real_prev));
    PSDRCHK(alloc(c->d_bb_tail, b.bb_tail));
    PSDRCHK(alloc(c->d_bb_last, b.bb_last));
    PSDRCHK(alloc(c->d_ssb_mark, b.ssb_mark));
    PSDRCHK(alloc(c->d_gscratch, b.gscratch));
    // the batch's client list + the slot -> list index table; behind them the tuned clients' list (ctx.h: ft_ring_off)
    if (b.client_ring && c->client_ring.init(b.client_ring)) return fail(PSDR_ERR_HIP, "client parameter ring allocation failed");
    // ---- waterfall clients
    c->wslots.resize(b.wslots);
    c->wf_sent_off = b.wf_sent_off;
    if (c->wf_ring.init(b.wf_ring)) return fail(PSDR_ERR_HIP, "waterfall parameter ring allocation failed");
    if (c->real_fused) {  // the plans of the two batch sizes every caller uses, now rather than in the first batch (a synchronous upload)
        const psdr_ctx::SegPlan *sp;
        PSDRCHK(seg_plan(c, c->max_batch, &sp));
        if (c->max_batch > 1) PSDRCHK(seg_plan(c, 1, &sp));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipDeviceSynchronize());
    return PSDR_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------
extern "C" int psdr_create(const psdr_config *cfg, psdr_ctx **out) {
    if (!cfg || !out) return fail(PSDR_ERR_INVALID, "null argument");
    if (cfg->struct_size != sizeof(psdr_config))
        return fail(PSDR_ERR_INVALID, "psdr_config.struct_size mismatch (%u vs %zu)",
                    cfg->struct_size, sizeof(psdr_config));
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail(PSDR_ERR_NO_DEVICE, "No HIP devices found");
    if (cfg->device < 0 || cfg->device >= count)
        return fail(PSDR_ERR_INVALID, "device %d out of range (%d devices)", cfg->device, count);
    const PlanStatus ok = create_check(*cfg);
    if (ok.code) return fail(ok.code, "%s", ok.msg.c_str());
    CreateEnv env;
    PSDRCHK(read_env(cfg->device, env));
    const ShapePlan shape = shape_plan(*cfg, env);
    const IdftPlan idft = idft_plan(cfg->audio_fft_size);
    if (idft.st.code) return fail(idft.st.code, "%s", idft.st.msg.c_str());
    psdr_ctx *c = new (std::nothrow) psdr_ctx();
    if (!c) return fail(PSDR_ERR_NOMEM, "out of memory");
    adopt(c, *cfg, env, shape, idft);
    int rc = build(c, idft);
    if (rc) {
        delete c;
        return rc;
    }
    *out = c;
    return PSDR_OK;
}

extern "C" void psdr_destroy(psdr_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->side) hipStreamSynchronize(c->side);
    delete c;  // (every buffer, event and stream goes with the member that owns it)
}

// ---- level 1 ---------------------------------------------------------------------------
extern "C" int psdr_host_alloc(psdr_ctx *c, size_t nfloats, float **out) {
    if (!out) return fail(PSDR_ERR_INVALID, "null argument");
    // ctx may be NULL: the reference allocates its half-frame buffers before planning
    // (src/fft.cpp:17-29), i.e. before the back-end knows whether the input is real
    if (c) HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipHostMalloc((void **)out, std::max<size_t>(nfloats, 1) * sizeof(float),
                         hipHostMallocDefault));
    return PSDR_OK;
}
extern "C" int psdr_host_free(psdr_ctx *, float *buf) {
    if (buf) HIPCHK(hipHostFree(buf));
    return PSDR_OK;
}
static int load_input(psdr_ctx *c, const float *a1, const float *a2) {
    if (!c || !a1 || !a2) return fail(PSDR_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(c->device));
    const size_t half_floats = c->is_real ? c->N / 2 : c->N;
    HIPCHK(hipMemcpyAsync(c->d_stage, a1, half_floats * sizeof(float), hipMemcpyHostToDevice,
                          c->stream));
    HIPCHK(hipMemcpyAsync(c->d_stage + half_floats, a2, half_floats * sizeof(float),
                          hipMemcpyHostToDevice, c->stream));
    c->loaded = true;
    c->input_on_main = true;
    return PSDR_OK;
}
extern "C" int psdr_load_real_input(psdr_ctx *c, const float *a1, const float *a2) {
    if (c && !c->is_real) return fail(PSDR_ERR_STATE, "context was planned for complex input");
    return load_input(c, a1, a2);
}
extern "C" int psdr_load_complex_input(psdr_ctx *c, const float *a1, const float *a2) {
    if (c && c->is_real) return fail(PSDR_ERR_STATE, "context was planned for real input");
    return load_input(c, a1, a2);
}
extern "C" int psdr_execute(psdr_ctx *c) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (!c->loaded) return fail(PSDR_ERR_STATE, "execute() before load_*_input()");
    HIPCHK(hipSetDevice(c->device));
    int rc = process_frames(c, c->d_stage, 1, PSDR_FMT_F32);
    if (rc) return rc;
    rc = drain(c);
    if (rc) return rc;
    c->executed = true;
    return PSDR_OK;
}

// make the level-major copy of frame `frame`'s pyramid current (levels 0..LT live in tiled
// ---- device helpers ----------------------------------------------------------------------
extern "C" int psdr_dev_alloc(psdr_ctx *c, size_t bytes, void **out) {
    if (!c || !out) return fail(PSDR_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc(out, std::max<size_t>(bytes, 16)));
    return PSDR_OK;
}
extern "C" int psdr_dev_free(psdr_ctx *c, void *p) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (p) HIPCHK(hipFree(p));
    return PSDR_OK;
}
extern "C" int psdr_memcpy_h2d(psdr_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c || !dst || !src) return fail(PSDR_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PSDR_OK;
}
extern "C" int psdr_memcpy_d2h(psdr_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c || !dst || !src) return fail(PSDR_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(c->device));
    {
        int rc = drain(c);
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PSDR_OK;
}
extern "C" int psdr_synchronize(psdr_ctx *c) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    return drain(c);
}
extern "C" size_t psdr_half_frame_bytes(const psdr_ctx *c) {
    if (!c) return 0;
    return (c->N / 2) * (c->is_real ? 1 : 2) * fmt_bytes(c->cfg.input_format);
}

// ---- level 2 -----------------------------------------------------------------------------
extern "C" int psdr_process_batch(psdr_ctx *c, const void *d_halves, int nframes) {
    if (!c || !d_halves) return fail(PSDR_ERR_INVALID, "null argument");
    if (nframes < 1 || nframes > c->max_batch)
        return fail(PSDR_ERR_INVALID, "nframes %d outside [1, max_batch=%d]", nframes, c->max_batch);
    HIPCHK(hipSetDevice(c->device));
    return process_frames(c, d_halves, nframes, c->cfg.input_format);
}

// ---- streaming ingest (src/fft.cpp:56-67, src/samplereader.cpp:42-70 on the device) -----------------
extern "C" int psdr_ring_create(psdr_ctx *c, int nhalves) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (nhalves < 2) return fail(PSDR_ERR_INVALID, "a ring needs at least 2 half-frames");
    if (c->ring.d) return fail(PSDR_ERR_STATE, "the context already has an ingest ring");
    HIPCHK(hipSetDevice(c->device));
    psdr_ctx::IngestRing r;  // built whole, then moved in: a failure leaves the context without a ring
    r.hb = psdr_half_frame_bytes(c);
    r.nhalves = nhalves;
    PSDRCHK(r.d.alloc((size_t)(nhalves + 1) * r.hb, true));
    PSDRCHK(r.copy.create());
    r.ev_written.resize(nhalves);
    r.ever_written.assign(nhalves, 0);
    r.reader_seq.assign(nhalves, 0);
    for (auto &e : r.ev_written) PSDRCHK(e.create());
    for (auto &e : r.ev_read) PSDRCHK(e.create());
    c->ring = std::move(r);
    return PSDR_OK;
}
extern "C" int psdr_ring_write_async(psdr_ctx *c, uint64_t half_index, const void *host_half) {
    if (!c || !host_half) return fail(PSDR_ERR_INVALID, "null argument");
    auto &r = c->ring;
    if (!r.d) return fail(PSDR_ERR_STATE, "psdr_ring_create() first");
    HIPCHK(hipSetDevice(c->device));
    const int slot = (int)(half_index % (uint64_t)r.nhalves);
    // the slot's previous content may still be waiting for its reader (a process call issued at
    // most NEV calls ago: older ones were waited for when their event was reused)
    const uint64_t rs = r.reader_seq[slot];
    if (rs && r.seq - rs < (uint64_t)psdr_ctx::IngestRing::NEV)
        HIPCHK(hipStreamWaitEvent(r.copy, r.ev_read[rs % psdr_ctx::IngestRing::NEV], 0));
    if (slot == 0 && r.reader_seq[r.nhalves - 1]) {  // the mirror of slot 0 is read with the LAST slot's frame
        const uint64_t rl = r.reader_seq[r.nhalves - 1];
        if (r.seq - rl < (uint64_t)psdr_ctx::IngestRing::NEV)
            HIPCHK(hipStreamWaitEvent(r.copy, r.ev_read[rl % psdr_ctx::IngestRing::NEV], 0));
    }
    HIPCHK(hipMemcpyAsync(r.d + (size_t)slot * r.hb, host_half, r.hb, hipMemcpyHostToDevice, r.copy));
    if (slot == 0)
        HIPCHK(hipMemcpyAsync(r.d + (size_t)r.nhalves * r.hb, host_half, r.hb, hipMemcpyHostToDevice, r.copy));
    HIPCHK(hipEventRecord(r.ev_written[slot], r.copy));
    r.ever_written[slot] = 1;
    return PSDR_OK;
}
extern "C" int psdr_ring_wait(psdr_ctx *c, uint64_t half_index) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    auto &r = c->ring;
    if (!r.d) return fail(PSDR_ERR_STATE, "psdr_ring_create() first");
    const int slot = (int)(half_index % (uint64_t)r.nhalves);
    if (r.ever_written[slot]) HIPCHK(hipEventSynchronize(r.ev_written[slot]));
    return PSDR_OK;
}
extern "C" int psdr_process_ring(psdr_ctx *c, uint64_t first_half, int nframes) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    auto &r = c->ring;
    if (!r.d) return fail(PSDR_ERR_STATE, "psdr_ring_create() first");
    if (nframes < 1 || nframes > c->max_batch)
        return fail(PSDR_ERR_INVALID, "nframes %d outside [1, max_batch=%d]", nframes, c->max_batch);
    const int s0 = (int)(first_half % (uint64_t)r.nhalves);
    if (s0 + nframes > r.nhalves)
        return fail(PSDR_ERR_INVALID, "frames %d..%d cross the end of the %d-half ring (one guard half-frame): split the batch",
                    s0, s0 + nframes - 1, r.nhalves);
    HIPCHK(hipSetDevice(c->device));
    for (int i = 0; i <= nframes; i++) {  // halves s0 .. s0+nframes (the last may be the mirror of slot 0)
        const int slot = (s0 + i) % r.nhalves;
        if (!r.ever_written[slot]) return fail(PSDR_ERR_STATE, "half-frame slot %d was never written", slot);
        HIPCHK(hipStreamWaitEvent(c->stream, r.ev_written[slot], 0));
    }
    r.seq++;
    hipEvent_t ev = r.ev_read[r.seq % psdr_ctx::IngestRing::NEV];
    HIPCHK(hipEventSynchronize(ev));  // the call that used it NEV calls ago (no-op if never recorded)
    // the impulse blanker (blanker.hip): behind the waits for the copies, in front of pass 1, so that `ev` covers it too
    if (c->nb.on)
        PSDRCHK(blanker_enqueue(c, first_half, nframes));
    else
        c->nb.last_n = 0;
    int rc = process_frames(c, r.d + (size_t)s0 * r.hb, nframes, c->cfg.input_format, ev);
    if (rc) return rc;
    for (int i = 0; i <= nframes; i++) r.reader_seq[(s0 + i) % r.nhalves] = r.seq;
    return PSDR_OK;
}

int psdr::side_done(psdr_ctx *c) {
    if (c->side == c->stream) return PSDR_OK;
    HIPCHK(hipEventRecord(c->ev_side_done, c->side));
    c->side_pending = true;
    HIPCHK(hipEventRecord(c->ev_set_done[c->cur_set], c->side));
    c->set_pending[c->cur_set] = true;
    return PSDR_OK;
}
int psdr::drain(psdr_ctx *c) {
    if (c->ring.copy) HIPCHK(hipStreamSynchronize(c->ring.copy));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->side != c->stream) HIPCHK(hipStreamSynchronize(c->side));
    for (hipStream_t st : c->pc_s)
        if (st) HIPCHK(hipStreamSynchronize(st));
    if (c->fetch_stream) HIPCHK(hipStreamSynchronize(c->fetch_stream));
    if (c->fetch_stream_pcm) HIPCHK(hipStreamSynchronize(c->fetch_stream_pcm));
    return PSDR_OK;
}

// ---- instrumentation -------------------------------------------------------------------------
extern "C" int psdr_set_profiling(psdr_ctx *c, int mode) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (mode < 0 || mode > 2) return fail(PSDR_ERR_INVALID, "profiling mode %d (0 off, 1 hipEvents, 2 device clocks)", mode);
    HIPCHK(hipSetDevice(c->device));
    resolve_pending(c);
    resolve_kclock(c);
    c->profiling = mode == 1;
    if (mode == 2 && !c->d_kclk) {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) == hipSuccess && khz > 0) c->wall_clock_khz = khz;
        PSDRCHK(c->d_kclk.alloc((size_t)2 * psdr_ctx::KCLK_SLOTS * 2));
        int rc = drain(c);
        if (rc) return rc;
        rc = reset_kclock(c);
        if (rc) return rc;
    }
    c->kclock = mode == 2;
    return PSDR_OK;
}
extern "C" int psdr_get_kernel_samples(psdr_ctx *c, const char *name, double *us_out, int cap, int *n_out) {
    if (!c || !name || !n_out) return fail(PSDR_ERR_INVALID, "null argument");
    resolve_pending(c);
    resolve_kclock(c);
    for (int k = 0; k < K_COUNT; k++) {
        if (strcmp(name, kKernelNames[k]) != 0) continue;
        const int n = (int)c->k_samples[k].size();
        for (int i = 0; i < n && i < cap && us_out; i++) us_out[i] = c->k_samples[k][i];
        *n_out = n;
        return PSDR_OK;
    }
    return fail(PSDR_ERR_INVALID, "no kernel named '%s'", name);
}
extern "C" int psdr_get_kernel_stats(psdr_ctx *c, int max_entries, const char **names, double *total_ms,
                                     int64_t *launches, int *n_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    resolve_pending(c);
    resolve_kclock(c);
    int n = 0;
    for (int k = 0; k < K_COUNT && n < max_entries; k++) {
        if (c->k_n[k] == 0) continue;
        if (names) names[n] = kKernelNames[k];
        if (total_ms) total_ms[n] = c->k_ms[k];
        if (launches) launches[n] = c->k_n[k];
        n++;
    }
    if (n_out) *n_out = n;
    return PSDR_OK;
}
extern "C" int psdr_reset_kernel_stats(psdr_ctx *c) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    resolve_pending(c);
    for (int k = 0; k < K_COUNT; k++) {
        c->k_ms[k] = 0;
        c->k_n[k] = 0;
        c->k_samples[k].clear();
    }
    if (c->d_kclk) {  // re-arm the stamp ring
        HIPCHK(hipSetDevice(c->device));
        int rc = drain(c);
        if (rc) return rc;
        return reset_kclock(c);
    }
    return PSDR_OK;
}
extern "C" int psdr_timer_start(psdr_ctx *c) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    HIPCHK(hipEventRecord(c->t0, c->stream));
    return PSDR_OK;
}
extern "C" int psdr_timer_stop_ms(psdr_ctx *c, double *ms_out) {
    if (!c || !ms_out) return fail(PSDR_ERR_INVALID, "null argument");
    if (c->side_pending && c->side != c->stream) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_side_done, 0));
    if (c->chain_pending && c->chain_seq > 0) HIPCHK(hipStreamWaitEvent(c->stream, c->pc.ev[3][(c->chain_seq - 1) % psdr_ctx::PC_SETS], 0));
    HIPCHK(hipEventRecord(c->t1, c->stream));
    HIPCHK(hipEventSynchronize(c->t1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->t0, c->t1));
    *ms_out = ms;
    return PSDR_OK;
}
extern "C" void *psdr_stream(psdr_ctx *c) { return c ? (void *)c->stream : nullptr; }
// tuning builds (-DPSDR_TRACE_ON): 4864 values; pass 1 at [0], pass 2 at [128 + 2304]: 128 phase
// stamps of work-group 0 ([iteration 0..7][16]) ... [256..]: wall clock [work-group][8]
extern "C" int psdr_debug_trace(psdr_ctx *c, unsigned long long *out256) {
    if (!c || !out256) return fail(PSDR_ERR_INVALID, "null argument");
    if (!c->d_trace) return fail(PSDR_ERR_UNSUPPORTED, "library built without PSDR_TRACE_ON");
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out256, c->d_trace, 4864 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PSDR_OK;
}
// (not in psdr.h: tools/seg_fallbacks.py and the hand-off test) segments of the LAST fused real-input launch, and how many
// of them did not find their carried row in memory in time and fell back to a seam (fft_pass.h: hand-off); 0 / 0 when the
// launch used uniform segments
extern "C" int psdr_debug_seg_fallbacks(psdr_ctx *c, unsigned *nsegs, unsigned *fallbacks, unsigned char *which, unsigned cap) {
    if (!c || !nsegs || !fallbacks) return fail(PSDR_ERR_INVALID, "null argument");
    *nsegs = *fallbacks = 0;
    if (!c->real_fused || !c->d_segflag || c->last_nframes <= 0) return PSDR_OK;
    const psdr_ctx::SegPlan *plan = nullptr;
    for (const auto &sp : c->seg_plans)
        if (sp.nframes == c->last_nframes) plan = &sp;
    if (!plan || !plan->handoff) return PSDR_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<unsigned> m(plan->nsegs);
    HIPCHK(hipMemcpy(m.data(), c->d_segflag + (size_t)(1 + c->cur_set) * c->seg_cap, m.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    *nsegs = plan->nsegs;
    for (unsigned i = 0; i < plan->nsegs; i++) {
        const bool fb = m[i] == c->seg_epoch;
        *fallbacks += fb;
        if (which && i < cap) which[i] = fb;  // (level-major: segment i is level i / nframes of frame i % nframes)
    }
    return PSDR_OK;
}
extern "C" int psdr_set_stream(psdr_ctx *c, void *hip_stream) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    {
        int rc = drain(c);
        if (rc) return rc;
    }
    resolve_pending(c);
    c->side_pending = false;
    c->set_pending[0] = c->set_pending[1] = false;
    select_set(c, 0);
    if (hip_stream) {  // everything in order on the caller's stream
        c->stream = (hipStream_t)hip_stream;
        c->side = c->stream;
    } else {
        c->stream = c->own_stream;
        c->side = c->own_side;
    }
    if (c->post_ready) pc_replan(c);  // (whether the post chain is a pipeline is one of its plan's facts)
    return PSDR_OK;
}

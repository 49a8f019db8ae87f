// postchain.hip - the post-demodulation chain of AudioClient::send_audio (src/signal.cpp:277-284) for all clients of a
// batch: DC blocker, AGC, int16 conversion (postchain.h) as a four-stage pipeline across batches over three rotating buffer sets.
#include <chrono>

#include "ctx.h"
#include "postchain.h"

// ---- post-demodulation chain ---------------------------------------------------
// Which hardware queue a stream gets is the runtime's business (round robin over the process's queues: it depends on every
// stream the process ever made), and it matters: a busy queue on the SAME pipe of the command processor as the main
// stream's makes every launch of the passes start 50 - 60 us late instead of 6 - 9 (4 % of the step; in a second context of
// the same process - bench.py's sub-workloads - the chain's stream landed exactly there: +35 % instead of +16 % with 256
// clients; on the side stream's pipe it is worse: its many short kernels wait, the passes wait for them, +52 %).  HIP
// does not tell, so the streams are CHOSEN BY MEASUREMENT when the chain is first enabled: of six candidates, the two
// beside which sixteen empty kernels on the main stream AND on the side stream take the least time while the candidate
// runs a 2 ms kernel (2 us against 6 per launch) - and which run side by side with each other and with the side stream
// (two streams can share a queue).  ~60 ms, once per context.
namespace {
__global__ void k_pc_spin(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
__global__ void k_pc_nop() {}

int pc_launch_gap_us(psdr_ctx *c, hipStream_t cand, hipStream_t on, double *us) {
    Event a, b;
    PSDRCHK(a.create_timing());
    PSDRCHK(b.create_timing());
    const unsigned long long ticks = (unsigned long long)(c->wall_clock_khz * 2.0);  // 2 ms
    hipLaunchKernelGGL(k_pc_spin, dim3(1), dim3(64), 0, cand, ticks);
    HIPCHK(hipEventRecord(a, on));
    for (int i = 0; i < 16; i++) hipLaunchKernelGGL(k_pc_nop, dim3(1), dim3(64), 0, on);
    HIPCHK(hipEventRecord(b, on));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    HIPCHK(hipStreamSynchronize(cand));
    *us = ms * 1e3 / 16.0;
    return PSDR_OK;
}
// do two streams run side by side?  (2 ms on either: ~2 ms together, ~4 ms in the same queue)
int pc_side_by_side(psdr_ctx *c, hipStream_t s1, hipStream_t s2, bool *yes) {
    const unsigned long long ticks = (unsigned long long)(c->wall_clock_khz * 2.0);
    HIPCHK(hipStreamSynchronize(s1));
    HIPCHK(hipStreamSynchronize(s2));
    const auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(k_pc_spin, dim3(1), dim3(64), 0, s1, ticks);
    hipLaunchKernelGGL(k_pc_spin, dim3(1), dim3(64), 0, s2, ticks);
    HIPCHK(hipStreamSynchronize(s1));
    HIPCHK(hipStreamSynchronize(s2));
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *yes = ms < 3.2;
    return PSDR_OK;
}
int pc_pick_streams(psdr_ctx *c) {
    constexpr int NC = 6;
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    Stream cand[NC];  // (the three chosen are moved into the context at the end; the others, or all on an error path, die here)
    double gap[NC] = {};
    for (Stream &st : cand) PSDRCHK(st.create(hi));
    hipLaunchKernelGGL(k_pc_nop, dim3(1), dim3(64), 0, c->stream);  // (code objects loaded, queues created)
    if (c->side != c->stream) hipLaunchKernelGGL(k_pc_nop, dim3(1), dim3(64), 0, c->side);
    for (hipStream_t st : cand) hipLaunchKernelGGL(k_pc_spin, dim3(1), dim3(64), 0, st, 1ull);
    HIPCHK(hipDeviceSynchronize());
    int order[NC];
    double gside[NC] = {}, score[NC] = {};
    for (int i = 0; i < NC; i++) {  // (the better of two readings each: beside the main stream, beside the side stream)
        double g1 = 0, g2 = 0, g3 = 0, g4 = 0;
        int rc = pc_launch_gap_us(c, cand[i], c->stream, &g1);
        if (!rc) rc = pc_launch_gap_us(c, cand[i], c->stream, &g2);
        if (!rc && c->side != c->stream) rc = pc_launch_gap_us(c, cand[i], c->side, &g3);
        if (!rc && c->side != c->stream) rc = pc_launch_gap_us(c, cand[i], c->side, &g4);
        if (rc) return rc;
        gap[i] = std::min(g1, g2);
        gside[i] = std::min(g3, g4);
        order[i] = i;
    }
    {
        const double m0 = std::max(*std::min_element(gap, gap + NC), 0.1), m1 = std::max(*std::min_element(gside, gside + NC), 0.1);
        for (int i = 0; i < NC; i++) score[i] = std::max(gap[i] / m0, c->side != c->stream ? gside[i] / m1 : 0.0);
    }
    std::stable_sort(order, order + NC, [&](int x, int y) { return score[x] < score[y]; });
    // The moving averages' stream: the quietest candidate (beside both).  The gain's stream: one that is quiet beside the
    // MAIN stream but shares the side stream's pipe, if there is one - two chain streams on the same quiet pipe measured
    // +46 % with 256 clients, quiet + side's pipe +14-16 % (five runs; the first context of a process gets that by itself) -
    // else the next quietest.  Either must run side by side with the other and with the side stream.
    auto beside = [&](int i, int j, bool *ok) -> int {  // j < 0: the side stream
        *ok = true;
        if (j < 0 && c->side == c->stream) return PSDR_OK;
        return pc_side_by_side(c, cand[i], j < 0 ? c->side : cand[j], ok);
    };
    int first = -1, second = -1;
    for (int k = 0; k < NC && first < 0; k++) {
        bool ok = true;
        int rc = beside(order[k], -1, &ok);
        if (rc) return rc;
        if (ok) first = order[k];
    }
    if (first < 0) first = order[0];
    const double m0 = std::max(*std::min_element(gap, gap + NC), 0.1), m1 = std::max(*std::min_element(gside, gside + NC), 0.1);
    for (int pass = 0; pass < 2 && second < 0; pass++)
        for (int k = 0; k < NC && second < 0; k++) {
            const int i = order[k];
            if (i == first) continue;
            const bool quiet_main = gap[i] < 1.6 * m0, on_side_pipe = c->side != c->stream && gside[i] > 1.6 * m1;
            if (pass == 0 && !(quiet_main && on_side_pipe)) continue;
            bool ok = true, ok2 = true;
            int rc = beside(i, first, &ok);
            if (!rc) rc = beside(i, -1, &ok2);
            if (rc) return rc;
            if (ok && ok2) second = i;
        }
    if (second < 0) second = order[0] == first ? order[1] : order[0];
    int third = -1;
    for (int k = 0; k < NC; k++)
        if (order[k] != first && order[k] != second) {
            third = order[k];
            break;
        }
    if (psdr_tuning_env("PSDR_PC_VERBOSE")) {
        fprintf(stderr, "psdr post chain: launch gap of the main / side stream beside each candidate stream [us]:");
        for (int i = 0; i < NC; i++) fprintf(stderr, " %.1f/%.1f", gap[i], gside[i]);
        fprintf(stderr, " -> streams %d and %d\n", first, second);
    }
    c->pc_s[0] = std::move(cand[first]);
    c->pc_s[2] = std::move(cand[second]);
    c->pc_s[1] = std::move(cand[third]);
    return PSDR_OK;
}
}  // namespace

// the tuning overrides of a tuning build (ctx.h psdr_tuning_env: nothing is read by the library that ships), once per resolve
static PcKnobs pc_knobs() {
    PcKnobs k;
    auto num = [](const char *name, int *v) {
        if (const char *e = psdr_tuning_env(name)) *v = atoi(e);
    };
    num("PSDR_PC_LANES", &k.lanes);
    num("PSDR_PC_RESERVE", &k.reserve);
    num("PSDR_PC_OWN", &k.own);
    num("PSDR_PC_FUSED", &k.fused);
    num("PSDR_PC_CMW", &k.cmw);
    num("PSDR_PC_DIRECT", &k.direct);
    num("PSDR_PC_STREAMS", &k.streams);
    num("PSDR_PC_SPLIT_PEAK", &k.split_peak);
    num("PSDR_PC_PICK", &k.pick);
    if (const char *e = psdr_tuning_env("PSDR_PC_SKIP")) k.skip = (int)strtol(e, nullptr, 0);
    return k;
}
static PcPlan pc_plan_of(const psdr_ctx *c, bool piped) {
    PcFacts f;
    f.audio_rate = c->cfg.audio_rate;
    f.n = c->n;
    f.max_batch = c->max_batch;
    f.slots = (int)c->aslots.size();
    f.piped = piped;
    f.opt_pc_agc = c->opt_pc_agc, f.opt_pc_pcm16 = c->opt_pc_pcm16, f.opt_pc_streams = c->opt_pc_streams;
    return pc_resolve(f, pc_knobs());
}
// (only a context that owns its side stream pipelines the chain: with a caller's stream - group members - everything rides
// on that one stream)
void psdr::pc_replan(psdr_ctx *c) {
    c->post_plan = pc_plan_of(c, c->side != c->stream && c->pc_s[0] != nullptr);
    pc_fill_args(c->post, c->post_plan);  // (the plan is the record; the kernels' copy of its numbers is written here and nowhere else)
}

extern "C" int psdr_set_option(psdr_ctx *c, int option, int value) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    switch (option) {
    case PSDR_OPT_POST_CHAIN_STREAMS:
        if (value != 0 && value != 1) return fail(PSDR_ERR_INVALID, "PSDR_OPT_POST_CHAIN_STREAMS: 0 (creation order) or 1 (measured), not %d", value);
        if (c->post_ready) return fail(PSDR_ERR_STATE, "PSDR_OPT_POST_CHAIN_STREAMS after the post chain was set up");
        c->opt_pc_streams = value;
        return PSDR_OK;
    case PSDR_OPT_POST_CHAIN_PCM16: {
        if (value != 0 && value != 1) return fail(PSDR_ERR_INVALID, "PSDR_OPT_POST_CHAIN_PCM16: 0 (int32 rows, the reference's buffer) or 1 (int16 rows), not %d", value);
        HIPCHK(hipSetDevice(c->device));
        const int rc = drain(c);
        if (rc) return rc;
        c->opt_pc_pcm16 = value;
        if (c->post_ready) pc_replan(c);
        return PSDR_OK;
    }
    case PSDR_OPT_POST_CHAIN_AGC: {
        if (value != 0 && value != 1) return fail(PSDR_ERR_INVALID, "PSDR_OPT_POST_CHAIN_AGC: 0 (five kernels) or 1 (one kernel behind chunk maxima), not %d", value);
        HIPCHK(hipSetDevice(c->device));
        const int rc = drain(c);
        if (rc) return rc;
        c->opt_pc_agc = value;
        if (c->post_ready) pc_replan(c);
        return PSDR_OK;
    }
    case PSDR_OPT_WATERFALL_DETECTOR:
        return set_wf_default_detector(c, value);
    case PSDR_OPT_FINE_TUNE: {
        if (value != 0 && value != 1) return fail(PSDR_ERR_INVALID, "PSDR_OPT_FINE_TUNE: 0 or 1, not %d", value);
        std::lock_guard<std::mutex> lk(c->mtx);
        c->opt_fine_tune = value;
        return PSDR_OK;
    }
    case PSDR_OPT_SAM_SIDEBAND: {
        if (value < PSDR_SAM_BOTH || value > PSDR_SAM_LOWER) return fail(PSDR_ERR_INVALID, "PSDR_OPT_SAM_SIDEBAND: a psdr_sam_sideband, not %d", value);
        std::lock_guard<std::mutex> lk(c->mtx);
        c->opt_sam_sideband = value;
        return PSDR_OK;
    }
    case PSDR_OPT_AUTO_NOTCH: {
        if (value != 0 && value != 1) return fail(PSDR_ERR_INVALID, "PSDR_OPT_AUTO_NOTCH: 0 or 1, not %d", value);
        std::lock_guard<std::mutex> lk(c->mtx);
        c->opt_auto_notch = value;
        return PSDR_OK;
    }
    case PSDR_OPT_NOISE_REDUCTION: {
        if (value < 0 || value > PSDR_NR_STRONG) return fail(PSDR_ERR_INVALID, "PSDR_OPT_NOISE_REDUCTION: 0 or a PSDR_NR_* preset, not %d", value);
        if (value && c->cfg.audio_rate <= 0) return fail(PSDR_ERR_STATE, "noise reduction: the context's audio_rate %d is not positive", c->cfg.audio_rate);
        std::lock_guard<std::mutex> lk(c->mtx);
        c->opt_nr = value;
        return PSDR_OK;
    }
    case PSDR_OPT_AUDIO_BLANKER: {
        if (value < 0 || value > PSDR_ANB_STRONG) return fail(PSDR_ERR_INVALID, "PSDR_OPT_AUDIO_BLANKER: 0 or a PSDR_ANB_* preset, not %d", value);
        std::lock_guard<std::mutex> lk(c->mtx);
        c->opt_anb = value;
        return PSDR_OK;
    }
    default:
        return fail(PSDR_ERR_INVALID, "unknown option %d", option);
    }
}
extern "C" int psdr_set_post_chain(psdr_ctx *c, int enable) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (c->n <= 0) return fail(PSDR_ERR_STATE, "context created with audio_fft_size 0");
    HIPCHK(hipSetDevice(c->device));
    {
        int rc = drain(c);
        if (rc) return rc;
    }
    if (!enable) {
        c->post_on = false;
        return PSDR_OK;
    }
    if (!c->post_ready) {
        // (one-time set-up, built in locals and moved into the context only when EVERY allocation and the stream choice went
        // through: a failure half-way leaves the context as it was, and a retry starts from scratch)
        const int rate = c->cfg.audio_rate;
        const PcPlan p = pc_plan_of(c, c->side != c->stream);
        if (p.verdict == PC_RATE_TOO_SMALL) return fail(PSDR_ERR_INVALID, "audio_rate %d too small for the DC blocker", rate);
        if (p.verdict == PC_NO_FRAME) return fail(PSDR_ERR_STATE, "audio_fft_size %d: no samples in a frame", c->n);
        if (p.verdict != PC_OK) return fail(PSDR_ERR_UNSUPPORTED, "audio_rate %d: DC delay %d / look-ahead %d unsupported", rate, p.D, p.L);
        PostArgs a{};
        psdr_ctx::PostChain pc;
        const size_t S = c->aslots.size(), Tm = p.Tm;
        a.max_batch = c->max_batch;
        a.slots = (int)S;
        const size_t S64 = (S + 63) / 64 * 64;  // (a block of 64 slots is allocated whole)
        int rc = 0;
        for (int i = 0; i < psdr_ctx::PC_SETS && !rc; i++) {
            rc = pc.fstart[i].alloc(S * c->max_batch, true);
            if (!rc) rc = pc.len[i].alloc(S, true);
            if (!rc) rc = pc.x[i].alloc(p.px * S64, true);
            if (!rc) rc = pc.m1[i].alloc(p.px * S64, true);
            if (!rc) rc = pc.v1[i].alloc(p.pv * S64, true);
            if (!rc) rc = pc.p[i].alloc(p.pv * S64, true);
            if (!rc) rc = pc.s[i].alloc(p.pv * S64, true);
            if (!rc) rc = pc.sm[i].alloc(S64 * pc_nblk(p.L, Tm) * p.nsub, true);
            if (p.agc_ok) {
                if (!rc) rc = pc.cm[i].alloc(S64 * p.nch, true);
                if (!rc) rc = pc.cp[i].alloc(S64 * p.nch, true);
                if (!rc) rc = pc.cs[i].alloc(S64 * p.nch, true);
                if (!rc) rc = pc.falive[i].alloc(S64 * c->max_batch, true);
            }
            for (auto &stage : pc.ev)
                if (!rc) rc = stage[i].create();
        }
        for (int k = 0; k < 2 && !rc; k++) rc = pc.pcm_pool[k].alloc(S * Tm, true);
        if (!rc) rc = pc.pcm_dump.alloc(64 * (1 + PC_AGC_NP) * 16 / sizeof(int32_t), true);
        if (!rc) rc = pc.dc_s1.alloc(S, true);
        if (!rc) rc = pc.dc_s2.alloc(S, true);
        if (!rc) rc = pc.agc_gain.alloc(S, true);
        if (!rc) rc = pc.agc_n0.alloc(S, true);
        if (rc) {
            const std::string msg = psdr_last_error();
            return fail(rc == PSDR_ERR_HIP ? PSDR_ERR_NOMEM : rc, "post chain set-up: %s", msg.c_str());
        }
        a.pcm = pc.pcm_pool[0];
        a.pcm_dump = pc.pcm_dump, a.dc_s1 = pc.dc_s1, a.dc_s2 = pc.dc_s2, a.agc_gain = pc.agc_gain, a.agc_n0 = pc.agc_n0;
        // The chain's streams (a pipelined chain only: with a caller's stream no chain stream is made).
        // PSDR_OPT_POST_CHAIN_STREAMS (PcPlan::pick_streams):
        //   0 (default)  three streams in creation order, the first and the third used: deterministic; the FIRST context of a
        //                process gets the quiet queues by itself
        //   1 (opt-in)   chosen by measurement (pc_pick_streams: ~60 ms, wall-clock thresholds): what a process that creates
        //                several contexts (bench.py's sub-workloads) needs to see +3 % instead of +15 %; a measurement that
        //                fails falls back to creation order instead of failing the call
        if (!c->pc_s[0] && c->side != c->stream) {
            if (p.pick_streams) (void)pc_pick_streams(c);  // (sets pc_s only when the whole measurement went through)
            if (!c->pc_s[0]) {
                int lo = 0, hi = 0;
                Stream s3[3];
                if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess || s3[0].create(hi) || s3[1].create(hi) || s3[2].create(hi))
                    return fail(PSDR_ERR_HIP, "post chain: stream creation failed");
                for (int i = 0; i < 3; i++) c->pc_s[i] = std::move(s3[i]);
            }
        }
        c->pc = std::move(pc);
        c->post = a;
        c->post_ready = true;
    }
    pc_replan(c);
    c->post_on = true;
    return PSDR_OK;
}

// the gain the client's last chain batch left behind (the one its next batch starts from, unless a mode change resets it)
extern "C" int psdr_read_agc_gain(psdr_ctx *c, int id, float *gain) {
    if (!c || !gain) return fail(PSDR_ERR_INVALID, "null argument");
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        PSDRCHK(check_slot(c, id));
        if (!c->post_ready) return fail(PSDR_ERR_STATE, "post chain not set up (psdr_set_post_chain)");
        // (agc_reset 2: a fresh client no chain batch has listed yet - the slot holds its previous occupant's gain)
        if (c->aslots[id].agc_reset == 2) return fail(PSDR_ERR_NO_DATA, "client %d has not been part of a post chain batch", id);
    }
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    HIPCHK(hipMemcpy(gain, c->pc.agc_gain + id, sizeof(float), hipMemcpyDeviceToHost));
    return PSDR_OK;
}

// run-time booleans -> template arguments: f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...)
template <typename F>
static auto pc_with_bools(F &&f) {
    return f();
}
template <typename F, typename... B>
static auto pc_with_bools(F &&f, bool b, B... rest) {
    if (b) return pc_with_bools([&](auto... c) { return f(std::true_type{}, c...); }, rest...);
    return pc_with_bools([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

// the chain's kernels for the batch whose demodulation has just been enqueued on c->side (d_clients: its parameter
// block - the nact active clients first, then npaused paused ones with an empty stream - and d_slot_ci: the list index of
// every slot's client, -1 = not listed).  What is launched, where and with how much LDS is c->post_plan's business
// (postplan.h); only what depends on nframes is worked out here.
int psdr::post_chain_enqueue(psdr_ctx *c, const ClientParams *d_clients, const int *d_slot_ci, int nact, int npaused, int nframes,
                             const int *d_drop, const AgcEntry *d_agc, hipStream_t *last_user) {
    constexpr int NS = psdr_ctx::PC_SETS;
    const PcPlan &p = c->post_plan;
    const int set = (int)(c->chain_seq % NS), nxt = (set + 1) % NS;
    const uint64_t seq = c->chain_seq;
    const bool piped = p.s_ma >= 0;
    auto stream_of = [&](int i) -> hipStream_t { return i < 0 ? c->side : (hipStream_t)c->pc_s[i]; };
    const hipStream_t sg = c->side, sm = stream_of(p.s_ma), sc = stream_of(p.s_gain), sp = stream_of(p.s_peak);
    // this batch's PCM goes to the other of two buffers (the copy of the last batch's to the host may still read its own)
    c->pcm_set ^= 1;
    c->post.pcm = c->pc.pcm_pool[c->pcm_set];
    PostArgs pa = c->post;
    c->pcm_is16 = p.pcm16;
    pa.audio = c->d_audio;  // (of THIS demodulation batch: the result sets alternate)
    pa.nan_flags = d_drop;  // (c->d_nan itself unless the batch has squelch clients: demod.hip)
    pa.clients = d_clients;
    pa.slot_ci = d_slot_ci;
    pa.nact = nact + npaused;
    pa.nframes = nframes;
    pa.X = c->pc.x[set], pa.Xn = c->pc.x[nxt];
    pa.M1 = c->pc.m1[set], pa.M1n = c->pc.m1[nxt];
    pa.V1 = c->pc.v1[set], pa.V1n = c->pc.v1[nxt];
    pa.P = c->pc.p[set];
    pa.S = c->pc.s[set];
    pa.SM = c->pc.sm[set];
    pa.fstart = c->pc.fstart[set];
    pa.len = c->pc.len[set];
    pa.CM = c->pc.cm[set], pa.CP = c->pc.cp[set], pa.CS = c->pc.cs[set];
    pa.falive = c->pc.falive[set];
    // the batch's AGC profiles: with a table the kernels that form w and step the gain are the forms with profiles (k_pc_want_prof, PcWithProfiles), which read each
    // lane's entry once; without one the batch gets the kernels it always got
    pa.agc_tab = c->post.agc_tab = d_agc;
    const bool prof = d_agc != nullptr;
    c->post_direct = p.direct;
    const int nall = nact + npaused, skip = p.skip;
    const unsigned groups = p.groups, rgroups = p.rgroups;
    const size_t Tb = (size_t)nframes * pa.h;  // longest possible stream of this batch
    const unsigned nblk = (unsigned)pc_nblk(pa.L, Tb);
    // Who touched what last (sets rotate: batch b uses set b mod 3 and writes the history rows of set b + 1):
    //   X[set] rows >= D, fstart / len[set]   gather(b)      <- moving averages, history, output of batch b - 3
    //   V1[set] rows >= L-1                   averages(b)    <- peak / output of batch b - 3
    //   X / M1 / V1[nxt] history rows         history(b)     <- averages(b - 2) (same stream), peak / output of batch b - 2
    //   P / S / SM[set]                       peak(b)        <- gain / output of batch b - 3
    //   CM / CP / CS[set] (one-kernel AGC)    averages(b) [CMW], chunk maxima / scans(b) on the averages' stream  <- k_pc_agc of batch b - 3
    //   falive[set]                           index(b)       <- k_pc_agc of batch b - 3
    //   d_audio[b mod 2] (DIRECT)             demodulation(b) <- averages / history of batch b - 2 (the wait is in demod.hip)
    // i.e. a stage waits for its predecessor of THIS batch and for the output stage of the batch that had the set.
    auto wait = [&](hipStream_t st, int stage, int which) -> int {
        if (piped) HIPCHK(hipStreamWaitEvent(st, c->pc.ev[stage][which], 0));
        return PSDR_OK;
    };
    auto done = [&](hipStream_t st, int stage) -> int {
        if (piped) HIPCHK(hipEventRecord(c->pc.ev[stage][set], st));
        return PSDR_OK;
    };
    int rc = 0;
    {  // ---- stage 0: frame offsets, audio rows -> X
        if (seq >= NS && ((rc = wait(sg, 1, set)) || (rc = wait(sg, 3, set)))) return rc;
        ProfScope ps(c, K_POST, sg);
        hipLaunchKernelGGL(k_pc_index, dim3(nall), dim3(64), 0, sg, pa);
        if (skip & 1)
            ;
        else if (p.rows4)
            hipLaunchKernelGGL(k_pc_gather4, dim3(groups, nframes), dim3(256), 0, sg, pa);
        else
            hipLaunchKernelGGL(k_pc_gather, dim3(nall, nframes), dim3(256), 0, sg, pa);
        HIPCHK(hipGetLastError());
        if ((rc = done(sg, 0))) return rc;
    }
    {  // ---- stage 1: the DC blocker's two moving averages (sequential), tails -> the next set's history rows
        if ((rc = wait(sm, 0, set))) return rc;
        if (seq >= NS && (rc = wait(sm, 3, set))) return rc;
        if (seq >= NS - 1 && (rc = wait(sm, 3, nxt))) return rc;
        ProfScope ps(c, K_POST, sm);
        if (skip & 2) {
        } else if (p.ma == MA2_CMW) {
            hipLaunchKernelGGL((k_pc_ma2<true, true>), dim3(rgroups), dim3(192), 0, sm, pa);
        } else if (p.ma == MA2) {
            pc_with_bools([&](auto own) { hipLaunchKernelGGL(k_pc_ma2<decltype(own)::value>, dim3(rgroups), dim3(128), p.ma_lds, sm, pa); }, p.own);
        } else if (p.ma == MAD) {
            rc = pc_with_bools(
                [&](auto own) -> int {
                    const void *fn = (const void *)k_pc_mad<decltype(own)::value>;
                    if (c->lds_attr_done.insert(fn).second) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024));
                    hipLaunchKernelGGL(k_pc_mad<decltype(own)::value>, dim3(rgroups), dim3(128), p.ma_lds, sm, pa);
                    return PSDR_OK;
                },
                p.own);
            if (rc) return rc;
        } else {
            pc_with_bools(
                [&](auto pow2) {
                    hipLaunchKernelGGL((k_pc_ma<false, decltype(pow2)::value>), dim3(groups), dim3(64), 0, sm, pa);
                    hipLaunchKernelGGL((k_pc_ma<true, decltype(pow2)::value>), dim3(groups), dim3(64), 0, sm, pa);
                },
                p.ma == MA_POW2);
        }
        if (!(skip & 4)) hipLaunchKernelGGL(k_pc_history, dim3(nall), dim3(256), 0, sm, pa);
        HIPCHK(hipGetLastError());
        if ((rc = done(sm, 1))) return rc;
    }
    if (p.agc == AGC_ONE_KERNEL) {
        // ---- stage 2: chunk maxima of |V1| and their block scans, behind the moving averages on THEIR stream (P / S / SM are not
        // used; CM / CP / CS of this set were last read by stage 3 of batch b - 3: waited for in stage 1)
        const int nchunks = (int)((pa.vo + pa.L - 1 + Tb + 15) / 16);
        const int W = pa.L / 16 - 1;
        {
            ProfScope ps(c, K_POST, sm);
            const int ncm = p.ma == MA2_CMW ? pa.L / 16 : nchunks;  // (k_pc_ma2 CMW left the new samples' chunk maxima: the history chunks only)
            if (!(skip & 8)) hipLaunchKernelGGL(k_pc_cm, dim3(groups, (ncm + 15) / 16), dim3(64), 0, sm, pa, ncm);
            if (!(skip & 16)) hipLaunchKernelGGL(k_pc_cscan, dim3(groups, (nchunks + W - 1) / W), dim3(64), 0, sm, pa, nchunks, W);
            HIPCHK(hipGetLastError());
        }
        if (sm != sc && ((rc = done(sm, 2)) || (rc = wait(sc, 2, set)))) return rc;
        // ---- stage 3: w_t, the gain recurrence, int16 - one kernel
        ProfScope ps(c, K_POST, sc);
        if ((rc = fetch_guard_wait(c, sc, c->guard_pcm[c->pcm_set]))) return rc;  // what read this PCM buffer two batches ago has landed
        c->guard_pcm[c->pcm_set] = nullptr;
        if (!(skip & 128)) hipLaunchKernelGGL(k_pc_zero, dim3(groups, nframes), dim3(256), 0, sc, pa);
        if (!(skip & 64))
            pc_with_bools(
                [&](auto att, auto p16, auto pr) {
                    if constexpr (decltype(pr)::value)
                        hipLaunchKernelGGL((k_pc_agc<decltype(att)::value, decltype(p16)::value, PcWithProfiles>), dim3(rgroups), dim3(64 * (1 + PC_AGC_NP)), 0, sc, pa);
                    else
                        hipLaunchKernelGGL((k_pc_agc<decltype(att)::value, decltype(p16)::value>), dim3(rgroups), dim3(64 * (1 + PC_AGC_NP)), 0, sc, pa);
                },
                p.att_faster, p.pcm16, prof);
        HIPCHK(hipGetLastError());
        if ((rc = done(sc, 3))) return rc;
    } else {
        {  // ---- stage 2: look-ahead peak and w_t (parallel along time)
            hipStream_t sp1 = p.split_peak ? sm : sp;  // (P[set]'s last readers - gain / output of batch b - 3 - were waited for in stage 1)
            if (sp1 != sm && (rc = wait(sp1, 1, set))) return rc;
            if (seq >= NS && sp1 != sm && (rc = wait(sp1, 3, set))) return rc;
            {
                ProfScope ps(c, K_POST, sp1);
                if (pa.nsub > 1 && !(skip & 8)) hipLaunchKernelGGL(k_pc_submax, dim3(groups, nblk * pa.nsub), dim3(64), 0, sp1, pa);
                if (!(skip & 16)) hipLaunchKernelGGL(k_pc_prefix, dim3(groups, nblk * pa.nsub), dim3(64), 0, sp1, pa);
            }
            if (p.split_peak) {
                if ((rc = done(sp1, 2)) || (rc = wait(sp, 2, set))) return rc;
            }
            {
                ProfScope ps(c, K_POST, sp);
                if (!(skip & 32)) hipLaunchKernelGGL(prof ? k_pc_want_prof : k_pc_want, dim3(groups, nblk * pa.nsub), dim3(64), 0, sp, pa);
            }
            HIPCHK(hipGetLastError());
            if (!p.split_peak && (rc = done(sp, 2))) return rc;
        }
        {  // ---- stage 3: the gain recurrence (sequential), int16 output
            if (sp != sc && (rc = wait(sc, 2, set))) return rc;
            ProfScope ps(c, K_POST, sc);
            if (!(skip & 64))
                pc_with_bools(
                    [&](auto att, auto own, auto pr) {
                        if constexpr (decltype(pr)::value)
                            hipLaunchKernelGGL((k_pc_gain<decltype(att)::value, decltype(own)::value, PcWithProfiles>), dim3(rgroups), dim3(128), p.gain_lds, sc, pa);
                        else
                            hipLaunchKernelGGL((k_pc_gain<decltype(att)::value, decltype(own)::value>), dim3(rgroups), dim3(128), p.gain_lds, sc, pa);
                    },
                    p.att_faster, p.own, prof);
            if ((rc = fetch_guard_wait(c, sc, c->guard_pcm[c->pcm_set]))) return rc;  // what read this PCM buffer two batches ago has landed
            c->guard_pcm[c->pcm_set] = nullptr;
            if (skip & 128)
                ;
            else if (p.rows4)
                hipLaunchKernelGGL(k_pc_out4, dim3(groups, nframes), dim3(256), 0, sc, pa);
            else
                hipLaunchKernelGGL(k_pc_out, dim3(nall, nframes), dim3(256), 0, sc, pa);
            HIPCHK(hipGetLastError());
            if ((rc = done(sc, 3))) return rc;
        }
    }
    if (piped) c->chain_pending = true;
    c->chain_seq++;
    *last_user = sc;
    return PSDR_OK;
}

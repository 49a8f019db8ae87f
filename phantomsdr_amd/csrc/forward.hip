// forward.hip - the frame loop of broadcast_server::fft_task (src/fft.cpp:47-105) for a batch of frames: the two FFT
// passes, the pyramid levels above the tile (seam, column tail, pyramid tail), then what reads a finished batch without
// demodulating it: spectrum / pyramid read-back in the reference's order, the band layout of multi-GPU sharding and
// the waterfall clients (src/waterfall.cpp, src/websocket.cpp:207-236).
#include "ctx.h"
#include "epilogue.h"
#include "fft_pass.h"

namespace psdr {

// stamp slot of the next launch of pass `which` (nullptr: mode 2 off or the ring is full)
static unsigned long long *next_kclk(psdr_ctx *c, int which) {
    if (!c->kclock || !c->d_kclk || c->kclk_pos[which] >= psdr_ctx::KCLK_SLOTS) return nullptr;
    return c->d_kclk + ((size_t)which * psdr_ctx::KCLK_SLOTS + c->kclk_pos[which]++) * 2;
}
// counters for the next launch of pass `which` on stream st
static int next_tickets(psdr_ctx *c, int which, hipStream_t st, unsigned **out) {
    unsigned &pos = c->ticket_pos[which];
    const unsigned slot = pos % TICKET_SLOTS;
    if (slot % (TICKET_SLOTS / 2) == 0 && pos >= TICKET_SLOTS / 2) {
        // entering a half of the ring: its counters were last used TICKET_SLOTS/2 launches ago on
        // this same stream, so clearing them here is ordered after those launches
        HIPCHK(hipMemsetAsync(c->d_tickets[which] + (size_t)slot * 8, 0, (TICKET_SLOTS / 2) * 8 * sizeof(unsigned), st));
    }
    *out = c->d_tickets[which] + (size_t)slot * 8;
    pos++;
    return PSDR_OK;
}
static_assert(SEG_CARRY_MEM == PSDR_SEG_CARRY_MEM, "forwardplan.h writes the flag fft_pass.h reads");
// the chain segments of a batch of nframes frames (forwardplan.h): planned, checked against what the seam buffers hold and
// uploaded on first use of a batch size
int seg_plan(psdr_ctx *c, int nframes, const psdr_ctx::SegPlan **out) {
    for (const auto &sp : c->seg_plans)
        if (sp.nframes == nframes) {
            *out = &sp;
            return PSDR_OK;
        }
    psdr_ctx::SegPlan sp;
    sp.nframes = nframes;
    sp.nsegs = seg_count(c->seg_facts, nframes);
    sp.handoff = seg_handoff(c->seg_facts, nframes);
    if (sp.nsegs > c->seg_cap) return fail(PSDR_ERR_STATE, "seam buffers too small (%u segments, %zu allocated)", sp.nsegs, c->seg_cap);
    std::vector<SegEntry> tab(sp.nsegs);
    seg_table(c->seg_facts, nframes, tab.data());
    PSDRCHK(sp.d_tab.alloc(tab.size()));
    HIPCHK(hipMemcpy(sp.d_tab, tab.data(), tab.size() * sizeof(SegEntry), hipMemcpyHostToDevice));  // (once per batch size)
    c->seg_plans.push_back(std::move(sp));
    *out = &c->seg_plans.back();
    return PSDR_OK;
}
void select_set(psdr_ctx *c, int set) {
    c->cur_set = set;
    c->d_spec = c->spec_pool[set];
    c->d_q = c->q_pool[set];
    c->d_qt = c->qt_pool[set];
    c->d_pscr[0] = c->pscr_pool[set][0];
    c->d_pscr[1] = c->pscr_pool[set][1];
    c->d_seamP = c->seam_pool[set][0];
    c->d_seamC = c->seam_pool[set][1];
}

// the pyramid levels above the tile for the batch process_frames has just transformed, on the side stream
static int enqueue_tails(psdr_ctx *c) {
    c->tails_pending = false;
    const psdr_ctx::SegPlan *plan = c->tails_plan;
    const int nframes = c->tails_nframes;
    if (plan) {  // fused real input: the mirror octets of the first tile of every chain segment without a carry-in (epilogue.h)
        SeamArgs sa{};
        sa.seamP = c->d_seamP;
        sa.seamC = c->d_seamC;
        sa.segtab = plan->d_tab;
        sa.segmark = c->d_segflag + (size_t)(1 + c->cur_set) * c->seg_cap;
        sa.epoch = c->seg_epoch;
        sa.L = c->M2;
        sa.cp = c->T2 / 2;
        sa.size_log2 = c->size_log2;
        sa.Qt = c->d_qt;
        sa.qt_stride = c->qt_stride;
        sa.Pscr = c->d_pscr[0];
        sa.p_stride = c->p_stride;
        ProfScope ps(c, K_SEAM, c->side);
        hipLaunchKernelGGL(k_real_seam, dim3(plan->nsegs), dim3(256), 0, c->side, sa);
        HIPCHK(hipGetLastError());
    }
    // remaining pyramid levels from the partial level in scratch: the steps psdr_create planned (forwardplan.h: tails_plan)
    for (int i = 0; i < c->tails.n; i++) {
        const TailStep &st = c->tails.step[i];
        ProfScope ps(c, K_TAIL, c->side);
        if (st.kind == TAIL_GENERIC) {
            TailArgs t{};
            t.Pin = c->d_pscr[st.src];
            t.in_stride = c->p_stride;
            t.len_in = st.len_in;
            t.lvl_in = st.lvl_in;
            t.nlevels = c->levels;
            t.size_log2 = c->size_log2;
            t.Q = c->d_q;
            t.q_stride = c->q_stride;
            t.R = c->R;
            t.Pout = c->d_pscr[st.dst];
            t.out_stride = c->p_stride;
            t.map = c->recmap;
            if (!st.mapped) t.map.mapped = 0;  // only pass 2's own output is tile-major
            const unsigned nb = (unsigned)((st.len_in / 2 + 255) / 256);
            hipLaunchKernelGGL(k_pyramid_tail, dim3(nb, nframes), dim3(256), 0, c->side, t);
        } else {
            ColTailArgs t{};
            t.Pin = c->d_pscr[st.src];
            t.in_stride = c->p_stride;
            t.mode = c->recmap.mapped;
            t.L = c->M2;
            t.l2L = c->log2M2;
            t.lvl_in = st.lvl_in;
            t.nlevels = c->levels;
            t.size_log2 = c->size_log2;
            t.Q = c->d_q;
            t.q_stride = c->q_stride;
            t.R = c->R;
            t.Pout = c->d_pscr[st.dst];
            t.out_stride = c->p_stride;
            const dim3 grid((unsigned)(c->M2 / 64), (unsigned)nframes);
            switch (st.kind) {
            case TAIL_COL_64:
                hipLaunchKernelGGL(k_col_tail<64>, grid, dim3(64), 0, c->side, t);
                break;
            case TAIL_COL_128:
                hipLaunchKernelGGL(k_col_tail<128>, grid, dim3(64), 0, c->side, t);
                break;
            case TAIL_COL_256_PAIRED:
                hipLaunchKernelGGL((k_col_tail<256, true>), grid, dim3(64), 0, c->side, t);
                break;
            default:
                hipLaunchKernelGGL(k_col_tail<256>, grid, dim3(64), 0, c->side, t);
            }
        }
        HIPCHK(hipGetLastError());
    }
    return side_done(c);
}

// forward FFT + power + int8 pyramid for nframes frames (src/fft.cpp:61-98 per frame)
int process_frames(psdr_ctx *c, const void *d_halves, int nframes, int fmt, hipEvent_t ev_raw_consumed) {
    // alternate the result set when the consumers run on their own stream
    // (banded spectrum: also on a caller's stream - the regions of batch b are read by the peers, asynchronously,
    // while batch b+1 is transformed)
    if (c->side != c->stream || c->nbands || c->alt_sets) select_set(c, c->cur_set ^ 1);
    const int sb = fmt <= PSDR_FMT_S8 ? 2 : (fmt <= PSDR_FMT_S16 ? 4 : 8);  // image bytes per sample
    const unsigned tiles1 = (unsigned)(c->M2 / c->T1), tiles2 = (unsigned)(c->M1 / c->T2);
    c->input_on_main = false;
    cf *Y = c->d_Y;
    Pass1Args a1{};
    a1.raw = d_halves;
    a1.Y = Y;
    a1.Wl = c->d_Wl1;
    a1.TB = c->d_TB;
    a1.yblk = (size_t)c->M1 * c->T1;  // plain: one linear block per pass-1 tile
    a1.l2t2 = ilog2((size_t)c->T2);
    // fused real: pass-2-tile-major (fft_pass.h, "Y layout")
    a1.ytile = (size_t)c->M2 * c->T2;
    a1.ytl = (size_t)c->T2 * c->T1;
    a1.yframe = c->M;
    a1.wdelta = c->wdelta;
    a1.M2 = c->M2;
    a1.log2M2 = c->log2M2;
    a1.fmt = fmt;
    a1.is_real = c->is_real ? 1 : 0;
    a1.rot = c->is_real ? 0 : 1;
    a1.trace = c->d_trace;
    a1.kclk = next_kclk(c, 0);
    a1.ymask = ~0u;
    // /N (src/fft_impl.cpp:29-31) - and the real untangle's 1/2 - as a power of two in the window weights: the fused
    // second passes store what their last stage leaves; the three-pass real path scales in k_untangle_real as before
    a1.yscale = !c->is_real ? 1.0f / (float)c->N : (c->real_fused ? 0.5f / (float)c->N : 1.0f);
    // (tuning builds only: a timing-only experiment with WRONG results - all frames of a launch share a few frames of Y)
    if (const char *e = psdr_tuning_env("PSDR_Y_ALIAS")) a1.ymask = (unsigned)atoi(e) - 1u;
    {
        int rc = next_tickets(c, 0, c->stream, &a1.tickets);
        if (rc) return rc;
    }
    a1.tiles_per_frame = tiles1;
    a1.total_slots = tiles1 * (unsigned)nframes;
    int rc = launch_pass1(c, c->M1, c->T1, sb, a1, a1.total_slots, c->real_fused);
    if (rc) return rc;
    if (ev_raw_consumed) HIPCHK(hipEventRecord(ev_raw_consumed, c->stream));  // pass 1 is the only reader of the raw halves

    Pass2Args a2{};
    a2.Y = Y;
    a2.Wl = c->d_Wl2;
    a2.M1 = c->M1;
    a2.log2M1 = c->log2M1;
    a2.TW = c->T1;
    a2.yblk = a1.yblk;
    a2.ytile = a1.ytile;
    a2.yjs = (size_t)c->T2 * c->T1;
    a2.yframe = a1.yframe;
    a2.log2TW = ilog2((size_t)c->T1);
    a2.inv_n = 1.0f / (float)c->N;
    a2.size_log2 = c->size_log2;
    a2.nlevels = c->levels;
    a2.Qt = c->d_qt;
    a2.qt_stride = c->qt_stride;
    a2.Pscr = c->d_pscr[0];
    a2.p_stride = c->p_stride;
    a2.trace = c->d_trace ? c->d_trace + 128 + 2304 : nullptr;
    a2.kclk = next_kclk(c, 1);
    a2.ymask = a1.ymask;
    {
        int rc2 = next_tickets(c, 1, c->stream, &a2.tickets);
        if (rc2) return rc2;
    }
    a2.tiles_per_frame = tiles2;
    a2.total_slots = tiles2 * (unsigned)nframes;
    // pass 2 overwrites this result set: its previous consumers (two batches ago) must be done
    if (c->set_pending[c->cur_set] && c->side != c->stream)
        HIPCHK(hipStreamWaitEvent(c->stream, c->ev_set_done[c->cur_set], 0));
    auto run_pass2 = [&](bool fused) -> int { return launch_pass2(c, c->M2, c->T2, fused, a2, a2.total_slots); };
    const psdr_ctx::SegPlan *plan = nullptr;  // fused real path: the seam kernel runs with the consumers
    if (!c->is_real) {
        a2.X = c->d_spec;
        a2.spec_stride = c->spec_stride;
        if (c->nbands) {
            a2.l2Lb = c->lay.l2Lb;
            a2.lbmask = (1 << c->lay.l2Lb) - 1;
            a2.Lw = c->lay.Lw;
            a2.band_stride = c->lay.band_stride;
            rc = launch_pass2_band(c, a2, a2.total_slots);
            if (rc) return rc;
            if (c->band_H > 0) {  // the first columns of band b+1 once more, behind band b's own
                const size_t n16 = (size_t)c->nbands * nframes * (c->M1 / 16) * c->band_H * 8;  // 16-byte pieces
                hipLaunchKernelGGL(k_band_halo, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, c->stream, c->d_spec,
                                   c->spec_stride, c->lay, c->nbands, nframes, c->M1 / 16, c->band_H);
                HIPCHK(hipGetLastError());
            }
        } else {
            rc = run_pass2(true);
            if (rc) return rc;
        }
    } else if (c->real_fused) {
        a2.X = c->d_spec;
        a2.spec_stride = c->spec_stride;
        a2.UA = c->d_UA;
        a2.UB = c->d_UB;
        a2.UG = c->d_UG;
        a2.log2UB = c->log2UB;
        rc = seg_plan(c, nframes, &plan);
        if (rc) return rc;
        a2.segtab = plan->d_tab;
        a2.seamP = c->d_seamP;
        a2.seamC = c->d_seamC;
        a2.segflag = plan->handoff ? c->d_segflag : nullptr;
        a2.segmark = c->d_segflag + (size_t)(1 + c->cur_set) * c->seg_cap;  // (of this result set, like seamP / seamC)
        if (++c->seg_epoch == 0) {  // 2^32 launches: no flag or mark of the previous cycle may look current
            HIPCHK(hipStreamSynchronize(c->stream));
            if (c->side != c->stream) HIPCHK(hipStreamSynchronize(c->side));
            HIPCHK(hipMemset(c->d_segflag, 0, 3 * c->seg_cap * sizeof(unsigned)));
            c->seg_epoch = 1;
        }
        a2.epoch = c->seg_epoch;
        a2.total_slots = plan->nsegs;
        rc = launch_pass2_real(c, a2);
        if (rc) return rc;
    } else {
        a2.X = c->d_Z;
        a2.spec_stride = c->M;
        rc = run_pass2(false);
        if (rc) return rc;
        UntangleArgs u{};
        u.Z = c->d_Z;
        u.X = c->d_spec;
        u.spec_stride = c->spec_stride;
        u.M = c->M;
        u.TA = c->d_UA;
        u.TB = c->d_UB;
        u.log2B = c->log2UB;
        u.inv_n = 1.0f / (float)c->N;
        u.size_log2 = c->size_log2;
        u.nlevels = c->levels;
        u.Q = c->d_q;
        u.q_stride = c->q_stride;
        u.Pscr = c->d_pscr[0];
        u.p_stride = c->p_stride;
        ProfScope ps(c, K_UNTANGLE);
        const unsigned nb = (unsigned)((c->M / 8 + 255) / 256);
        hipLaunchKernelGGL(k_untangle_real, dim3(nb, nframes), dim3(256), 0, c->stream, u);
        HIPCHK(hipGetLastError());
    }
    // consumers of the finished batch go to the side stream
    if (c->side != c->stream) {
        HIPCHK(hipEventRecord(c->ev_fft_done, c->stream));
        HIPCHK(hipStreamWaitEvent(c->side, c->ev_fft_done, 0));
    }
    // The pyramid levels above the tile (seam, column tail, generic tail) go FIRST on the side stream, the demodulation behind
    // them.  Round 6 measured the other order (tails enqueued behind the batch's demodulation, which then starts beside the
    // next batch's first pass) and a delayed start of all consumers (beside the next second pass): bench.py's cfg2 level,
    // cfg3 level or 1 % worse, cfg5's share 1.2 % worse - where a batch's consumers run is a zero-sum choice between the
    // two passes, what they cost is their instruction count (profiles/r06_consumer_placement.json).
    c->tails_plan = plan;
    c->tails_nframes = nframes;
    c->tails_pending = true;
    rc = enqueue_tails(c);
    if (rc) return rc;
    c->last_nframes = nframes;
    c->out_valid = c->q_valid = false;
    std::fill(c->q_untiled.begin(), c->q_untiled.end(), 0);
    return PSDR_OK;
}

}  // namespace psdr

// the level-major pyramid of `frame`, complete and at rest: behind everything enqueued, with the levels that live in tiled
// records copied out (once per frame and batch)
static int level_major_ready(psdr_ctx *c, int frame) {
    PSDRCHK(drain(c));
    if (c->tiled_lt < 0 || c->q_untiled[frame]) return PSDR_OK;
    const size_t nrec = c->R / (size_t)c->tile_ch;
    hipLaunchKernelGGL(k_untile_q, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, c->side,
                       c->d_qt + (size_t)frame * c->qt_stride, c->d_q + (size_t)frame * c->q_stride, c->R,
                       c->tile_ch, c->tiled_lt, c->levels, c->recmap);
    HIPCHK(hipGetLastError());
    c->q_untiled[frame] = 1;
    return drain(c);
}

// spectrum of `frame` to host in the reference's k order
static int copy_spectrum_k_order(psdr_ctx *c, int frame, cf *dst) {
    const cf *src = c->d_spec + (size_t)frame * c->spec_stride;
    {
        int rc = drain(c);
        if (rc) return rc;
    }
    if (c->lay.mode) {
        // the device keeps the frame in tile-major lines (SpecLayout): k order through one frame of staging
        hipLaunchKernelGGL(k_spec_k_order, dim3((unsigned)((c->M + 1 + 255) / 256)), dim3(256), 0, c->stream, src, c->d_Z,
                           c->M, c->is_real ? 1 : 0, c->lay);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(dst, c->d_Z, (c->is_real ? c->N / 2 + 1 : c->N) * sizeof(cf), hipMemcpyDeviceToHost, c->stream));
    } else if (c->is_real) {
        HIPCHK(hipMemcpyAsync(dst, src, (c->N / 2 + 1) * sizeof(cf), hipMemcpyDeviceToHost,
                              c->stream));
    } else {
        // client order c -> bin k = (c + N/2 + 1) mod N: two contiguous runs
        const size_t N = c->N, h = N / 2;
        HIPCHK(hipMemcpyAsync(dst, src + (h - 1), (h + 1) * sizeof(cf), hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipMemcpyAsync(dst + h + 1, src, (h - 1) * sizeof(cf), hipMemcpyDeviceToHost,
                              c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return PSDR_OK;
}
extern "C" int psdr_get_output_buffer(psdr_ctx *c, float **out) {
    if (!c || !out) return fail(PSDR_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(c->device));
    if (c->last_nframes > 0 && !c->out_valid) {
        int rc = copy_spectrum_k_order(c, 0, c->h_out);
        if (rc) return rc;
        if (!c->is_real && c->cfg.additional_size > 0)  // wrap copy, src/fft.cpp:91-98
            memcpy(c->h_out + c->N, c->h_out, sizeof(cf) * (size_t)c->cfg.additional_size);
        c->out_valid = true;
    }
    *out = (float *)c->h_out.get();
    return PSDR_OK;
}
extern "C" int psdr_get_quantized_buffer(psdr_ctx *c, int8_t **out) {
    if (!c || !out) return fail(PSDR_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(c->device));
    if (c->last_nframes > 0 && !c->q_valid) {
        PSDRCHK(level_major_ready(c, 0));
        HIPCHK(hipMemcpyAsync(c->h_q, c->d_q, c->q_len, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->q_valid = true;
    }
    *out = c->h_q;
    return PSDR_OK;
}
extern "C" int psdr_pack_band(psdr_ctx *c, int nframes, uint32_t first_bin, uint32_t nbins, float *d_out,
                              size_t out_stride_bins) {
    if (!c || !d_out) return fail(PSDR_ERR_INVALID, "null argument");
    if (c->last_nframes < 1) return fail(PSDR_ERR_STATE, "pack_band before process_batch/execute");
    if (nframes < 1 || nframes > c->last_nframes)
        return fail(PSDR_ERR_INVALID, "nframes %d outside [1, %d] (the last batch)", nframes, c->last_nframes);
    const uint32_t R = (uint32_t)(c->is_real ? c->N / 2 : c->N);
    if (first_bin >= R || nbins < 1 || nbins > R) return fail(PSDR_ERR_INVALID, "band [%u, +%u) outside [0, %u)", first_bin, nbins, R);
    if (out_stride_bins < nbins) return fail(PSDR_ERR_INVALID, "output stride smaller than the band");
    HIPCHK(hipSetDevice(c->device));
    ProfScope ps(c, K_BAND, c->stream);
    hipLaunchKernelGGL(k_band_pack, dim3((nbins + 255) / 256, nframes), dim3(256), 0, c->stream, c->d_spec, c->spec_stride,
                       c->lay, (int)R, (int)first_bin, (int)nbins, (cf *)d_out, out_stride_bins);
    HIPCHK(hipGetLastError());
    return PSDR_OK;
}
// ---- band sharding without the pack: pass 2 writes band regions ------------------------------------------------
extern "C" int psdr_set_band_layout(psdr_ctx *c, int nbands, uint32_t halo_bins) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    const BandPlan b = band_plan(c->shape, c->lay, nbands, halo_bins, c->max_batch);
    if (b.st.code) return fail(b.st.code, "%s", b.st.msg.c_str());
    HIPCHK(hipSetDevice(c->device));
    {
        int rc = drain(c);
        if (rc) return rc;
    }
    HIPCHK(hipDeviceSynchronize());
    {  // the new buffers first: a failed allocation leaves the context as it was
        DevBuf<cf> fresh[2];
        for (auto &f : fresh)
            if (f.alloc((size_t)nbands * b.region, true)) {
                (void)hipGetLastError();
                return fail(PSDR_ERR_NOMEM, "banded spectrum: %zu bytes per result set", (size_t)nbands * b.region * sizeof(cf));
            }
        for (int s = 0; s < 2; s++) c->spec_pool[s] = std::move(fresh[s]);
    }
    c->nbands = nbands;
    c->band_H = b.H;
    c->spec_stride = b.frame_stride;
    c->lay = b.lay;
    c->set_pending[0] = c->set_pending[1] = false;
    select_set(c, c->cur_set);
    c->last_nframes = 0;
    c->out_valid = false;
    return PSDR_OK;
}
extern "C" int psdr_band_region(psdr_ctx *c, int band, const float **d_region, size_t *frame_stride_bins, uint32_t *first_bin,
                                uint32_t *nbins) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (!c->nbands) return fail(PSDR_ERR_STATE, "psdr_set_band_layout() first");
    if (band < 0 || band >= c->nbands) return fail(PSDR_ERR_INVALID, "band %d outside [0, %d)", band, c->nbands);
    if (d_region) *d_region = (const float *)(c->d_spec + (size_t)band * c->lay.band_stride);
    if (frame_stride_bins) *frame_stride_bins = c->spec_stride;
    if (first_bin) *first_bin = (uint32_t)((size_t)band << (c->lay.l2Lb + c->log2M1));
    if (nbins) *nbins = (uint32_t)c->spec_stride;
    return PSDR_OK;
}
// ---- waterfall ---------------------------------------------------------------------------
static int check_wslot(psdr_ctx *c, int id) {
    if (id < 0 || id >= (int)c->wslots.size() || !c->wslots[id].active)
        return fail(PSDR_ERR_INVALID, "no waterfall client with id %d", id);
    return PSDR_OK;
}
extern "C" int psdr_waterfall_add(psdr_ctx *c, int *id_out) {
    if (!c || !id_out) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    for (size_t i = 0; i < c->wslots.size(); i++)
        if (!c->wslots[i].active) {
            WfSlot &s = c->wslots[i];
            s = WfSlot();
            s.active = true;
            // default = whole spectrum at the coarsest level (src/websocket.cpp:198)
            s.level = c->levels - 1;
            s.l = 0;
            s.r = std::min(c->min_waterfall_fft, (int)(c->R >> s.level));  // set_waterfall_range(levels-1, 0, min_waterfall_fft)
            s.det = c->opt_wf_det;
            *id_out = (int)i;
            return PSDR_OK;
        }
    return fail(PSDR_ERR_NOMEM, "all %zu waterfall client slots are in use", c->wslots.size());
}
extern "C" int psdr_waterfall_remove(psdr_ctx *c, int id) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    int rc = check_wslot(c, id);
    if (rc) return rc;
    c->wslots[id].active = false;
    return PSDR_OK;
}
// PSDR_WF_MEAN's sums are 32 bits wide: 255 per frame, at most skip_num frames in a window
static int check_wf_detector(const psdr_ctx *c, int detector) {
    if (detector != PSDR_WF_SAMPLE && detector != PSDR_WF_PEAK && detector != PSDR_WF_MEAN)
        return fail(PSDR_ERR_INVALID, "waterfall detector %d: PSDR_WF_SAMPLE, PSDR_WF_PEAK or PSDR_WF_MEAN", detector);
    if (detector == PSDR_WF_MEAN && c->cfg.skip_num > (1 << 24))
        return fail(PSDR_ERR_UNSUPPORTED, "PSDR_WF_MEAN with skip_num %d > 2^24", c->cfg.skip_num);
    return PSDR_OK;
}
int psdr::set_wf_default_detector(psdr_ctx *c, int detector) {
    int rc = check_wf_detector(c, detector);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mtx);
    c->opt_wf_det = detector;
    return PSDR_OK;
}
extern "C" int psdr_waterfall_set_detector(psdr_ctx *c, int id, int detector) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    int rc = check_wslot(c, id);
    if (rc) return rc;
    rc = check_wf_detector(c, detector);
    if (rc) return rc;
    c->wslots[id].det = detector;
    return PSDR_OK;
}
extern "C" int psdr_waterfall_set_range(psdr_ctx *c, int id, int level, int l, int r) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    int rc = check_wslot(c, id);
    if (rc) return rc;
    if (level < 0 || level >= c->levels) return fail(PSDR_ERR_INVALID, "level %d out of range", level);
    const int len = (int)(c->R >> level);
    if (l < 0) l = 0;
    if (r > len) r = len;  // the reference forgets this bound (src/waterfall.cpp:55-58)
    if (l > r) return fail(PSDR_ERR_INVALID, "empty waterfall range");
    WfSlot &s = c->wslots[id];
    s.level = level;
    s.l = l;
    s.r = r;
    return PSDR_OK;
}
extern "C" int psdr_waterfall_on_window_message(psdr_ctx *c, int id, int new_l, int new_r,
                                                int *level_out, int *l_out, int *r_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    // src/waterfall.cpp:53-79
    if (new_l < 0 || new_r < 0 || new_l >= new_r) return fail(PSDR_ERR_INVALID, "window rejected");
    const int mwf = c->min_waterfall_fft;
    float new_l_f = (float)new_l, new_r_f = (float)new_r;
    int new_level = c->levels - 1;
    float best = (float)(mwf * 2);
    for (int i = 0; i < c->levels; i++) {
        const float send_size = std::fabs((new_r_f - new_l_f) - (float)mwf);
        if (send_size < best) {
            best = send_size;
            new_level = i;
            new_l = (int)std::round(new_l_f);
            new_r = (int)std::round(new_r_f);
        }
        new_l_f /= 2;
        new_r_f /= 2;
    }
    int rc = psdr_waterfall_set_range(c, id, new_level, new_l, new_r);
    if (rc) return rc;
    if (level_out) *level_out = new_level;
    if (l_out) *l_out = c->wslots[id].l;
    if (r_out) *r_out = c->wslots[id].r;
    return PSDR_OK;
}

extern "C" int psdr_waterfall_batch(psdr_ctx *c, uint64_t first_frame_num) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (c->last_nframes < 1) return fail(PSDR_ERR_STATE, "waterfall_batch before process_batch/execute");
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    const int ring = c->wf_ring.acquire();
    if (ring < 0) return fail(PSDR_ERR_HIP, "waterfall parameter ring: event wait failed");
    WfClient *h_wf = (WfClient *)c->wf_ring.host(ring);
    WfClient *d_wf = (WfClient *)c->wf_ring.dev(ring);
    int *h_sent = (int *)((unsigned char *)c->wf_ring.host(ring) + c->wf_sent_off);
    int *d_sent = (int *)((unsigned char *)c->wf_ring.dev(ring) + c->wf_sent_off);
    const int nf = c->last_nframes;
    WfFacts facts;
    facts.R = c->R, facts.levels = c->levels, facts.tiled_lt = c->tiled_lt, facts.tile_ch = c->tile_ch, facts.skip_num = c->cfg.skip_num;
    // who is sent which frames and where, and what becomes of the detectors' carry (forwardplan.h)
    const WfPlan p = wf_plan(c->wslots.data(), c->wslots.size(), facts, c->wf_carry, first_frame_num, nf, h_wf, h_sent);
    c->wf_carry.carry_n = p.carry_n;  // (0 unless this call continues the carry's run: before anything below can fail)
    c->wf_carry.run = false;          // (true again once everything below is enqueued)
    if (!p.gather && !p.hold) return PSDR_OK;
    const int nsent = p.nsent, maxid = p.maxid;
    WfHoldArgs ha{};
    if (p.hold) {
        if (!c->d_wf_peak) {  // first use: the carry mirrors one frame's records and upper levels
            const WfCarryLayout lay = wf_carry_layout(c->tiled_lt, c->levels, c->R, c->q_len, c->q_stride, c->qt_stride);
            if (!lay.ok)
                return fail(PSDR_ERR_UNSUPPORTED, "waterfall detectors: record buffers of %zu / %zu bytes per frame", c->qt_stride, c->q_stride);
            c->wf_lay = lay;
            const size_t len = lay.lenA + lay.lenB;
            DevBuf<int8_t> pk;
            DevBuf<uint32_t> sm;
            if (pk.alloc(len) || sm.alloc(len)) {
                (void)hipGetLastError();
                return fail(PSDR_ERR_NOMEM, "waterfall detectors: carry of %zu bytes", len * 5);
            }
            c->d_wf_peak = std::move(pk);
            c->d_wf_sum = std::move(sm);
        }
        ha.Q = c->d_q;
        ha.Qt = c->d_qt;
        ha.q_stride = c->q_stride;
        ha.qt_stride = c->qt_stride;
        ha.lenA = c->wf_lay.lenA;
        ha.qB0 = c->wf_lay.qB0;
        ha.lenB = c->wf_lay.lenB;
        ha.peak = c->d_wf_peak;
        ha.sum = c->d_wf_sum;
        ha.carry_n = p.carry_n;
        ha.skip = c->cfg.skip_num;
        ha.nframes = nf;
    }
    if (p.gather) {
        if (p.total > c->wfout_cap) {
            PSDRCHK(c->d_wfout.alloc(p.total));  // (the old rows are given up only once the new buffer exists)
            c->wfout_cap = p.total;
        }
        {  // d_wfout exists once: a result fetch in flight (psdr_fetch_begin) reads it first
            int rc = fetch_guard_wait(c, c->side, c->guard_wf);
            if (rc) return rc;
            c->guard_wf = nullptr;
        }
        HIPCHK(hipMemcpyAsync(d_wf, h_wf, (size_t)(maxid + 1) * sizeof(WfClient), hipMemcpyHostToDevice,
                              c->side));
        HIPCHK(hipMemcpyAsync(d_sent, h_sent, (size_t)nsent * sizeof(int), hipMemcpyHostToDevice,
                              c->side));
        if (p.any_sample || !p.hold) {
            ProfScope ps(c, K_WFALL, c->side);
            hipLaunchKernelGGL(k_waterfall_gather, dim3(maxid + 1, nsent), dim3(256), 0, c->side, c->d_q,
                               c->q_stride, c->d_qt, c->qt_stride, c->tiled_lt, c->tile_ch, c->recmap, d_wf, d_sent, nsent,
                               c->d_wfout);
            HIPCHK(hipGetLastError());
        }
        if (p.hold) {  // behind the gather: it rewrites the rows of the clients with a detector
            ProfScope ps(c, K_WFHOLD, c->side);
            hipLaunchKernelGGL(k_waterfall_hold, dim3(maxid + 1, nsent), dim3(256), 0, c->side, ha, c->tiled_lt, c->tile_ch,
                               c->recmap, d_wf, d_sent, nsent, c->d_wfout);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(c->wf_ring.release(ring, c->side));
    }
    if (p.hold) {
        if (p.f0 < nf) {  // the carry for the next call
            ProfScope ps(c, K_WFCARRY, c->side);
            const size_t lanes = (ha.lenA + ha.lenB) / 16;
            hipLaunchKernelGGL(k_waterfall_carry, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, c->side, ha, p.f0, p.accumulate);
            HIPCHK(hipGetLastError());
        }
        c->wf_carry = p.after;
    }
    return side_done(c);
}
extern "C" int psdr_read_waterfall(psdr_ctx *c, int id, int8_t *out, size_t out_cap, int *nsent_out, int *level_out,
                                   int *l_out, int *r_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    int rc = check_wslot(c, id);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    const WfSlot &s = c->wslots[id];
    // the window of the BATCH, not the live one (it may have changed since)
    const size_t bytes = (size_t)s.nsent * (size_t)(s.b_r - s.b_l);
    if (nsent_out) *nsent_out = s.nsent;
    if (level_out) *level_out = s.b_level;
    if (l_out) *l_out = s.b_l;
    if (r_out) *r_out = s.b_r;
    if (bytes == 0 || !out) return PSDR_OK;
    if (bytes > out_cap) return fail(PSDR_ERR_INVALID, "output buffer too small (%zu > %zu)", bytes, out_cap);
    {
        int rc2 = drain(c);
        if (rc2) return rc2;
    }
    HIPCHK(hipMemcpyAsync(out, c->d_wfout + s.out_off, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PSDR_OK;
}

// ---- raw results ---------------------------------------------------------------------------
extern "C" int psdr_spectrum_device_ptr(psdr_ctx *c, int frame, const float **d_spec, size_t *nbins) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (frame < 0 || frame >= c->max_batch) return fail(PSDR_ERR_INVALID, "frame %d out of range", frame);
    if (c->nbands) return fail(PSDR_ERR_UNSUPPORTED, "banded spectrum: a frame is not one piece (psdr_band_region)");
    if (d_spec) *d_spec = (const float *)(c->d_spec + (size_t)frame * c->spec_stride);
    if (nbins) *nbins = c->is_real ? c->N / 2 + 1 : c->N;
    return PSDR_OK;
}
extern "C" int psdr_quantized_device_ptr(psdr_ctx *c, int frame, const int8_t **d_q, size_t *nbytes) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (frame < 0 || frame >= c->max_batch) return fail(PSDR_ERR_INVALID, "frame %d out of range", frame);
    PSDRCHK(level_major_ready(c, frame));
    if (d_q) *d_q = c->d_q + (size_t)frame * c->q_stride;
    if (nbytes) *nbytes = c->q_len;
    return PSDR_OK;
}
extern "C" int psdr_read_spectrum(psdr_ctx *c, int frame, float *out) {
    if (!c || !out) return fail(PSDR_ERR_INVALID, "null argument");
    if (frame < 0 || frame >= c->last_nframes) return fail(PSDR_ERR_INVALID, "frame %d not in the last batch", frame);
    HIPCHK(hipSetDevice(c->device));
    return copy_spectrum_k_order(c, frame, (cf *)out);
}
extern "C" int psdr_read_quantized(psdr_ctx *c, int frame, int8_t *out) {
    if (!c || !out) return fail(PSDR_ERR_INVALID, "null argument");
    if (frame < 0 || frame >= c->last_nframes) return fail(PSDR_ERR_INVALID, "frame %d not in the last batch", frame);
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(level_major_ready(c, frame));
    HIPCHK(hipMemcpyAsync(out, c->d_q + (size_t)frame * c->q_stride, c->q_len, hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PSDR_OK;
}

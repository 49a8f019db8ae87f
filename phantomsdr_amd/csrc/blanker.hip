// blanker.hip - the wideband impulse blanker on the ingest ring: psdr_ring_set_blanker / psdr_ring_read_blanker /
// psdr_ring_read of the C-ABI and blanker_enqueue, which psdr_process_ring (context.hip) calls in front of pass 1 when the
// blanker is on.  The plan of a call is blankerplan.h's nb_plan; the kernels are blanker.h's.
#include "blanker.h"
#include "ctx.h"

namespace psdr {

int blanker_enqueue(psdr_ctx *c, uint64_t first_half, int nframes) {
    auto &nb = c->nb;
    const auto &r = c->ring;
    const NbPlan p = nb_plan(nb.st, first_half, nframes, r.nhalves, nb.rcap);
    nb.st = p.after;
    nb.last_first = p.first_new, nb.last_n = p.nnew, nb.last_r0 = p.r0;
    if (p.nnew == 0) return PSDR_OK;  // every half of the call was blanked by an earlier one
    NbArgs a{};
    a.ring = r.d;
    a.hb = r.hb;
    a.nhalves = r.nhalves, a.slot0 = p.slot0, a.nnew = p.nnew;
    a.nblocks = (int)(c->N / 2 / NB_BLOCK);
    a.fmt = c->cfg.input_format, a.real = c->is_real ? 1 : 0, a.guard = nb.guard;
    a.kf = nb.kf;
    a.bmax = nb.d_bmax;
    a.R = nb.d_R;
    a.rcap = nb.rcap, a.r0 = p.r0, a.own = p.own ? 1 : 0;
    a.mask = nb.d_mask;
    a.list = nb.d_list;
    a.nlist = nb.d_count + (c->max_batch + 1);
    a.count = nb.d_count;
    const size_t ntiles = r.hb / NB_TILE * (size_t)p.nnew, nblk = (size_t)p.nnew * a.nblocks;
    const unsigned sparse = (unsigned)std::min<size_t>(nblk, (size_t)c->num_cus * 2);
    {
        ProfScope ps(c, K_NB_SCAN);
        hipLaunchKernelGGL(k_nb_block_max, dim3((unsigned)std::min<size_t>(ntiles, (size_t)c->num_cus * 16)), dim3(256), 0, c->stream, a);
        HIPCHK(hipGetLastError());
    }
    ProfScope ps(c, K_NB_APPLY);
    hipLaunchKernelGGL(k_nb_ref, dim3(p.nnew), dim3(64), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_nb_list, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_nb_mark, dim3(sparse), dim3(256), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_nb_zero, dim3(sparse), dim3(256), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return PSDR_OK;
}

}  // namespace psdr

extern "C" int psdr_ring_set_blanker(psdr_ctx *c, int on, double threshold_db, int guard) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (!c->ring.d) return fail(PSDR_ERR_STATE, "psdr_ring_create() first");
    switch (nb_check(on, threshold_db, guard)) {
    case NB_BAD_DB: return fail(PSDR_ERR_INVALID, "threshold_db %g outside [0, %g]", threshold_db, NB_DB_MAX);
    case NB_BAD_GUARD: return fail(PSDR_ERR_INVALID, "guard %d outside 0..%d", guard, NB_GUARD_MAX);
    case NB_OK: break;
    }
    auto &nb = c->nb;
    if (!on) {
        nb.on = false;
        return PSDR_OK;
    }
    if (!nb.d_bmax) {  // the first on = 1: all of the device state or none of it
        HIPCHK(hipSetDevice(c->device));
        const size_t halves = (size_t)c->max_batch + 1, nblk = halves * (c->N / 2 / NB_BLOCK);
        DevBuf<float> bmax, R;
        DevBuf<unsigned> mask, list, count;
        if (bmax.alloc(nblk) || R.alloc(halves + 1, true) || mask.alloc(nblk * 8) || list.alloc(nblk) || count.alloc(halves + 1, true))
            return fail(PSDR_ERR_NOMEM, "the blanker's device state (%zu blocks) could not be allocated", nblk);
        nb.d_bmax = std::move(bmax), nb.d_R = std::move(R), nb.d_mask = std::move(mask), nb.d_list = std::move(list), nb.d_count = std::move(count);
        nb.rcap = (int)halves + 1;
    }
    if (!nb.on) nb.st.fresh = true;  // switching on starts the reference afresh
    nb.on = true;
    nb.kf = nb_factor(threshold_db);
    nb.guard = guard;
    return PSDR_OK;
}

extern "C" int psdr_ring_read_blanker(psdr_ctx *c, uint64_t half_index, uint32_t *blanked, float *ref_level) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (!c->ring.d) return fail(PSDR_ERR_STATE, "psdr_ring_create() first");
    const auto &nb = c->nb;
    if (half_index < nb.last_first || half_index - nb.last_first >= (uint64_t)nb.last_n)
        return fail(PSDR_ERR_NO_DATA, "half %llu was not blanked by the last psdr_process_ring call", (unsigned long long)half_index);
    const int j = (int)(half_index - nb.last_first);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (blanked) HIPCHK(hipMemcpy(blanked, nb.d_count + j, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (ref_level) HIPCHK(hipMemcpy(ref_level, nb.d_R + (nb.last_r0 + j) % nb.rcap, sizeof(float), hipMemcpyDeviceToHost));
    return PSDR_OK;
}

extern "C" int psdr_ring_read(psdr_ctx *c, uint64_t half_index, void *host_half) {
    if (!c || !host_half) return fail(PSDR_ERR_INVALID, "null argument");
    const auto &r = c->ring;
    if (!r.d) return fail(PSDR_ERR_STATE, "psdr_ring_create() first");
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    HIPCHK(hipMemcpy(host_half, r.d + (size_t)(half_index % (uint64_t)r.nhalves) * r.hb, r.hb, hipMemcpyDeviceToHost));
    return PSDR_OK;
}

// (not in psdr.h: the blanker's tests) the device state a context that never switched the blanker on does not have: block
// maxima, levels, masks, work list, counts; and the mirror copy of slot 0 at out[5]
extern "C" int psdr_debug_blanker_ptrs(psdr_ctx *c, const void *out[6]) {
    if (!c || !out) return fail(PSDR_ERR_INVALID, "null argument");
    const auto &nb = c->nb;
    out[0] = nb.d_bmax.get(), out[1] = nb.d_R.get(), out[2] = nb.d_mask.get(), out[3] = nb.d_list.get(), out[4] = nb.d_count.get();
    out[5] = c->ring.d ? c->ring.d.get() + (size_t)c->ring.nhalves * c->ring.hb : nullptr;
    return PSDR_OK;
}

// fax.hip - k_audio_fax, the kernel behind fax.h
#include "fax.h"

namespace psdr {

constexpr int FAX_CHUNK = 256;  // samples the work-group takes at once, one per thread
constexpr int FAX_LRING = 512;  // samples of z, y and v in LDS, by t % 512: the chunk, the boxcar's reach and an unfinished hop behind it
constexpr int FAX_HOPS = FAX_CHUNK / 8 + 1;  // hops a chunk can complete at the shortest hop
static_assert(FAX_LRING >= FAX_CHUNK + FAX_ZT && FAX_LRING >= FAX_CHUNK + FAX_HMAX && (FAX_LRING & (FAX_LRING - 1)) == 0, "a chunk overwrites nothing it reads");
static_assert(4 * FAX_HOPS <= FAX_CHUNK, "four threads per hop");

// the machine's scalars are the same in every thread: said to the compiler, word by word, they stay out of the vector registers
__device__ inline void fax_uniform(FaxScalars &z) {
    static_assert(sizeof(FaxScalars) % 4 == 0, "words");
    int w[sizeof(FaxScalars) / 4];
    memcpy(w, &z, sizeof(z));
#pragma unroll
    for (size_t i = 0; i < sizeof(FaxScalars) / 4; i++) w[i] = __builtin_amdgcn_readfirstlane(w[i]);
    memcpy(&z, w, sizeof(z));
}

// One work-group of 256 threads per listed client, in the coordinates of fax_stream.  The batch's samples go in chunks of up to 256
// that end where the line being built ends, so that line, origin and state are the same for a whole chunk: (1) a thread per sample
// takes z, behind a barrier y, behind another v and the column, all into LDS rings by t % 512 that the carried tails were loaded
// into; (2) the thread on a pixel's first sample sums the pixel in ascending order and stores its byte into the line being built
// (the one the chunk leaves open goes on as sum and count); (3) four threads per hop the chunk completes take the three tone
// correlations and Q, M; (4) every thread walks those hops in order with fax_hop_step on the same values - the machine is a handful
// of scalars, the same in all four waves - and wave 0 writes the records of the frames each hop ends.  A completed line is the
// work-group's: the phasing search's window sums a column per thread with an integer arg-max in LDS, a kept line's copy into the
// ring a byte per thread.
__global__ __launch_bounds__(FAX_CHUNK) void k_audio_fax(FaxArgs a) {
    __shared__ ToneC zs[FAX_LRING], ys[FAX_LRING];
    __shared__ float vs[FAX_LRING];
    __shared__ float hopr[FAX_HOPS][8];
    __shared__ uint16_t cs[FAX_CHUNK];
    __shared__ uint8_t lm[FAX_WIDTH_MAX];
    __shared__ unsigned s_key, s_sum;
    __shared__ float s_psum;
    __shared__ int s_pcnt, s_pcol;
    const int tid = threadIdx.x, lane = tid & 63;
    if ((int)blockIdx.x >= a.nlist) return;
    const FaxEntry &e = a.list[blockIdx.x];
    const int slot = e.slot, width = e.width;
    const size_t frow = (size_t)slot * a.max_batch;
    FaxState *st = a.state + slot;
    uint8_t *line = st->line;
    uint8_t *ring = a.ring + (size_t)slot * a.rmax * FAX_WIDTH_MAX;
    uint32_t *meta = a.meta + (size_t)slot * a.rmax;
    const float *rows = a.audio + frow * a.h;
    const int *flags = a.nan_flags + frow;
    const ToneTables *T = &a.tab->t;
    const int h = a.h, H = a.tab->H, hs = __ffs(H) - 1;  // (H is a power of two)
    const ToneC rot = {e.rot[0], e.rot[1]};
    // ---- what the state holds is read before anything is written
    const uint64_t pos0 = st->pos, L = (uint64_t)a.nframes * (uint64_t)h, pos1 = pos0 + L, b0 = pos0 >> hs;
    FaxScalars z = st->z;
    fax_uniform(z);
    FaxRec last = st->last;
    if (pos0 == 0) fax_start(z, e), last = fax_record(z, e);
    if (tid < FAX_ZT) zs[(pos0 - FAX_ZT + tid) & (FAX_LRING - 1)] = st->zt[tid];
    if (tid < FAX_YT) ys[(pos0 - FAX_YT + tid) & (FAX_LRING - 1)] = st->yt[tid];
    if (tid < FAX_HMAX && b0 * H + tid < pos0) vs[(b0 * H + tid) & (FAX_LRING - 1)] = st->vpart[tid];
    __syncthreads();

    // the frames at whose end D hops are complete take the record behind hop D - 1 (wave 0)
    auto emit = [&](uint64_t D) {
        const int lo = cw_first_frame(D, pos0, h, H), up = min(a.nframes, cw_first_frame(D + 1, pos0, h, H));
        for (int f = lo + lane; f < up; f += 64) a.rec[frow + f] = last;
    };
    if (tid < 64) emit(b0);

    for (uint64_t t0 = pos0; t0 < pos1;) {
        // ---- the lines that sample t0 completes (a second one only behind a move of less than a sample)
        while (fax_tq(t0, e.Lq) >= z.lstart + e.Lq) {
            if (tid == 0 && z.pcnt) line[z.pcol] = fax_byte(z.psum, z.pcnt);
            z.pcnt = 0, z.psum = 0.f, z.pcol = -1;
            __syncthreads();
            uint64_t move = 0;
            if (z.skip) {
                z.skip = 0;
            } else if (z.state == FAX_PHASING) {
                unsigned part = 0;
                for (int c = tid; c < width; c += FAX_CHUNK) part += (lm[c] = line[c]);
                if (tid == 0) s_key = 0u, s_sum = 0u;
                __syncthreads();
                atomicAdd(&s_sum, part);
                __syncthreads();
                const int sum = (int)s_sum;
                const bool dark = 2 * sum >= 255 * width;
                for (int c = tid; c < width; c += FAX_CHUNK) {
                    int win = 0, j = c;
                    for (int i = 0; i < e.wp; i++) {
                        win += lm[j];
                        j = j + 1 == width ? 0 : j + 1;
                    }
                    const unsigned dev = (unsigned)(dark ? 255 * e.wp - win : win);
                    atomicMax(&s_key, dev << 12 | (unsigned)(4095 - c));  // the largest dev, of those the lowest column
                }
                __syncthreads();
                const unsigned key = s_key;
                move = fax_phase_step(z, e, (int)(key >> 12), 4095 - (int)(key & 4095u), dark ? 255 * width - sum : sum);
            } else if (z.state == FAX_IMAGE) {
                const size_t r = (size_t)z.rrow;
                for (int c = tid; c < width; c += FAX_CHUNK) ring[r * width + c] = line[c];
                const uint32_t m = fax_keep(z, e);
                if (tid == 0) meta[r] = m;
            }
            fax_next_line(z, e, move);
            __syncthreads();
        }
        const uint64_t stop = min(pos1, fax_line_stop(z.lstart));
        const int n = (int)min((uint64_t)FAX_CHUNK, stop - t0);
        const uint64_t t = t0 + (uint64_t)tid;
        // ---- (1) z, y, v and the column
        if (tid < n) {
            const uint32_t o = (uint32_t)(t - pos0);
            const float x = flags[o / (uint32_t)h] ? 0.f : rows[o];
            zs[t & (FAX_LRING - 1)] = fax_z(x, fax_w(T, e.inc, rot, t, H));
        }
        __syncthreads();
        if (tid < n) ys[t & (FAX_LRING - 1)] = fax_y(e.K, [&](int i) { return zs[(t - (uint64_t)i) & (FAX_LRING - 1)]; });
        __syncthreads();
        if (tid < n) {
            vs[t & (FAX_LRING - 1)] = fax_v(ys[t & (FAX_LRING - 1)], ys[(t - (uint64_t)e.D) & (FAX_LRING - 1)], e.s);
            cs[tid] = (uint16_t)fax_col(fax_tq(t, e.Lq), z.lstart, e.Lq, width);
        }
        __syncthreads();
        // ---- (2) the pixels: the thread on a pixel's first sample sums it, t ascending
        if (tid < n) {
            const int col = cs[tid];
            if (tid == 0 || (int)cs[tid - 1] != col) {
                float acc = 0.f;
                int cnt = 0;
                if (tid == 0) {
                    if (col == z.pcol)
                        acc = z.psum, cnt = z.pcnt;
                    else if (z.pcnt)
                        line[z.pcol] = fax_byte(z.psum, z.pcnt);
                }
                int j = tid;
                for (; j < n && (int)cs[j] == col; j++) acc = acc + vs[(t0 + (uint64_t)j) & (FAX_LRING - 1)], cnt++;
                if (j < n)
                    line[col] = fax_byte(acc, cnt);
                else
                    s_psum = acc, s_pcnt = cnt, s_pcol = col;
            }
        }
        // ---- (3) the hops the chunk completes: threads 4 q .. 4 q + 3 take hop hb0 + q
        const uint64_t hb0 = t0 >> hs;
        const int nh = (int)(((t0 + (uint64_t)n) >> hs) - hb0);
        if (e.mode == PSDR_FAX_AUTO && (tid >> 2) < nh) {
            const int q = tid >> 2, k = tid & 3;
            const uint64_t b = hb0 + (uint64_t)q;
            auto V = [&](int i) { return vs[(b * (uint64_t)H + (uint64_t)i) & (FAX_LRING - 1)]; };
            if (k < 3) {
                const ToneC c = fax_tone_corr(T, e.tinc[k], ToneC{e.trot[k][0], e.trot[k][1]}, b, H, V);
                hopr[q][2 * k] = c.re, hopr[q][2 * k + 1] = c.im;
            } else {
                fax_tone_qm(H, V, hopr[q][6], hopr[q][7]);
            }
        }
        __syncthreads();
        z.psum = s_psum, z.pcnt = s_pcnt, z.pcol = s_pcol;
        // ---- (4) the hops in order
        for (int q = 0; q < nh; q++) {
            if (e.mode == PSDR_FAX_AUTO) fax_hop_step(z, e, hopr[q]);
            last = fax_record(z, e);
            if (tid < 64) emit(hb0 + (uint64_t)q + 1);
        }
        __syncthreads();  // the chunk's columns, sums and hops are read: the next chunk may write its own
        t0 += (uint64_t)n;
    }
    // ---- the tails, the unfinished hop and the machine
    if (tid < FAX_ZT) st->zt[tid] = zs[(pos1 - FAX_ZT + tid) & (FAX_LRING - 1)];
    if (tid < FAX_YT) st->yt[tid] = ys[(pos1 - FAX_YT + tid) & (FAX_LRING - 1)];
    if (tid < FAX_HMAX) {
        const uint64_t u = (pos1 >> hs << hs) + (uint64_t)tid;
        st->vpart[tid] = u < pos1 ? vs[u & (FAX_LRING - 1)] : 0.f;
    }
    if (tid == 0) st->pos = pos1, st->z = z, st->last = last;
}

hipError_t audio_fax_launch(const FaxArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_audio_fax, dim3((unsigned)a.nlist), dim3(FAX_CHUNK), 0, s, a);
    return hipGetLastError();
}

}  // namespace psdr

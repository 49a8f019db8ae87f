// nr.hip - k_audio_nr, the kernel behind nr.h
#include "nr.h"

namespace psdr {

constexpr int NR_SPAN = (NR_WAVES - 1) * NR_R + NR_M;  // input samples under a group of NR_WAVES blocks
constexpr int NR_GROUP = NR_WAVES * NR_R;              // outputs a full group finishes
constexpr int NR_TW = 192;                             // twiddles the network reads: r k < 3 * 64

// between two stages: every point to where stage s puts it, then point lane + 64 r back (buf: the wave's own)
__device__ inline void nr_exchange(int s, int lane, NrC *v, NrC *buf) {
#pragma unroll
    for (int r = 0; r < 4; r++) buf[nr_out_index(s, lane, r)] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = buf[lane + 64 * r];
    __syncthreads();
}
// nr_fft with butterfly j = lane: in and out, lane holds points lane + 64 r (behind the last stage nothing moves)
__device__ inline void nr_fft_wave(int lane, NrC *v, NrC *buf, const float (*tw)[2]) {
#pragma unroll
    for (int s = 0; s < NR_STAGES; s++) {
        nr_butterfly(s, lane, v, tw);
        if (s + 1 < NR_STAGES) nr_exchange(s, lane, v, buf);
    }
}

// One work-group per listed client, in the coordinates of nr_stream: u counts from the first unconsumed input sample, X(u) is
// the carried tail (u < t0) and then the rows, the batch finishes blocks 0 .. nbn - 1 and Y(u) for u < nbn R, and Y(u) belongs
// at row offset u + M - t0 - or, behind the batch's end, into the pending outputs.  The blocks go in groups of NR_WAVES, one per
// wave: (1) the group's input span into LDS, W floats per load (the loads of rows are unconditional and come before anything that
// depends on a flag; t0, U and h are multiples of W, so a piece is tail, row or nothing as a whole and lies in one frame), (2) the
// outputs of the group BEFORE, which sit in the waves' buffers since its inverse transforms - the rows they overwrite are input
// that only now is all in LDS, (3) window and forward transform, the bins' powers to LDS, (4) threads 0..128 take bin k through the
// group's blocks in order, Ps, N and G in registers for the whole batch, (5) applied gains, inverse transform, window.  The pass
// behind the last full group holds the remaining blocks, if any, and the new tail.
template <int W>
__global__ __launch_bounds__(64 * NR_WAVES) void k_audio_nr(NrArgs a) {
    typedef float vec __attribute__((ext_vector_type(W)));
    __shared__ __attribute__((aligned(16))) float xin[NR_SPAN];
    __shared__ __attribute__((aligned(16))) NrC fb[NR_WAVES][NR_M];  // a wave's exchange buffer; its first M floats: its block's s
    __shared__ __attribute__((aligned(16))) float ola[NR_R];
    __shared__ float gb[NR_WAVES][NR_PAD];
    __shared__ float tw[NR_TW][2];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    if ((int)blockIdx.x >= a.nlist) return;
    const NrEntry e = a.list[blockIdx.x];
    NrState *st = a.state + e.slot;
    float *rows = a.audio + (size_t)e.slot * a.max_batch * a.h;
    const int *flags = a.nan_flags + (size_t)e.slot * a.max_batch;
    const int h = a.h, L = a.nframes * h;
    const uint64_t T0 = st->pos, nb0 = nr_blocks_done(T0);
    const int t0 = (int)(T0 - nb0 * NR_R), U = t0 + L;
    const int nbn = U >= NR_M ? (U - NR_M) / NR_R + 1 : 0;
    const bool had = nb0 != 0;
    const int npend = NR_M - t0;  // outputs p < npend are not of this batch's blocks: pending ones, or the first M zeros

    // ---- what the state holds is read before anything is written
    float Ps = 0.f, N = 0.f, G = 0.f;
    if (tid < NR_BINS) Ps = st->Ps[tid], N = st->N[tid], G = st->G[tid];
    if (tid < NR_R) ola[tid] = st->ola[tid];
    if (tid < NR_TW) tw[tid][0] = a.tab->tw[tid][0], tw[tid][1] = a.tab->tw[tid][1];
    float win[4];
#pragma unroll
    for (int r = 0; r < 4; r++) win[r] = a.tab->win[lane + 64 * r];
    const int pp = tid * W;
    vec pv = (vec)(0.f);
    if (had && pp < npend) pv = *(const vec *)(st->pend + pp);
    float keep = 0.f;  // no block finished: what stays pending moves up by L
    const bool moves = had && nbn == 0 && tid + L < npend;
    if (moves) keep = st->pend[tid + L];

    // outputs of blocks q0 .. q0 + cnt - 1, whose s sit in fb[0 .. cnt): Y = nr_ola(earlier block's second half, s's first)
    auto flush = [&](int q0, int cnt) {
        const int i = tid * W;
        if (i >= NR_GROUP) return;
        const int wq = i / NR_R, t = i % NR_R;
        const vec prev = wq ? *(const vec *)((const float *)fb[wq ? wq - 1 : 0] + NR_R + t) : *(const vec *)(ola + t);
        if (wq == 0 && cnt > 0) *(vec *)(ola + t) = *(const vec *)((const float *)fb[cnt - 1] + NR_R + t);
        if (wq >= cnt) return;
        const vec s = *(const vec *)((const float *)fb[wq] + t);
        vec y;
#pragma unroll
        for (int k = 0; k < W; k++) y[k] = nr_ola(prev[k], s[k]);
        const int p = (q0 + wq) * NR_R + t + npend;
        if (p < L) {
            if (flags[p / h] == 0) *(vec *)(rows + p) = y;
        } else {
            *(vec *)(st->pend + (p - L)) = y;  // (p - L < R: the last block's, nrplan.h)
        }
    };

    const int ngroups = nbn / NR_WAVES;
    for (int g = 0; g <= ngroups; g++) {
        const int u0 = g * NR_GROUP;
        for (int pc = tid; pc < NR_SPAN / W; pc += 64 * NR_WAVES) {
            const int u = u0 + pc * W, off = u - t0;
            const bool inrow = off >= 0 && u < U;
            vec v = *(const vec *)(rows + (inrow ? off : 0));
            const int flagged = flags[inrow ? off / h : 0];
            if (!inrow || flagged != 0) v = (vec)(0.f);
            if (u < t0) v = *(const vec *)(st->tail + u);
            *(vec *)(xin + pc * W) = v;
        }
        __syncthreads();
        if (g > 0) flush((g - 1) * NR_WAVES, NR_WAVES);
        __syncthreads();
        NrC v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) v[r].re = nr_window_in(xin[w * NR_R + lane + 64 * r], win[r]), v[r].im = 0.f;
        nr_fft_wave(lane, v, fb[w], tw);
        gb[w][lane] = nr_power(v[0].re, v[0].im), gb[w][lane + 64] = nr_power(v[1].re, v[1].im);
        if (lane == 0) gb[w][128] = nr_power(v[2].re, v[2].im);
        __syncthreads();
        if (tid < NR_BINS)
            for (int wq = 0; wq < NR_WAVES; wq++) {
                const int q = g * NR_WAVES + wq;
                if (q < nbn) gb[wq][tid] = nr_bin(gb[wq][tid], nb0 + (uint64_t)q == 0, e.g_min, e.beta, e.a_up, Ps, N, G);
            }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float gn = nr_applied(gb[w], nr_mirror(lane + 64 * r), e.g_min);
            const NrC z = {nr_mul(v[r].im, gn), nr_mul(v[r].re, gn)};  // (swapped: the inverse)
            v[r] = z;
        }
        nr_fft_wave(lane, v, fb[w], tw);
#pragma unroll
        for (int r = 0; r < 4; r++) ((float *)fb[w])[lane + 64 * r] = nr_window_out(v[r].im, win[r]);
    }
    __syncthreads();
    const int cnt = nbn - ngroups * NR_WAVES;
    flush(ngroups * NR_WAVES, cnt);
    // the new tail X[nbn R, U): inside the last pass's span
    st->tail[tid] = tid < U - nbn * NR_R ? xin[cnt * NR_R + tid] : 0.f;
    if (pp < npend && pp < L && flags[pp / h] == 0) *(vec *)(rows + pp) = pv;
    if (moves) st->pend[tid] = keep;
    if (tid < NR_BINS) st->Ps[tid] = Ps, st->N[tid] = N, st->G[tid] = G;
    __syncthreads();
    if (tid < NR_R) st->ola[tid] = ola[tid];
    if (tid == 0) st->pos = T0 + (uint64_t)L;
}

hipError_t audio_nr_launch(const NrArgs &a, hipStream_t s) {
    if (a.h % 4 == 0)
        hipLaunchKernelGGL(k_audio_nr<4>, dim3((unsigned)a.nlist), dim3(64 * NR_WAVES), 0, s, a);
    else
        hipLaunchKernelGGL(k_audio_nr<2>, dim3((unsigned)a.nlist), dim3(64 * NR_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace psdr

// anb.hip - k_audio_nb, the kernel behind anb.h
#include "anb.h"

namespace psdr {

constexpr int ANB_GROUP = ANB_WAVES * ANB_B;       // samples under a group of ANB_WAVES blocks
constexpr int ANB_SPAN = ANB_GROUP + 2 * ANB_E;    // ... with the edges the blocks read
constexpr int ANB_OUT = ANB_GROUP + 2 * ANB_G;     // ... with what the gaps reach
constexpr int ANB_WPE = 6;                         // waves per SIMD the kernel is built for: 512 / 6 leaves it 80 VGPRs
constexpr int ANB_EB = ANB_B + 16;                 // a wave's buffer: e[0, B + P), then its repaired gaps, 16 floats each

// the sum of the waves' 64 partials, in every lane the bits of anb_tree
__device__ inline float anb_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

// One work-group per listed client, in the batch's own coordinates: r = stream index - pos, so the carried input is r in
// [-H, 0) and the rows are r in [0, L).  The batch derives blocks qF .. qL - 1 (anb_stream) in groups of ANB_WAVES, one per wave;
// group g's first sample is sg.  xin holds the input [sg - E, sg + GROUP + E), yout the processed samples [sg - G, sg + GROUP + G):
// its first 2 G samples come from the group before (the input, with that group's gaps), the others from xin, and then the group's
// gaps go in, in the order of the centres.  Per group: (1) the input span into LDS, W floats per load (the loads of rows are
// unconditional and come before anything that depends on a flag; pos, L, H, E and h are multiples of W, so a piece is carried
// input, row or nothing as a whole and lies in one frame), (2) the processed samples of the group BEFORE to the rows - they
// overwrite input that only now is all in LDS -, (3) steps 1 to 3 of anbplan.h per wave, e to LDS, (4) matched filter, threshold
// and the scan by ballot, (5) lane k repairs gap k into the wave's buffer, (6) the gaps into yout.  The new carried input is
// written to the state's other half before any row is.
template <int W>
__global__ __launch_bounds__(64 * ANB_WAVES, ANB_WPE) void k_audio_nb(AnbArgs a) {
    typedef float vec __attribute__((ext_vector_type(W)));
    __shared__ __attribute__((aligned(16))) float xin[ANB_SPAN];
    __shared__ __attribute__((aligned(16))) float yout[ANB_OUT];
    __shared__ __attribute__((aligned(16))) float eb[ANB_WAVES][ANB_EB];
    __shared__ int cen[ANB_WAVES][ANB_MAX];
    __shared__ int ncen[ANB_WAVES];
    __shared__ unsigned tot[ANB_WAVES][2];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    if ((int)blockIdx.x >= a.nlist) return;
    const AnbEntry en = a.list[blockIdx.x];
    AnbState *st = a.state + en.slot;
    float *rows = a.audio + (size_t)en.slot * a.max_batch * a.h;
    const int *flags = a.nan_flags + (size_t)en.slot * a.max_batch;
    const int h = a.h, L = a.nframes * h;
    const int width = en.width, pl = (width - 1) / 2;
    const uint64_t T0 = st->pos;
    const int64_t qF = anb_first_block(T0), qL = anb_blocks_done(T0 + (uint64_t)L);
    const int base0 = (int)(qF * ANB_B - (int64_t)T0);                // block qF's first sample: inside (-H + E, 0]
    const int nblk = qL > qF ? (int)(qL - qF) : 0;                    // blocks this batch derives
    const int qnew = (int)(anb_blocks_done(T0) - qF);                 // ... of which these were counted before
    const int rstart = T0 < (uint64_t)ANB_H ? -(int)T0 : -ANB_H;      // the stream's start, as far as this batch can see it
    const int nzero = T0 < (uint64_t)ANB_D ? ANB_D - (int)T0 : 0;      // outputs of this batch among the stream's first D

    // ---- the new carried input [L - H, L) goes to the state's other half before any row is written (st->cur says which half holds
    // the carried input; it changes sides at the end)
    const float *hist = st->hist[st->cur & 1];
    {
        float *hnew = st->hist[(st->cur & 1) ^ 1];
#pragma unroll 1
        for (int pc = tid; pc < ANB_H / W; pc += 64 * ANB_WAVES) {
            const int r = L - ANB_H + pc * W;
            const bool inrow = r >= 0;
            vec v = *(const vec *)(rows + (inrow ? r : 0));
            const int flagged = flags[inrow ? r / h : 0];
            if (flagged != 0) v = (vec)(0.f);
            if (!inrow) v = *(const vec *)(hist + (r + ANB_H));
            *(vec *)(hnew + pc * W) = v;
        }
    }
    __syncthreads();

    // the processed samples of a group whose first sample is sg, cnt blocks of it derived: yout[0, cnt B) to the rows they are due in
    auto flush = [&](int sg, int cnt) {
#pragma unroll 1
        for (int yi = tid * W; yi < cnt * ANB_B; yi += 64 * ANB_WAVES * W) {
            const int r = sg - ANB_G + yi, p = r + ANB_D;
            if (r >= rstart && p >= 0 && p < L && flags[p / h] == 0) *(vec *)(rows + p) = *(const vec *)(yout + yi);
        }
    };

    unsigned imp = 0, smp = 0;
    const int ngroups = (nblk + ANB_WAVES - 1) / ANB_WAVES;
    for (int g = 0; g < ngroups; g++) {
        const int sg = base0 + g * ANB_GROUP;
#pragma unroll 1
        for (int pc = tid; pc < ANB_SPAN / W; pc += 64 * ANB_WAVES) {
            const int r = sg - ANB_E + pc * W;
            const bool inrow = r >= 0 && r < L;
            vec v = *(const vec *)(rows + (inrow ? r : 0));
            const int flagged = flags[inrow ? r / h : 0];
            if (!inrow || flagged != 0) v = (vec)(0.f);
            if (r < 0 && r >= -ANB_H) v = *(const vec *)(hist + (r + ANB_H));
            *(vec *)(xin + pc * W) = v;
        }
        __syncthreads();
        float carry = 0.f;
        if (tid < 2 * ANB_G) carry = g > 0 ? yout[ANB_GROUP + tid] : xin[ANB_E - ANB_G + tid];
        if (g > 0) flush(sg - ANB_GROUP, ANB_WAVES);
        __syncthreads();
        if (tid < 2 * ANB_G) yout[tid] = carry;
#pragma unroll 1
        for (int i = 2 * ANB_G + tid; i < ANB_OUT; i += 64 * ANB_WAVES) yout[i] = xin[i + ANB_E - ANB_G];

        // ---- steps 1 to 3: this wave's block (a wave without one runs on whatever its span holds and detects nothing)
        const int blk = g * ANB_WAVES + w;
        const float *xb = xin + ANB_E + w * ANB_B;
        float R[ANB_P + 1], c[ANB_P + 1];
#pragma unroll
        for (int i = 0; i <= ANB_P; i++) {
            R[i] = anb_wave_sum(anb_corr_partial(xb, lane, i));
            __builtin_amdgcn_sched_barrier(0);  // (one lag's loads at a time: all of them in flight cost the registers)
        }
        const bool usable = blk < nblk && __ballot(anb_usable(R[0])) != 0ull;  // (every lane holds the same R: a scalar for the scan below)
        anb_levinson(R, c);
#pragma unroll 1
        for (int r = 0; r < 4; r++) eb[w][lane + 64 * r] = anb_residual(c, xb + lane + 64 * r);
        if (lane < ANB_P) eb[w][ANB_B + lane] = anb_residual(c, xb + ANB_B + lane);
        __syncthreads();

        // ---- steps 4 and 5
        float m[4];
#pragma unroll
        for (int r = 0; r < 4; r++) m[r] = anb_matched(c, eb[w] + lane + 64 * r);
        const float mean = anb_mean(anb_wave_sum(((m[0] + m[1]) + m[2]) + m[3]));
        float dv = 0.f;
#pragma unroll
        for (int r = 0; r < 4; r++) dv = anb_dev2(m[r], mean, dv);
        const float T = anb_level(anb_wave_sum(dv), en.threshold);
        int cnt = 0, next = 0, myc = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            unsigned long long mask = usable ? __ballot(fabsf(m[r]) > T) : 0ull;  // samples [64 r, 64 r + 64) over T
            while (cnt < ANB_MAX) {
                const int lo = next - 64 * r;
                if (lo >= 64) break;
                if (lo > 0) mask &= ~0ull << lo;
                if (!mask) break;
                const int n = 64 * r + __ffsll(mask) - 1;
                if (lane == cnt) myc = n;
                if (blk >= qnew) imp += 1, smp += (unsigned)anb_gap_samples(qF + blk == 0 ? (int64_t)n : (int64_t)ANB_B, width);
                cnt++;
                next = n + pl + 1;
            }
        }
        if (lane < cnt) cen[w][lane] = myc;
        if (lane == 0) ncen[w] = cnt;
        __syncthreads();  // (every wave is done with e)

        // ---- step 6: lane k repairs gap k
        if (lane < cnt) anb_repair(c, xb + myc - pl, width, eb[w] + 16 * lane);
        __syncthreads();

        // ---- step 7: the gaps into yout; a sample that the next centre's gap holds too is left to it
        {
            const int k = tid >> 4, i = tid & 15;
#pragma unroll 1
            for (int wq = 0; wq < ANB_WAVES; wq++) {
                const int nc = ncen[wq];
                if (k < nc && i < width) {
                    const int pos = wq * ANB_B + cen[wq][k] - pl + i;
                    int nextc = 1 << 30;
                    if (k + 1 < nc)
                        nextc = wq * ANB_B + cen[wq][k + 1];
                    else if (wq + 1 < ANB_WAVES && ncen[wq + 1] > 0)
                        nextc = (wq + 1) * ANB_B + cen[wq + 1][0];
                    if (pos < nextc - pl) yout[pos + ANB_G] = eb[wq][16 * k + i];
                }
            }
        }
        __syncthreads();
    }
    if (ngroups > 0) flush(base0 + (ngroups - 1) * ANB_GROUP, nblk - (ngroups - 1) * ANB_WAVES);
    // the stream's first D outputs
    for (int p = tid * W; p < nzero && p < L; p += 64 * ANB_WAVES * W)
        if (flags[p / h] == 0) *(vec *)(rows + p) = (vec)(0.f);
    if (lane == 0) tot[w][0] = imp, tot[w][1] = smp;
    __syncthreads();
    if (tid == 0) {
        st->impulses += (uint64_t)tot[0][0] + tot[1][0] + tot[2][0] + tot[3][0];
        st->samples += (uint64_t)tot[0][1] + tot[1][1] + tot[2][1] + tot[3][1];
        st->pos = T0 + (uint64_t)L;
        st->cur ^= 1;
    }
}

hipError_t audio_nb_launch(const AnbArgs &a, hipStream_t s) {
    if (a.h % 4 == 0)
        hipLaunchKernelGGL(k_audio_nb<4>, dim3((unsigned)a.nlist), dim3(64 * ANB_WAVES), 0, s, a);
    else
        hipLaunchKernelGGL(k_audio_nb<2>, dim3((unsigned)a.nlist), dim3(64 * ANB_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace psdr

// audiofilter.hip - k_audio_filter, the kernel behind audiofilter.h
#include "audiofilter.h"

namespace psdr {

// bit k: sample i0 + k of the stream is not filtered data - it lies behind the stream's end L, or in a frame whose NaN flag is
// set.  A chunk spans several frames when h < 16 and two wherever a frame boundary falls inside it (h = 180).
__device__ inline unsigned af_dead_mask(const int *flags, int i0, int h, int L) {
    unsigned m = 0;
    int f = i0 / h, left = h - (i0 - f * h);
    for (int k = 0; k < AF_CHUNK;) {
        const int cnt = min(left, AF_CHUNK - k);
        if (i0 + k >= L || flags[f] != 0) m |= ((1u << cnt) - 1u) << k;  // (i0 + k < L: f < nframes)
        k += cnt, f++, left = h;
    }
    return m;
}

// One wave per listed client; the stream goes in blocks of 64 lanes x 16 consecutive samples.  W floats per load and store: 4
// where h % 4 == 0 (a client's stream base, max_batch * h floats into the rows, and every lane's chunk are then 16-byte aligned, and
// no 16-byte piece crosses a frame), else 2 (h is even).  The loads are unconditional - a lane behind the stream's end reads the
// stream's first bytes and drops them - and come before anything that depends on a flag.
template <int W>
__global__ __launch_bounds__(64) void k_audio_filter(AudioFilterArgs a) {
    typedef float vec __attribute__((ext_vector_type(W)));
    constexpr int NV = AF_CHUNK / W;
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= a.nlist) return;
    const AfEntry *__restrict__ e = a.list + blockIdx.x;
    const int slot = __builtin_amdgcn_readfirstlane(e->slot), nsec = __builtin_amdgcn_readfirstlane(e->nsec);
    float *rows = a.audio + (size_t)slot * a.max_batch * a.h;
    const int *flags = a.nan_flags + (size_t)slot * a.max_batch;
    const int L = a.nframes * a.h;
    float st[2 * PSDR_AUDIO_FILTER_SECTIONS];
    for (int i = 0; i < 2 * PSDR_AUDIO_FILTER_SECTIONS; i++) st[i] = a.state[(size_t)slot * 2 * PSDR_AUDIO_FILTER_SECTIONS + i];
    for (int b0 = 0; b0 < L; b0 += AF_BLOCK) {
        const int i0 = b0 + lane * AF_CHUNK;
        float x[AF_CHUNK];
#pragma unroll
        for (int q = 0; q < NV; q++) {
            const int i = i0 + q * W;
            const vec v = *(const vec *)(rows + (i < L ? i : 0));
#pragma unroll
            for (int k = 0; k < W; k++) x[q * W + k] = v[k];
        }
        const unsigned dead = af_dead_mask(flags, i0, a.h, L);
#pragma unroll
        for (int k = 0; k < AF_CHUNK; k++) x[k] = (dead >> k) & 1u ? 0.f : x[k];
        const int cnt = min(max(L - i0, 0), AF_CHUNK);            // the lane's samples inside the stream
        const int last = min(AF_LANES - 1, (L - b0 - 1) / AF_CHUNK);  // the last lane that holds data
#pragma unroll
        for (int s = 0; s < PSDR_AUDIO_FILTER_SECTIONS; s++) {
            if (s >= nsec) break;
            const AfSection &c = e->sec[s];
            float v1, v2;
            af_chunk_zero(c, x, v1, v2);
            if (lane == 0) af_combine(c.P[0], st[2 * s], st[2 * s + 1], v1, v2);  // the carried state enters as lane -1
#pragma unroll
            for (int k = 0; k < AF_LEVELS; k++) {
                const float u1 = __shfl_up(v1, 1u << k), u2 = __shfl_up(v2, 1u << k);
                if (lane >= (1 << k)) af_combine(c.P[k], u1, u2, v1, v2);
            }
            float e1 = __shfl_up(v1, 1u), e2 = __shfl_up(v2, 1u);
            if (lane == 0) e1 = st[2 * s], e2 = st[2 * s + 1];
            af_chunk_run(c, x, cnt, e1, e2);
            st[2 * s] = __shfl(e1, last), st[2 * s + 1] = __shfl(e2, last);
        }
#pragma unroll
        for (int q = 0; q < NV; q++) {
            if ((dead >> (q * W)) & 1u) continue;  // (a piece lies in one frame, and inside the stream or behind it, as a whole)
            vec v;
#pragma unroll
            for (int k = 0; k < W; k++) v[k] = x[q * W + k];
            *(vec *)(rows + i0 + q * W) = v;
        }
    }
    if (lane == 0)
        for (int i = 0; i < 2 * PSDR_AUDIO_FILTER_SECTIONS; i++) a.state[(size_t)slot * 2 * PSDR_AUDIO_FILTER_SECTIONS + i] = st[i];
}

hipError_t audio_filter_launch(const AudioFilterArgs &a, hipStream_t s) {
    if (a.h % 4 == 0)
        hipLaunchKernelGGL(k_audio_filter<4>, dim3((unsigned)a.nlist), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL(k_audio_filter<2>, dim3((unsigned)a.nlist), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace psdr

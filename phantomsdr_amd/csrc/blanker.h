// blanker.h - the kernels of the wideband impulse blanker (include/psdr.h: psdr_ring_set_blanker).  They run on the raw ring
// in front of k_fft_pass1, on the passes' stream; the passes themselves are not touched.  Order of one call, by launches:
//   k_nb_block_max  one streaming read of the new halves (16 bytes per lane): the maximum power of every block of 256 samples
//   k_nb_ref        one wave per half: R = the minimum of its block maxima; clears the half's count and the work list
//   k_nb_list       one thread per block: the blocks that hold a sample above T, and their neighbours, go on the work list
//   k_nb_mark       listed blocks with a sample above T: the 256-bit mask of those samples, from the RAW data
//   k_nb_zero       listed blocks: the masks of the block and its neighbours, dilated by `guard`, become zeros and a count
// Every k_nb_mark is done before the first k_nb_zero stores: no block decides from samples another work-group may be zeroing.
// On a clean stream the list is empty and no sample is read a second time.  The rule's arithmetic is blankerplan.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "blankerplan.h"

namespace psdr {

struct NbArgs {
    unsigned char *ring;  // nhalves + 1 slots of hb bytes (the last mirrors slot 0)
    size_t hb;
    int nhalves, slot0, nnew;  // new half j sits in slot (slot0 + j) % nhalves
    int nblocks;               // blocks per half
    int fmt, real, guard;
    float kf;
    float *bmax;      // [nnew][nblocks]
    float *R;         // ring of rcap levels: half j at (r0 + j) % rcap
    int rcap, r0, own;
    unsigned *mask;   // [nnew][nblocks][8]
    unsigned *list;   // [nnew * nblocks]: (half * nblocks + block) | 0x80000000 if the block itself holds a sample above T
    unsigned *nlist;
    unsigned *count;  // [nnew]
};

__device__ __forceinline__ int nb_slot(const NbArgs &a, int j) { return (a.slot0 + j) % a.nhalves; }
// T of half j: kf times the level of the half before it (or its own: NbPlan::own), one f32 product
__device__ __forceinline__ float nb_T(const NbArgs &a, int j) {
    const int pos = (j == 0 && a.own) ? a.r0 : (a.r0 + j - 1 + a.rcap) % a.rcap;
    return a.kf * a.R[pos];
}

// A work-group takes tiles of 4096 bytes: thread t the t-th 16-byte chunk.  A block of 256 samples is 16 * (bytes per sample)
// consecutive chunks: 16 .. 64 lanes of one wave, or two or four whole waves.
__global__ __launch_bounds__(256) void k_nb_block_max(NbArgs a) {
    __shared__ float wmax[4];
    const int t = threadIdx.x;
    const int cpb = NB_BLOCK * nb_sample_bytes(a.fmt, a.real != 0) / NB_CHUNK;  // chunks per block: 16, 32, 64, 128 or 256
    const unsigned tph = (unsigned)(a.hb / NB_TILE), ntiles = tph * (unsigned)a.nnew;
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int j = (int)(tile / tph);
        const unsigned ti = tile % tph;
        const unsigned char *src = a.ring + (size_t)nb_slot(a, j) * a.hb + (size_t)ti * NB_TILE + (size_t)t * NB_CHUNK;
        const uint4 v = *reinterpret_cast<const uint4 *>(src);
        float m = nb_max4(0.f, v.x, v.y, v.z, v.w, a.fmt, a.real != 0);
        const int width = cpb < 64 ? cpb : 64;
        for (int o = 1; o < width; o <<= 1) m = nb_max(m, __shfl_xor(m, o, 64));
        float *out = a.bmax + (size_t)j * a.nblocks + (size_t)ti * (256 / cpb);
        if (cpb <= 64) {
            if (t % cpb == 0) out[t / cpb] = m;
        } else {
            if ((t & 63) == 0) wmax[t >> 6] = m;
            __syncthreads();
            if (cpb == 128 && t < 2) out[t] = nb_max(wmax[2 * t], wmax[2 * t + 1]);
            if (cpb == 256 && t == 0) out[0] = nb_max(nb_max(wmax[0], wmax[1]), nb_max(wmax[2], wmax[3]));
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(64) void k_nb_ref(NbArgs a) {
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= a.nnew) return;
    const float *bm = a.bmax + (size_t)j * a.nblocks;
    float r = bm[lane < a.nblocks ? lane : 0];  // (a half has at least 8 blocks; the maxima are never NaN)
    for (int b = lane + 64; b < a.nblocks; b += 64) r = (bm[b] < r) ? bm[b] : r;
    for (int o = 1; o < 64; o <<= 1) {
        const float x = __shfl_xor(r, o, 64);
        r = (x < r) ? x : r;
    }
    if (lane == 0) {
        a.R[(a.r0 + j) % a.rcap] = r;
        a.count[j] = 0u;
        if (j == 0) *a.nlist = 0u;
    }
}

__device__ __forceinline__ bool nb_block_hit(const NbArgs &a, int j, int b, float T) {
    return b >= 0 && b < a.nblocks && nb_exceed(a.bmax[(size_t)j * a.nblocks + b], T);
}

__global__ __launch_bounds__(256) void k_nb_list(NbArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.nnew * a.nblocks) return;
    const int j = (int)(i / a.nblocks), b = (int)(i % a.nblocks);
    const float T = nb_T(a, j);
    if (!nb_threshold_valid(T)) return;
    const bool self = nb_block_hit(a, j, b, T);
    if (!self && !nb_block_hit(a, j, b - 1, T) && !nb_block_hit(a, j, b + 1, T)) return;
    a.list[atomicAdd(a.nlist, 1u)] = (unsigned)i | (self ? 0x80000000u : 0u);
}

// thread = sample of the block; the four waves' ballots are the mask
__global__ __launch_bounds__(256) void k_nb_mark(NbArgs a) {
    const unsigned n = *a.nlist;
    const int t = threadIdx.x;
    const int sb = nb_sample_bytes(a.fmt, a.real != 0);
    for (unsigned k = blockIdx.x; k < n; k += gridDim.x) {
        const unsigned e = a.list[k];
        if (!(e & 0x80000000u)) continue;
        const unsigned i = e & 0x7FFFFFFFu;
        const int j = (int)(i / a.nblocks), b = (int)(i % a.nblocks);
        const float T = nb_T(a, j);
        const unsigned char *s = a.ring + (size_t)nb_slot(a, j) * a.hb + ((size_t)b * NB_BLOCK + t) * sb;
        const unsigned long long m = __ballot(nb_exceed(nb_sample_power(s, a.fmt, a.real != 0), T));
        if ((t & 63) == 0) {
            unsigned *dst = a.mask + (size_t)i * 8 + (t >> 6) * 2;
            dst[0] = (unsigned)m, dst[1] = (unsigned)(m >> 32);
        }
    }
}

__device__ __forceinline__ void nb_store_zero(unsigned char *p, int sb, unsigned z) {
    if (sb == 1) *p = (unsigned char)z;
    else if (sb == 2) *reinterpret_cast<unsigned short *>(p) = (unsigned short)z;
    else if (sb == 4) *reinterpret_cast<unsigned *>(p) = z;
    else if (sb == 8) *reinterpret_cast<uint2 *>(p) = make_uint2(z, z);
    else *reinterpret_cast<uint4 *>(p) = make_uint4(z, z, z, z);
}

__global__ __launch_bounds__(256) void k_nb_zero(NbArgs a) {
    __shared__ unsigned mk[24];  // the masks of blocks b - 1, b, b + 1: bit 256 + t is sample t of block b
    const unsigned n = *a.nlist;
    const int t = threadIdx.x;
    const int sb = nb_sample_bytes(a.fmt, a.real != 0);
    const unsigned z = nb_zero_word(a.fmt);
    for (unsigned k = blockIdx.x; k < n; k += gridDim.x) {
        const unsigned i = a.list[k] & 0x7FFFFFFFu;
        const int j = (int)(i / a.nblocks), b = (int)(i % a.nblocks);
        const float T = nb_T(a, j);
        if (t < 24) {
            const int nb = b - 1 + t / 8;  // the guard is clipped to the half: a block outside it has no mask
            mk[t] = nb_block_hit(a, j, nb, T) ? a.mask[((size_t)j * a.nblocks + nb) * 8 + t % 8] : 0u;
        }
        __syncthreads();
        const int lo = NB_BLOCK + t - a.guard, hi = NB_BLOCK + t + a.guard;  // 1 .. 766
        bool hit = false;
        for (int w = lo >> 5; w <= hi >> 5; w++) {
            unsigned bits = mk[w];
            if (w == lo >> 5) bits &= ~0u << (lo & 31);
            if (w == hi >> 5) bits &= ~0u >> (31 - (hi & 31));
            hit = hit || bits != 0u;
        }
        if (hit) {
            const int slot = nb_slot(a, j);
            const size_t off = ((size_t)b * NB_BLOCK + t) * sb;
            nb_store_zero(a.ring + (size_t)slot * a.hb + off, sb, z);
            if (slot == 0) nb_store_zero(a.ring + (size_t)a.nhalves * a.hb + off, sb, z);  // the mirror behind the last slot
        }
        const unsigned long long bal = __ballot(hit);
        if ((t & 63) == 0 && bal) atomicAdd(a.count + j, (unsigned)__popcll(bal));
        __syncthreads();
    }
}

}  // namespace psdr

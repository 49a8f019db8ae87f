// cw.hip - k_audio_cw, the kernel behind cw.h
#include "cw.h"

namespace psdr {

// lo over the ring as wave 0 holds it - value i in lane i (r0) and value 64 + i in lane i (r1) -: the value of rank CW_LO_RANK, as
// cwplan.h's cw_lo: ordered as unsigned integers on the bit patterns, ties by the lower index.  Wave-uniform result.
__device__ inline float cw_lo_wave(float r0, float r1, int lane) {
    const uint32_t u0 = tone_bits(r0), u1 = tone_bits(r1);
    int c0 = 0, c1 = 0;
#pragma unroll 8
    for (int j = 0; j < 64; j++) {
        const uint32_t v0 = (uint32_t)__builtin_amdgcn_readlane((int)u0, j), v1 = (uint32_t)__builtin_amdgcn_readlane((int)u1, j);
        c0 += ((v0 < u0 || (v0 == u0 && j < lane)) ? 1 : 0) + (v1 < u0 ? 1 : 0);
        c1 += (v0 <= u1 ? 1 : 0) + ((v1 < u1 || (v1 == u1 && j < lane)) ? 1 : 0);
    }
    const unsigned long long m0 = __ballot(c0 == CW_LO_RANK), m1 = __ballot(c1 == CW_LO_RANK);  // (exactly one bit in both)
    return m0 ? __shfl(r0, __ffsll((long long)m0) - 1) : __shfl(r1, __ffsll((long long)m1) - 1);
}

// One work-group of CW_GROUP waves per listed client, in the coordinates of cw_stream: the batch completes hops b0 .. b1 - 1.  They
// go in groups of CW_GROUP, one per wave: (1) the hop's H samples into the wave's LDS row (the carried partial hop, then the rows,
// a flagged frame as zeros), (2) lane = pitch: the correlation over the row, read as broadcasts, into the group's LDS row of
// correlations, (3) behind a barrier wave 0 takes the group's hops in order - cw_hop_step with the lanes' part done by wave
// operations - and writes the text and the records of the frames each hop ends.
__global__ __launch_bounds__(64 * CW_GROUP) void k_audio_cw(CwArgs a) {
    __shared__ __attribute__((aligned(16))) float xin[CW_GROUP][CW_HMAX];
    __shared__ ToneC Cg[CW_GROUP][CW_LANES];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    if ((int)blockIdx.x >= a.nlist) return;
    const CwEntry e = a.list[blockIdx.x];
    const size_t frow = (size_t)e.slot * a.max_batch;
    CwState *st = a.state + e.slot;
    uint8_t *text = a.text + (size_t)e.slot * CW_TEXT;
    const float *rows = a.audio + frow * a.h;
    const int *flags = a.nan_flags + frow;
    const CwTables *T = a.tab;
    const int h = a.h, H = T->H, umin = T->umin, umax = T->umax;
    // ---- what the state holds is read before anything is written
    const uint64_t pos0 = st->pos, L = (uint64_t)a.nframes * (uint64_t)h, b0 = pos0 / (uint64_t)H, b1 = (pos0 + L) / (uint64_t)H;
    ToneC cprev = st->cprev[lane];
    float A = st->A[lane], r0 = st->ring[lane], r1 = st->ring[lane + 64], hi = st->hi;
    uint64_t nchars = st->nchars;
    int p = st->lane;
    CwKey k = st->k;
    if (pos0 == 0) p = e.p0, k.u = e.u0;
    const uint32_t inc = T->t.inc[lane];
    const ToneC rot = {T->t.rot[lane][0], T->t.rot[lane][1]};
    const bool cand = (e.cand >> lane) & 1ull;
    __syncthreads();

    // the frames at whose end D hops are complete take the state as it stands (wave 0)
    auto emit = [&](uint64_t D) {
        const int lo = cw_first_frame(D, pos0, h, H), up = min(a.nframes, cw_first_frame(D + 1, pos0, h, H));
        for (int f = lo + lane; f < up; f += 64) a.rec[frow + f] = cw_record(T, D, nchars, k, p, hi);
    };
    if (w == 0) emit(b0);

    for (uint64_t bg = b0; bg < b1; bg += CW_GROUP) {
        const uint64_t b = bg + (uint64_t)w;
        const bool active = b < b1;  // (wave-uniform)
        if (active)
            for (int n = lane; n < H; n += 64) xin[w][n] = cw_sample(b * (uint64_t)H + (uint64_t)n, pos0, b0, H, st->part, rows, flags, h);
        __syncthreads();
        if (active) {
            ToneC wv = tone_seed(&T->t, tone_phase(inc, b * (uint64_t)H));
            ToneC acc = {0.f, 0.f};
            for (int n = 0; n < H; n += 4) {
                const float4 x = *(const float4 *)&xin[w][n];
                tone_step(acc, wv, rot, x.x);
                tone_step(acc, wv, rot, x.y);
                tone_step(acc, wv, rot, x.z);
                tone_step(acc, wv, rot, x.w);
            }
            Cg[w][lane] = acc;
        }
        __syncthreads();
        if (w == 0)
            for (int q = 0; q < CW_GROUP && bg + (uint64_t)q < b1; q++) {
                const uint64_t bq = bg + (uint64_t)q;
                const ToneC c = Cg[q][lane];
                const float E = cw_energy(c, cprev);
                cprev = c;
                A = cw_follow(A, E);
                // the lowest candidate with the largest A (A >= +0: a lane that is no candidate enters as 0 and is not chosen)
                const uint32_t ua = cand ? tone_bits(A) : 0u;
                uint32_t m = ua;
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
                const int qn = __ffsll((long long)__ballot(cand && ua == m)) - 1;
                if (cw_moves(__shfl(A, qn), __shfl(A, p))) p = qn;
                const float en = __shfl(E, p);
                hi = cw_hi(hi, en);
                const int i = (int)(bq % CW_RING);
                if (lane == (i & 63)) {
                    if (i < 64) r0 = en;
                    else r1 = en;
                }
                const bool full = bq + 1 >= (uint64_t)CW_RING;
                const float lo = full ? cw_lo_wave(r0, r1, lane) : 0.f;
                const int raw = cw_raw(cw_present(full, hi, lo, e.ratio), en, hi);
                for (uint32_t out = cw_key_step(k, raw, e.track, umin, umax, T->morse); out; out >>= 8) {
                    if (lane == 0) text[nchars % CW_TEXT] = (uint8_t)out;
                    nchars++;
                }
                emit(bq + 1);
            }
        __syncthreads();  // the group's correlations are read: the next group may write its own
    }
    // the new partial hop: what the batch left behind hop b1 - 1 (behind a kept partial hop the rows are appended)
    const uint64_t u = b1 * (uint64_t)H + (uint64_t)tid;
    if (u >= pos0) st->part[tid] = u < pos0 + L ? cw_sample(u, pos0, b0, H, st->part, rows, flags, h) : 0.f;
    if (w == 0) {
        st->cprev[lane] = cprev;
        st->A[lane] = A;
        st->ring[lane] = r0, st->ring[lane + 64] = r1;
        if (lane == 0) {
            st->pos = pos0 + L, st->nchars = nchars;
            st->hi = hi, st->lane = p;
            st->k = k;
        }
    }
}

hipError_t audio_cw_launch(const CwArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_audio_cw, dim3((unsigned)a.nlist), dim3(64 * CW_GROUP), 0, s, a);
    return hipGetLastError();
}

}  // namespace psdr

// rtty.hip - k_audio_rtty, the kernel behind rtty.h
#include "rtty.h"

namespace psdr {

constexpr int RTTY_LROWS = 32;  // rows of the correlations' ring in LDS: the 23 hops behind a group's first and the group's 8
static_assert(RTTY_LROWS >= RTTY_WMAX - 1 + RTTY_GROUP && (RTTY_LROWS & (RTTY_LROWS - 1)) == 0, "a group's hops overwrite nothing its windows read");

// One work-group of 256 threads per listed client, in the coordinates of rtty_stream: the batch completes hops b0 .. b1 - 1.  They
// go in groups of RTTY_GROUP; thread (g, k) = (tid / 32, tid % 32) has hop bg + g and lane k, so a wave takes two hops at once.
// (1) the hops' samples into LDS (the carried partial hop, then the rows, a flagged frame as zeros), (2) the correlation over the
// hop's row, read as float4 broadcasts, into the LDS ring of correlations, (3) behind a barrier the bit window's sum over the ring
// and its energy, (4) behind another wave 0 takes the group's hops in order - rtty_stream's loop body with the pairs' part done by
// wave operations (lane j & 15 has pair j) - and writes the text and the records of the frames each hop ends.
__global__ __launch_bounds__(32 * RTTY_GROUP) void k_audio_rtty(RttyArgs a) {
    __shared__ __attribute__((aligned(16))) float xin[RTTY_GROUP][RTTY_HMAX];
    __shared__ ToneC ring[RTTY_LROWS][RTTY_LANES];
    __shared__ float Eg[RTTY_GROUP][RTTY_LANES];
    const int tid = threadIdx.x, g = tid >> 5, k = tid & 31, lane = tid & 63;
    if ((int)blockIdx.x >= a.nlist) return;
    const RttyEntry *e = a.list + blockIdx.x;
    const int slot = e->slot, wn = e->wn;
    const size_t frow = (size_t)slot * a.max_batch;
    RttyState *st = a.state + slot;
    uint8_t *text = a.text + (size_t)slot * RTTY_TEXT;
    const float *rows = a.audio + frow * a.h;
    const int *flags = a.nan_flags + frow;
    const RttyTables *T = a.tab;
    const int h = a.h, H = T->H, hs = __ffs(H) - 1;
    // ---- what the state holds is read before anything is written
    const uint64_t pos0 = st->pos, L = (uint64_t)a.nframes * (uint64_t)h, b0 = pos0 / (uint64_t)H, b1 = (pos0 + L) / (uint64_t)H;
    RttyScalars z = {st->nchars, st->em, st->es, st->T, st->Nn, st->errors, pos0 == 0 ? RTTY_P0 : st->p, st->present, st->f};
    float A = st->A[lane & 15];
    const uint32_t inc = e->inc[k];
    const ToneC rot = {e->rot[k][0], e->rot[k][1]};
    const bool cand = (e->cand >> (lane & 15)) & 1u;
    // the hops behind b0 that a window may read: row hb % 24 of the state into row hb % 32
    for (int i = tid; i < (RTTY_WMAX - 1) * RTTY_LANES; i += 32 * RTTY_GROUP) {
        const int64_t hb = (int64_t)b0 - 1 - (i >> 5);
        if (hb >= 0) ring[hb & (RTTY_LROWS - 1)][i & 31] = st->ring[hb % RTTY_WMAX][i & 31];
    }
    __syncthreads();

    // the frames at whose end D hops are complete take the state as it stands (wave 0)
    auto emit = [&](uint64_t D) {
        const int lo = cw_first_frame(D, pos0, h, H), up = min(a.nframes, cw_first_frame(D + 1, pos0, h, H));
        for (int f = lo + lane; f < up; f += 64) a.rec[frow + f] = rtty_record(D, z.nchars, z.errors, z.p, z.em, z.es, z.T, z.Nn, z.present, e->lscale);
    };
    if (tid < 64) emit(b0);

    for (uint64_t bg = b0; bg < b1; bg += RTTY_GROUP) {
        const int cnt = (int)min((uint64_t)RTTY_GROUP, b1 - bg);
        for (int i = tid; i < cnt * H; i += 32 * RTTY_GROUP)  // (H is a power of two: i >> hs is the hop, the rest the sample)
            xin[i >> hs][i & (H - 1)] = cw_sample(bg * (uint64_t)H + (uint64_t)i, pos0, b0, H, st->part, rows, flags, h);
        __syncthreads();
        const uint64_t b = bg + (uint64_t)g;
        const bool active = g < cnt;  // (uniform over a half-wave)
        if (active) {
            ToneC wv = tone_seed(&T->t, tone_phase(inc, b * (uint64_t)H));
            ToneC acc = {0.f, 0.f};
            for (int n = 0; n < H; n += 4) {
                const float4 x = *(const float4 *)&xin[g][n];
                tone_step(acc, wv, rot, x.x);
                tone_step(acc, wv, rot, x.y);
                tone_step(acc, wv, rot, x.z);
                tone_step(acc, wv, rot, x.w);
            }
            ring[b & (RTTY_LROWS - 1)][k] = acc;
        }
        __syncthreads();
        if (active) Eg[g][k] = rtty_energy(rtty_window(b, wn, [&](uint64_t hb) { return ring[hb & (RTTY_LROWS - 1)][k]; }));
        __syncthreads();
        if (tid < 64)
            for (int q = 0; q < cnt; q++) {
                const uint64_t bq = bg + (uint64_t)q;
                const int j = lane & 15;
                A = rtty_follow(A, Eg[q][2 * j], Eg[q][2 * j + 1]);
                // the lowest candidate with the largest A (A >= +0: a pair that is no candidate enters as 0 and is not chosen)
                const uint32_t ua = cand ? tone_bits(A) : 0u;
                uint32_t m = ua;
#pragma unroll
                for (int off = 8; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
                const int qn = __ffsll((long long)__ballot(cand && ua == m)) - 1;  // (lanes 0..15 come first: qn is a pair)
                z.p = rtty_pair(z.p, qn, __shfl(A, qn), __shfl(A, z.p));
                const uint32_t out = rtty_scalar_step(z, *e, bq, Eg[q][2 * z.p], Eg[q][2 * z.p + 1], T->baudot);
                if (out) {
                    if (lane == 0) text[z.nchars % RTTY_TEXT] = (uint8_t)out;
                    z.nchars++;
                }
                emit(bq + 1);
            }
        __syncthreads();  // the group's energies and samples are read: the next group may write its own
    }
    // the new partial hop: what the batch left behind hop b1 - 1 (behind a kept partial hop the rows are appended)
    if (tid < RTTY_HMAX) {
        const uint64_t u = b1 * (uint64_t)H + (uint64_t)tid;
        if (u >= pos0) st->part[tid] = u < pos0 + L ? cw_sample(u, pos0, b0, H, st->part, rows, flags, h) : 0.f;
    }
    // the last 24 hops' correlations: the ones this batch completed go to their rows of the state
    for (int i = tid; i < RTTY_WMAX * RTTY_LANES; i += 32 * RTTY_GROUP) {
        const int64_t hb = (int64_t)b1 - 1 - (i >> 5);
        if (hb >= (int64_t)b0) st->ring[hb % RTTY_WMAX][i & 31] = ring[hb & (RTTY_LROWS - 1)][i & 31];
    }
    if (tid < 64) {
        if (lane < RTTY_PAIRS) st->A[lane] = A;
        if (lane == 0) {
            st->pos = pos0 + L, st->nchars = z.nchars;
            st->em = z.em, st->es = z.es, st->T = z.T, st->Nn = z.Nn;
            st->errors = z.errors, st->p = z.p, st->present = z.present;
            st->f = z.f;
        }
    }
}

hipError_t audio_rtty_launch(const RttyArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_audio_rtty, dim3((unsigned)a.nlist), dim3(32 * RTTY_GROUP), 0, s, a);
    return hipGetLastError();
}

}  // namespace psdr

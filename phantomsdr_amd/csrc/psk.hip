// psk.hip - k_audio_psk, the kernel behind psk.h
#include "psk.h"

namespace psdr {

constexpr int PSK_LROWS = 64;  // rows of the correlations' ring in LDS: the 31 hops behind a group's first and the group's 16
static_assert(PSK_LROWS >= PSK_WMAX - 1 + PSK_GROUP && (PSK_LROWS & (PSK_LROWS - 1)) == 0, "a group's hops overwrite nothing its windows read");
static_assert(PSK_LANES == 16 && PSK_BINS == 16, "a quarter-wave holds the lanes and the timing bins alike");

// One work-group of 256 threads per listed client, in the coordinates of psk_stream: the batch completes hops b0 .. b1 - 1.  They
// go in groups of PSK_GROUP; thread (g, k) = (tid / 16, tid % 16) has hop bg + g and lane k, so a wave takes four hops at once.
// (1) the hops' samples into LDS (the carried partial hop, then the rows, a flagged frame as zeros), (2) the correlation over the
// hop's row, read as float4 broadcasts, into the LDS ring of correlations, (3) behind a barrier the symbol window's sum over the
// ring and, over the hop's quarter-wave, the clock's energy, (4) behind another wave 0 takes the group's hops in order -
// psk_stream's loop body with the lanes' and the bins' part done by wave operations (lane j & 15 has lane j and bin j) - and
// writes the text and the records of the frames each hop ends.
__global__ __launch_bounds__(16 * PSK_GROUP) void k_audio_psk(PskArgs a) {
    __shared__ __attribute__((aligned(16))) float xin[PSK_GROUP][PSK_HMAX];
    __shared__ ToneC ring[PSK_LROWS][PSK_LANES];
    __shared__ ToneC Sg[PSK_GROUP][PSK_LANES];
    __shared__ float Tg[PSK_GROUP];
    const int tid = threadIdx.x, g = tid >> 4, k = tid & 15, lane = tid & 63;
    if ((int)blockIdx.x >= a.nlist) return;
    const PskEntry *e = a.list + blockIdx.x;
    const int slot = e->slot, wn = e->wn;
    const size_t frow = (size_t)slot * a.max_batch;
    PskState *st = a.state + slot;
    uint8_t *text = a.text + (size_t)slot * PSK_TEXT;
    const float *rows = a.audio + frow * a.h;
    const int *flags = a.nan_flags + frow;
    const PskTables *T = a.tab;
    const int h = a.h, H = T->H, hs = __ffs(H) - 1;
    // ---- what the state holds is read before anything is written
    const uint64_t pos0 = st->pos, L = (uint64_t)a.nframes * (uint64_t)h, b0 = pos0 / (uint64_t)H, b1 = (pos0 + L) / (uint64_t)H;
    PskScalars z = psk_scalars(*st);
    ToneC prev = st->prev[k];
    float Qre = st->Qre[k], G = st->G[k];
    const uint32_t inc = e->inc[k], cands = e->cand;
    const ToneC rot = {e->rot[k][0], e->rot[k][1]};
    const bool cand = (cands >> k) & 1u;
    // the hops behind b0 that a window may read: row hb % 32 of the state into row hb % 64
    for (int i = tid; i < (PSK_WMAX - 1) * PSK_LANES; i += 16 * PSK_GROUP) {
        const int64_t hb = (int64_t)b0 - 1 - (i >> 4);
        if (hb >= 0) ring[hb & (PSK_LROWS - 1)][i & 15] = st->ring[hb % PSK_WMAX][i & 15];
    }
    __syncthreads();

    // the frames at whose end D hops are complete take the state as it stands (wave 0)
    auto emit = [&](uint64_t D) {
        const int lo = cw_first_frame(D, pos0, h, H), up = min(a.nframes, cw_first_frame(D + 1, pos0, h, H));
        for (int f = lo + lane; f < up; f += 64) a.rec[frow + f] = psk_record(D, z, e->df, e->lscale);
    };
    if (tid < 64) emit(b0);

    for (uint64_t bg = b0; bg < b1; bg += PSK_GROUP) {
        const int cnt = (int)min((uint64_t)PSK_GROUP, b1 - bg);
        for (int i = tid; i < cnt * H; i += 16 * PSK_GROUP)  // (H is a power of two: i >> hs is the hop, the rest the sample)
            xin[i >> hs][i & (H - 1)] = cw_sample(bg * (uint64_t)H + (uint64_t)i, pos0, b0, H, st->part, rows, flags, h);
        __syncthreads();
        const uint64_t b = bg + (uint64_t)g;
        const bool active = g < cnt;  // (uniform over a quarter-wave)
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
            ring[b & (PSK_LROWS - 1)][k] = acc;
        }
        __syncthreads();
        if (active) {
            const ToneC S = rtty_window(b, wn, [&](uint64_t hb) { return ring[hb & (PSK_LROWS - 1)][k]; });
            Sg[g][k] = S;
            const float E = rtty_energy(S);
            // (the candidates are the same for the whole quarter-wave: every lane of it takes every step)
            const float tot = psk_clock_energy(cands, [&](int j) { return __shfl(E, (lane & 48) + j); });
            if (k == 0) Tg[g] = tot;
        }
        __syncthreads();
        if (tid < 64)
            for (int q = 0; q < cnt; q++) {
                const uint64_t bq = bg + (uint64_t)q;
                const int j = lane & 15;
                const int bin = psk_clock_bin(z, e->u);
                if (j == bin) G = psk_follow(G, Tg[q]);
                // the lowest bin with the largest G (G >= +0)
                const uint32_t ug = tone_bits(G);
                uint32_t m = ug;
#pragma unroll
                for (int off = 8; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
                const int gq = __ffsll((long long)__ballot(ug == m)) - 1;  // (lanes 0..15 come first: gq is a bin)
                if (psk_clock_sample(z, *e, gq)) {
                    const PskD d = psk_lane_step(Sg[q][j], prev, Qre);
                    // the lowest candidate with the largest M (M >= +0: a lane that is no candidate enters as 0 and is not chosen)
                    const float M = psk_merit(Qre);
                    const uint32_t um = cand ? tone_bits(M) : 0u;
                    uint32_t mm = um;
#pragma unroll
                    for (int off = 8; off >= 1; off >>= 1) mm = max(mm, (uint32_t)__shfl_xor((int)mm, off));
                    const int qn = __ffsll((long long)__ballot(cand && um == mm)) - 1;  // (lane 8 is a candidate: there is one)
                    const float Mq = __shfl(M, qn), Mp = __shfl(M, z.p);
                    psk_move(z, qn, Mq, Mp);
                    const PskD dp = {__shfl(d.re, z.p), __shfl(d.q, z.p), __shfl(d.w, z.p)};
                    const uint32_t out = psk_symbol_step(z, *e, rtty_energy(Sg[q][z.p]), dp, T->vari);
                    if (out) {
                        if (lane == 0) text[z.nchars % PSK_TEXT] = (uint8_t)out;
                        z.nchars++;
                    }
                }
                emit(bq + 1);
            }
        __syncthreads();  // the group's sums and samples are read: the next group may write its own
    }
    // the new partial hop: what the batch left behind hop b1 - 1 (behind a kept partial hop the rows are appended)
    if (tid < PSK_HMAX) {
        const uint64_t u = b1 * (uint64_t)H + (uint64_t)tid;
        if (u >= pos0) st->part[tid] = u < pos0 + L ? cw_sample(u, pos0, b0, H, st->part, rows, flags, h) : 0.f;
    }
    // the last 32 hops' correlations: the ones this batch completed go to their rows of the state
    for (int i = tid; i < PSK_WMAX * PSK_LANES; i += 16 * PSK_GROUP) {
        const int64_t hb = (int64_t)b1 - 1 - (i >> 4);
        if (hb >= (int64_t)b0) st->ring[hb % PSK_WMAX][i & 15] = ring[hb & (PSK_LROWS - 1)][i & 15];
    }
    if (tid < 64) {
        if (lane < PSK_LANES) st->prev[lane] = prev, st->Qre[lane] = Qre, st->G[lane] = G;
        if (lane == 0) psk_keep(*st, z, pos0 + L);
    }
}

hipError_t audio_psk_launch(const PskArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_audio_psk, dim3((unsigned)a.nlist), dim3(16 * PSK_GROUP), 0, s, a);
    return hipGetLastError();
}

}  // namespace psdr

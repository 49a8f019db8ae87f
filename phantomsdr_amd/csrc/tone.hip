// tone.hip - k_audio_tone, the kernel behind tone.h
#include "tone.h"

namespace psdr {

// The decision of one block over the lanes' powers (lane = tone, 50 live), as toneplan.h's tone_decide: the maximum and the rank
// are taken on the bit patterns as unsigned integers, ties go to the lower lane.  Wave-uniform result.
__device__ inline ToneDecision tone_decide_wave(float P, int lane, const ToneEntry &e, float lscale) {
    const bool live = lane < TONE_N;
    ToneDecision d = {0, 0, 0.f};
    if (__ballot(live && !tone_finite(P)) != 0ull) return d;
    const uint32_t u = live ? tone_bits(P) : 0u;
    uint32_t m = u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
    d.best = __ffsll((long long)__ballot(live && u == m)) - 1;
    // rank by counting: the lanes behind the tones hold the largest pattern and the highest indices, so they rank last
    const uint32_t ur = live ? u : 0xFFFFFFFFu;
    int rank = 0;
    for (int j = 0; j < TONE_N; j++) {
        const uint32_t uj = (uint32_t)__shfl((int)ur, j);
        rank += (uj < ur || (uj == ur && j < lane)) ? 1 : 0;
    }
    const int rl = __ffsll((long long)__ballot(live && rank == TONE_REF_RANK)) - 1;
    const float ref = __shfl(P, rl), Pbest = __shfl(P, d.best);
    d.level = tone_level(Pbest, lscale);
    d.hit = tone_hit(Pbest, ref, d.level, d.best, e) ? 1 : 0;
    return d;
}

// One work-group of TONE_GROUP waves per listed client, in the coordinates of tone_stream: the batch completes blocks b0 .. b1 - 1.
// They go in groups of TONE_GROUP, one per wave: (1) the block's 256 samples into the wave's LDS row (the carried partial block,
// then the rows, a flagged frame as zeros), (2) lane = tone: the correlation over the row, read as broadcasts, into the block's row
// of the history ring, (3) behind a barrier the window sum over the ring's last NB rows, the powers and the decision, (4) wave 0
// takes the group's decisions through the gate in block order and writes the records of the frames each block ends.  A copy entry
// (attack == 0) copies its drop flags and is done.
__global__ __launch_bounds__(64 * TONE_GROUP) void k_audio_tone(ToneArgs a) {
    __shared__ __attribute__((aligned(16))) float xin[TONE_GROUP][TONE_B];
    __shared__ ToneDecision dec[TONE_GROUP];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    if ((int)blockIdx.x >= a.nlist) return;
    const ToneEntry e = a.list[blockIdx.x];
    const size_t frow = (size_t)e.slot * a.max_batch;
    if (e.attack == 0) {
        if (a.drop)
            for (int f = tid; f < a.nframes; f += 64 * TONE_GROUP) a.drop[frow + f] = a.prev_drop[frow + f];
        return;
    }
    ToneState *st = a.state + e.slot;
    ToneC *hist = a.hist + (size_t)e.slot * a.ring * TONE_LANES;
    const float *rows = a.audio + frow * a.h;
    const int *flags = a.nan_flags + frow;
    const ToneTables *T = a.tab;
    const int h = a.h, nb = T->nb, ring = a.ring;
    const float lscale = T->lscale;
    // ---- what the state holds is read before anything is written
    const uint64_t pos0 = st->pos, L = (uint64_t)a.nframes * (uint64_t)h, b0 = pos0 / TONE_B, b1 = (pos0 + L) / TONE_B;
    SquelchState g = {st->open, st->cnt};
    int tp1 = st->tone_plus1;
    float level = st->level;
    const uint32_t inc = T->inc[lane];
    const ToneC rot = {T->rot[lane][0], T->rot[lane][1]};
    __syncthreads();

    // the frames at whose end D blocks are complete take the state as it stands (wave 0)
    auto emit = [&](uint64_t D) {
        const int lo = tone_first_frame(D, pos0, h), hi = min(a.nframes, tone_first_frame(D + 1, pos0, h));
        for (int f = lo + lane; f < hi; f += 64) {
            a.rec[frow + f] = tone_record(g, tp1, level);
            if (a.drop) a.drop[frow + f] = tone_drop(a.prev_drop[frow + f], e.gate, g.open);
        }
    };
    if (w == 0) emit(b0);

    int bm = (int)(b0 % (uint64_t)ring);  // the ring row of the group's first block
    for (uint64_t bg = b0; bg < b1; bg += TONE_GROUP) {
        const uint64_t b = bg + (uint64_t)w;
        const bool active = b < b1;  // (wave-uniform)
        if (active) {
#pragma unroll
            for (int r = 0; r < TONE_B / 64; r++) xin[w][lane + 64 * r] = tone_sample(b * TONE_B + (uint64_t)(lane + 64 * r), pos0, b0, st->part, rows, flags, h);
        }
        __syncthreads();
        int myrow = bm + w;  // (ring >= TONE_GROUP: one step back is enough)
        if (myrow >= ring) myrow -= ring;
        if (active) {
            ToneC wv = tone_seed(T, tone_phase(inc, b * TONE_B));
            ToneC acc = {0.f, 0.f};
            for (int n = 0; n < TONE_B; n += 4) {
                const float4 x = *(const float4 *)&xin[w][n];
                tone_step(acc, wv, rot, x.x);
                tone_step(acc, wv, rot, x.y);
                tone_step(acc, wv, rot, x.z);
                tone_step(acc, wv, rot, x.w);
            }
            hist[(size_t)myrow * TONE_LANES + lane] = acc;
        }
        __syncthreads();  // the group's rows of the ring are written: a block's window may hold its neighbours'
        ToneDecision d = {-1, 0, 0.f};
        if (active && b + 1 >= (uint64_t)nb) {
            int j0 = myrow - (nb - 1);
            if (j0 < 0) j0 += ring;
            ToneC S = {0.f, 0.f};
            for (int j = 0; j < nb; j++) {
                tone_window_step(S, T->h[j], hist[(size_t)j0 * TONE_LANES + lane]);
                j0 = j0 + 1 == ring ? 0 : j0 + 1;
            }
            d = tone_decide_wave(tone_power(S), lane, e, lscale);
        }
        if (lane == 0) dec[w] = d;
        __syncthreads();
        if (w == 0)
            for (int q = 0; q < TONE_GROUP && bg + (uint64_t)q < b1; q++) {
                const ToneDecision dq = dec[q];
                if (dq.hit >= 0) tone_gate(g, tp1, level, dq.hit, dq.best, dq.level, e);
                emit(bg + (uint64_t)q + 1);
            }
        bm += TONE_GROUP;
        if (bm >= ring) bm -= ring;
    }
    // the new partial block: what the batch left behind block b1 - 1 (behind a kept partial block the rows are appended)
    const uint64_t u = b1 * TONE_B + (uint64_t)tid;
    if (u >= pos0) st->part[tid] = u < pos0 + L ? tone_sample(u, pos0, b0, st->part, rows, flags, h) : 0.f;
    if (tid == 0) {
        st->pos = pos0 + L;
        st->open = g.open, st->cnt = g.cnt;
        st->tone_plus1 = tp1, st->level = level;
    }
}

hipError_t audio_tone_launch(const ToneArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_audio_tone, dim3((unsigned)a.nlist), dim3(64 * TONE_GROUP), 0, s, a);
    return hipGetLastError();
}

}  // namespace psdr

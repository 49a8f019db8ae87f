// noise.h - k_noise_floor: the per-client noise floor behind a batch's last demodulation kernel (include/psdr.h:
// psdr_client_set_noise_floor), a sibling of the auto-notch detector (demod.h: k_notch_detect).  It reads the raw spectrum bins
// of a client's window through the batch's layout, keeps the per-bin power sums and the ring of evaluations, and writes the
// frames' noise power W - what psdr_read_noise delivers and what k_squelch (squelch.h), launched behind it, compares a
// noise-referenced client's pwr against.  The FFT passes and the demodulation kernels are not touched.  Every step of the rule is
// noiseplan.h's text, shared with the host.
#pragma once
#include <hip/hip_runtime.h>

#include "demod.h"
#include "noiseplan.h"

namespace psdr {

struct NoiseArgs {
    const NoiseEntry *list;  // the batch's table (noiseplan.h): slot and window of every noise-floor client
    int nlist;
    float *acc;         // [slots][n]: the power sums since the last evaluation
    NoiseState *state;  // [slots]
    float *W;           // [slots][max_batch]: the frames' noise power, of this batch
    int period;         // max(1, audio_rate / audio_fft_size) frames
};

// One wave (one work-group of 64 threads) per listed client.  Lane i owns the bins t = i + 64 j in every loop - the sums, the
// selection's counts and the restart - so a lane only ever reads what it wrote itself, and the lanes meet in ballots alone.  A run
// of frames up to the next evaluation is summed per bin with the frames in the inner loop (k_notch_detect's order: a bin's sum
// grows in frame order, whatever the batch split).  The selection walks the 32 bits of the answer from the top: per bit one
// ballot and population count per 64 bins.  The state is wave-uniform; lane 0 stores it.
__global__ __launch_bounds__(64) void k_noise_floor(DemodArgs a, NoiseArgs na) {
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= na.nlist) return;
    NoiseEntry e = na.list[blockIdx.x];
    e.slot = __builtin_amdgcn_readfirstlane(e.slot);
    e.l = __builtin_amdgcn_readfirstlane(e.l);
    e.r = __builtin_amdgcn_readfirstlane(e.r);
    const int len = e.r - e.l;
    float *W = na.W + (size_t)e.slot * a.max_batch;
    if (len <= 0) {  // nothing is added, the state stands
        for (int f = lane; f < a.nframes; f += 64) W[f] = 0.f;
        return;
    }
    float *acc = na.acc + (size_t)e.slot * a.n;  // (len <= n: psdr_client_set_audio_range)
    NoiseState st = na.state[e.slot];
    st.fill = __builtin_amdgcn_readfirstlane(st.fill);
    st.pos = __builtin_amdgcn_readfirstlane(st.pos);
    st.cnt = __builtin_amdgcn_readfirstlane(st.cnt);
    if ((unsigned)st.cnt >= (unsigned)na.period) st.cnt = 0;  // (never so: the runs below must advance whatever the memory holds)
    int f = 0;
    while (f < a.nframes) {
        const int fe = min(a.nframes, f + na.period - st.cnt);
        for (int t = lane; t < len; t += 64) {
            const cf *S = a.spec + a.lay.pos(e.l + t);
            float s = acc[t];
            for (int g = f; g < fe; g++) {
                const cf v = S[(size_t)g * a.spec_stride];
                s += noise_bin_power(v.x, v.y);
            }
            acc[t] = s;
        }
        const float before = noise_window_power(noise_estimate(st), len);
        st.cnt += fe - f;
        const bool evaluate = st.cnt >= na.period;
        if (evaluate) {
            const uint32_t q = noise_select(noise_rank(len), [&](uint32_t prefix, uint32_t mask) {
                int c = 0;
                for (int t0 = 0; t0 < len; t0 += 64) {
                    const int t = t0 + lane;
                    const bool hit = t < len && (noise_bits(acc[t]) & mask) == prefix;
                    c += __popcll(__ballot(hit));
                }
                return c;
            });
            noise_push(st, noise_entry(noise_float(q), na.period));
            for (int t = lane; t < len; t += 64) acc[t] = 0.f;
            st.cnt = 0;
        }
        const float after = noise_window_power(noise_estimate(st), len);
        for (int g = f + lane; g < fe; g += 64) W[g] = (evaluate && g == fe - 1) ? after : before;
        f = fe;
    }
    if (lane == 0) na.state[e.slot] = st;
}

}  // namespace psdr

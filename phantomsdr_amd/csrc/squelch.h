// squelch.h - k_squelch: the per-client level gate behind a batch's last demodulation kernel (include/psdr.h:
// psdr_client_set_squelch).  It reads what the demodulation kernels left - pwr and the NaN flags - and writes the frames' open
// flags, the gate's carried state and, for a post-chain batch, the drop flags the chain's k_pc_index reads in place of the NaN
// flags.  The demodulator is not touched.  The rule itself is squelchplan.h's squelch_step, shared with the host.  A
// noise-referenced client (psdr_client_set_squelch_reference) compares against its thresholds times the frame's noise power W,
// which k_noise_floor (noise.h) has written in front of this kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "squelchplan.h"

namespace psdr {

struct SquelchArgs {
    const SquelchEntry *list;  // the batch's table (squelchplan.h): squelch clients, then the chain's other audio clients
    int nlist;
    const float *pwr;      // [slots][max_batch], of this batch
    const int *nan_flags;  // ...
    int *open;             // [slots][max_batch]: 1 = the frame is heard
    int *drop;             // [slots][max_batch]: nan | !open (a copy entry: nan); null: no post chain behind this batch
    SquelchState *state;   // [slots]
    const float *noise;    // [slots][max_batch]: the batch's noise power rows W (noise.h); null: no client of the batch is noise-referenced
    int nframes, max_batch;
};

// One wave per listed client.  Frames go in chunks of 64: lane = frame loads pwr and the NaN flag, the two comparisons become
// two ballots, the state machine walks the chunk's masks in scalar code, and every lane stores its frame's flags.
__global__ __launch_bounds__(64) void k_squelch(SquelchArgs a) {
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= a.nlist) return;
    SquelchEntry e = a.list[blockIdx.x];
    e.slot = __builtin_amdgcn_readfirstlane(e.slot);
    e.attack = __builtin_amdgcn_readfirstlane(e.attack);
    e.hang = __builtin_amdgcn_readfirstlane(e.hang);
    const size_t row = (size_t)e.slot * a.max_batch;
    if (e.attack == 0) {  // no squelch: the chain drops what the NaN guard drops
        if (a.drop)
            for (int f = lane; f < a.nframes; f += 64) a.drop[row + f] = a.nan_flags[row + f];
        return;
    }
    SquelchState st = a.state[e.slot];
    st.open = __builtin_amdgcn_readfirstlane(st.open);
    st.cnt = __builtin_amdgcn_readfirstlane(st.cnt);
    const bool relative = __builtin_amdgcn_readfirstlane(e.pad) != 0 && a.noise != nullptr;
    for (int f0 = 0; f0 < a.nframes; f0 += 64) {
        const int f = f0 + lane;
        const bool in = f < a.nframes;
        const float p = in ? a.pwr[row + f] : 0.f;
        const int nf = in ? a.nan_flags[row + f] : 0;
        float t_open = e.t_open, t_close = e.t_close;
        if (relative) {  // (wave-uniform)
            const float w = in ? a.noise[row + f] : 0.f;
            t_open = squelch_relative(e.t_open, w), t_close = squelch_relative(e.t_close, w);
        }
        const unsigned long long ge_open = __ballot(in && squelch_ge(p, t_open)), ge_close = __ballot(in && squelch_ge(p, t_close));
        const unsigned long long heard = squelch_walk(st, ge_open, ge_close, min(64, a.nframes - f0), e.attack, e.hang);
        if (in) {
            const int o = (int)((heard >> lane) & 1ull);
            a.open[row + f] = o;
            if (a.drop) a.drop[row + f] = (nf != 0 || !o) ? 1 : 0;
        }
    }
    if (lane == 0) a.state[e.slot] = st;  // (the state is wave-uniform: every lane holds the state behind the batch's last frame)
}

}  // namespace psdr

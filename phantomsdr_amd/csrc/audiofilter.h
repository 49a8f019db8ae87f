// audiofilter.h - the launch of k_audio_filter (audiofilter.hip): the per-client biquad cascade on the audio rows, behind a batch's last demodulation kernel and in
// front of the post chain (include/psdr.h: psdr_client_set_audio_filter).  It filters the rows in place and carries the sections'
// state; no other kernel knows of it.  The arithmetic - step, zero-state pass, combine, true pass - is audiofilterplan.h's,
// shared with the host; audiofilter.hip is the wave's side of it: loads, the scan's lane exchange, stores.  The kernel has a
// translation unit of its own: beside the demodulation kernels in demod.hip it moved their register allocation
// (tests/test_notch_host.py pins k_demod_chain_fixed<360> at the 77 VGPRs of before the notches).
#pragma once
#include <hip/hip_runtime.h>

#include "audiofilterplan.h"

namespace psdr {

struct AudioFilterArgs {
    const AfEntry *list;   // the batch's table (audiofilterplan.h)
    int nlist;
    float *audio;          // [slots][max_batch][h], of this batch
    const int *nan_flags;  // [slots][max_batch]
    float *state;          // [slots][2 sections][2]
    int nframes, max_batch, h;
};

// one wave per listed client on `s`; the 16-byte form where h % 4 == 0, else the 8-byte form (h is even)
hipError_t audio_filter_launch(const AudioFilterArgs &a, hipStream_t s);

}  // namespace psdr

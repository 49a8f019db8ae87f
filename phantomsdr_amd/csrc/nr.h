// nr.h - the launch of k_audio_nr (nr.hip): the per-client noise reduction on the audio rows, behind a batch's last demodulation
// kernel and in front of k_audio_filter and the post chain (include/psdr.h: psdr_client_set_noise_reduction).  It works on the rows
// in place and carries each client's NrState; no other kernel knows of it.  The arithmetic - windows, butterflies, the bins' gain
// rule, the overlap-add - is nrplan.h's, shared with the host; nr.hip is the work-group's side of it: loads, the exchanges between
// the stages, stores.  The kernel has a translation unit of its own, as k_audio_filter has and for its reason.
#pragma once
#include <hip/hip_runtime.h>

#include "nrplan.h"

namespace psdr {

constexpr int NR_WAVES = 4;  // blocks of a stream that a work-group transforms at once, one per wave

struct NrArgs {
    const NrEntry *list;   // the batch's table (nrplan.h)
    int nlist;
    const NrTables *tab;   // window and twiddles
    float *audio;          // [slots][max_batch][h], of this batch
    const int *nan_flags;  // [slots][max_batch]
    NrState *state;        // [slots]
    int nframes, max_batch, h;
};

// one work-group of NR_WAVES waves per listed client on `s`; the 16-byte form where h % 4 == 0, else the 8-byte form (h is even)
hipError_t audio_nr_launch(const NrArgs &a, hipStream_t s);

}  // namespace psdr

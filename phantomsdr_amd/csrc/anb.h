// anb.h - the launch of k_audio_nb (anb.hip): the per-client audio blanker on the audio rows, behind a batch's last demodulation
// kernel and in front of k_audio_nr, k_audio_filter and the post chain (include/psdr.h: psdr_client_set_audio_blanker).  It works
// on the rows in place and carries each client's AnbState; no other kernel knows of it.  The arithmetic - autocorrelation,
// Levinson-Durbin, residual, matched filter, threshold, gap repair - is anbplan.h's, shared with the host; anb.hip is the
// work-group's side of it: loads, wave reductions, the scan by ballot, stores.  The kernel has a translation unit of its own, as
// k_audio_nr has and for its reason.
#pragma once
#include <hip/hip_runtime.h>

#include "anbplan.h"

namespace psdr {

constexpr int ANB_WAVES = 4;  // blocks of a stream that a work-group derives at once, one per wave

struct AnbArgs {
    const AnbEntry *list;  // the batch's table (anbplan.h)
    int nlist;
    float *audio;          // [slots][max_batch][h], of this batch
    const int *nan_flags;  // [slots][max_batch]
    AnbState *state;       // [slots]
    int nframes, max_batch, h;
};

// one work-group of ANB_WAVES waves per listed client on `s`; the 16-byte form where h % 4 == 0, else the 8-byte form (h is even)
hipError_t audio_nb_launch(const AnbArgs &a, hipStream_t s);

}  // namespace psdr

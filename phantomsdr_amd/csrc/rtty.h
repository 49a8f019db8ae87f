// rtty.h - the launch of k_audio_rtty (rtty.hip): the per-client RTTY decoder on the audio rows, at the tone and CW decoders'
// reading point - behind a batch's last demodulation kernel and k_squelch, in front of k_audio_nb, k_audio_nr, k_audio_filter and
// the post chain (include/psdr.h: psdr_client_set_rtty_decoder).  It reads the rows and never writes them; it carries each client's
// RttyState and text ring and writes the frames' records.  The arithmetic - twiddles, hop correlation, bit window, follower,
// slicer, presence, framing, records, the frames of a hop - is rttyplan.h's, shared with the host; rtty.hip is the work-group's
// side of it: loads, the arg-max over the pairs, stores.  The kernel has a translation unit of its own, as k_audio_cw has.
#pragma once
#include <hip/hip_runtime.h>

#include "rttyplan.h"

namespace psdr {

struct RttyArgs {
    const RttyEntry *list;  // the batch's table (rttyplan.h)
    int nlist;
    const RttyTables *tab;
    const float *audio;    // [slots][max_batch][h], of this batch
    const int *nan_flags;  // [slots][max_batch]
    RttyState *state;      // [slots]
    uint8_t *text;         // [slots][RTTY_TEXT]
    RttyRec *rec;          // [slots][max_batch]
    int nframes, max_batch, h;
};

// one work-group of RTTY_GROUP / 2 waves per listed client on `s`
hipError_t audio_rtty_launch(const RttyArgs &a, hipStream_t s);

}  // namespace psdr

// cw.h - the launch of k_audio_cw (cw.hip): the per-client CW decoder on the audio rows, at the tone decoder's reading point -
// behind a batch's last demodulation kernel and k_squelch, in front of k_audio_nb, k_audio_nr, k_audio_filter and the post chain
// (include/psdr.h: psdr_client_set_cw_decoder).  It reads the rows and never writes them; it carries each client's CwState and text
// ring and writes the frames' records.  The arithmetic - twiddles, hop correlation, energies, follower, levels, keying, records, the
// frames of a hop - is cwplan.h's, shared with the host; cw.hip is the work-group's side of it: loads, the arg-max and the rank over
// the lanes, stores.  The kernel has a translation unit of its own, as k_audio_tone has.
#pragma once
#include <hip/hip_runtime.h>

#include "cwplan.h"

namespace psdr {

struct CwArgs {
    const CwEntry *list;  // the batch's table (cwplan.h)
    int nlist;
    const CwTables *tab;
    const float *audio;    // [slots][max_batch][h], of this batch
    const int *nan_flags;  // [slots][max_batch]
    CwState *state;        // [slots]
    uint8_t *text;         // [slots][CW_TEXT]
    CwRec *rec;            // [slots][max_batch]
    int nframes, max_batch, h;
};

// one work-group of CW_GROUP waves per listed client on `s`
hipError_t audio_cw_launch(const CwArgs &a, hipStream_t s);

}  // namespace psdr

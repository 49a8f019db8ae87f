// psk.h - the launch of k_audio_psk (psk.hip): the per-client PSK31 decoder on the audio rows, at the tone, CW and RTTY decoders'
// reading point - behind a batch's last demodulation kernel and k_squelch, in front of k_audio_nb, k_audio_nr, k_audio_filter and
// the post chain (include/psdr.h: psdr_client_set_psk_decoder).  It reads the rows and never writes them; it carries each client's
// PskState and text ring and writes the frames' records.  The arithmetic - twiddles, hop correlation, symbol window, clock,
// differential detection, carrier follower, presence, varicode, records, the frames of a hop - is pskplan.h's, shared with the
// host; psk.hip is the work-group's side of it: loads, the two arg-maxes over the lanes, stores.  The kernel has a translation
// unit of its own, as k_audio_rtty has.
#pragma once
#include <hip/hip_runtime.h>

#include "pskplan.h"

namespace psdr {

struct PskArgs {
    const PskEntry *list;  // the batch's table (pskplan.h)
    int nlist;
    const PskTables *tab;
    const float *audio;    // [slots][max_batch][h], of this batch
    const int *nan_flags;  // [slots][max_batch]
    PskState *state;       // [slots]
    uint8_t *text;         // [slots][PSK_TEXT]
    PskRec *rec;           // [slots][max_batch]
    int nframes, max_batch, h;
};

// one work-group of PSK_GROUP / 4 waves per listed client on `s`
hipError_t audio_psk_launch(const PskArgs &a, hipStream_t s);

}  // namespace psdr

// tone.h - the launch of k_audio_tone (tone.hip): the per-client tone decoder on the audio rows, behind a batch's last
// demodulation kernel and k_squelch and in front of k_audio_nb, k_audio_nr, k_audio_filter and the post chain (include/psdr.h:
// psdr_client_set_tone_decoder).  It reads the rows and never writes them; it carries each client's ToneState and history ring and
// writes the frames' records and, for a post-chain batch with gated clients, the drop flags the chain reads.  The arithmetic -
// twiddles, block correlation, window sum, level, hit, gate, the frames of a block - is toneplan.h's, shared with the host;
// tone.hip is the work-group's side of it: loads, the maximum and the rank over the lanes, stores.  The kernel has a translation
// unit of its own, as k_audio_nr has and for its reason.
#pragma once
#include <hip/hip_runtime.h>

#include "toneplan.h"

namespace psdr {

struct ToneArgs {
    const ToneEntry *list;  // the batch's table (toneplan.h): tone clients, then the chain's other audio clients
    int nlist;
    const ToneTables *tab;
    const float *audio;     // [slots][max_batch][h], of this batch
    const int *nan_flags;   // [slots][max_batch]
    ToneState *state;       // [slots]
    ToneC *hist;            // [slots][tone_ring(nb)][64]
    ToneRec *rec;           // [slots][max_batch]
    const int *prev_drop;   // [slots][max_batch]: what the chain would have read without the decoder (NaN flags, or the squelch's drop flags)
    int *drop;              // [slots][max_batch]: prev | (gate && !open); null: the chain does not read it
    int nframes, max_batch, h, ring;
};

// one work-group of TONE_GROUP waves per listed client on `s`
hipError_t audio_tone_launch(const ToneArgs &a, hipStream_t s);

}  // namespace psdr

// fax.h - the launch of k_audio_fax (fax.hip): the per-client radiofax decoder on the audio rows, at the tone, CW, RTTY and PSK
// decoders' reading point - behind a batch's last demodulation kernel and k_squelch, in front of k_audio_nb, k_audio_nr,
// k_audio_filter and the post chain (include/psdr.h: psdr_client_set_fax_decoder).  It reads the rows and never writes them; it
// carries each client's FaxState and line ring and writes the frames' records.  The arithmetic - twiddles, discriminator, line and
// column, pixel, tone blocks, machine, the phasing search's decision, records, the frames of a hop - is faxplan.h's, shared with
// the host; fax.hip is the work-group's side of it: loads, the chunk's samples and pixels in parallel, the search's sums, stores.
// The kernel has a translation unit of its own, as k_audio_psk has.
#pragma once
#include <hip/hip_runtime.h>

#include "faxplan.h"

namespace psdr {

struct FaxArgs {
    const FaxEntry *list;  // the batch's table (demodplan.h)
    int nlist;
    const FaxTables *tab;
    const float *audio;    // [slots][max_batch][h], of this batch
    const int *nan_flags;  // [slots][max_batch]
    FaxState *state;       // [slots]
    uint8_t *ring;         // [slots][rmax][FAX_WIDTH_MAX] bytes; a client's R <= rmax lines of its width lie packed at the front
    uint32_t *meta;        // [slots][rmax]
    FaxRec *rec;           // [slots][max_batch]
    int nframes, max_batch, h, rmax;
};

// one work-group of four waves per listed client on `s`
hipError_t audio_fax_launch(const FaxArgs &a, hipStream_t s);

}  // namespace psdr

// types.h - plain parameter structs shared by the host translation units and the kernels (no device code: every .hip
// of the library includes this; the kernel headers are included by exactly one translation unit each)
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace psdr {

#define PSDR_MAX_STAGES 12

struct ClientParams {
    int l, r;       // [l, r) in client bin coordinates
    int m_floor;    // floor(audio_mid)
    int mode;       // psdr_mode
    int slot;       // persistent slot (state + output rows)
    int state_cur;  // which half of the double-buffered state is current
    int agc_reset;  // post chain: 1 = the demodulation changed since the last batch (AGC::reset),
                    // 2 = a new client took this slot (all chain state starts from zero)
    int paused;     // psdr_client_set_paused: listed BEHIND the batch's active clients, for the post chain only (its
                    // double-buffered streams must carry the client's history across the batch it sits out)
};

// a tuned client (demod.h: k_demod_chain_ft / k_demod_ola_ft), beside its ClientParams in the tuned clients' list
struct FtClient {
    unsigned phi0, step;  // phase of sample 0 of the batch's frame 0; phase step per audio sample (units of 2^-32 turn)
    int l, r;             // the whole window [l, r): pwr (ClientParams::l, r: the range that is placed)
};

// a sideband SAM client (demod.h: k_demod_chain_sbsam / k_demod_ola_sbsam), beside its ClientParams in the sideband SAM
// clients' list
struct SbClient {
    int l, r;   // the whole window [l, r): carrier and pwr (ClientParams::l, r: the range that is placed, clipped to the sideband)
    int side;   // psdr_sam_sideband: PSDR_SAM_UPPER or PSDR_SAM_LOWER
    int pad;
};

// floats of padding behind every slot's stream rows: the recurrence kernels' loader waves read whole blocks of 16 ahead of
// the stream's end (rings of 12 register sets: postchain.h PC_MA_RING, PC_GAIN_RING)
#define PSDR_PC_PAD (16 * 20)

// One slot's AGC profile as the chain's kernels read it (agcplan.h; include/psdr.h: psdr_client_set_agc_profile): the f32 numbers
// of the rule, rounded once on the host.  The batch's table holds one entry per slot, `on` = 0 where the slot has no profile
// (the kernels then take PostArgs::desired / attack / release).
struct alignas(16) AgcEntry {
    float desired, att, rel;  // target level, attack and release coefficients
    float cap;                // upper bound of the wanted gain, +Inf: none
    float manual_gain;        // the wanted gain of every sample where manual != 0
    int on, manual, pad;
};
static_assert(sizeof(AgcEntry) == 32, "the device table's layout: two 16-byte loads per lane");

struct PostArgs {
    const ClientParams *clients;  // this batch's list: the active clients, then the paused ones (empty streams)
    const int *slot_ci;           // [slots] index into `clients` of the slot's client, -1 = not listed in this batch
    int nact, nframes, max_batch, h;  // h = n/2 samples per frame
    int slots;
    int D, L;                         // DC delay, AGC look-ahead (samples)
    float desired, attack, release;   // AGC
    const float *audio;               // [slots][max_batch][h]
    const int *nan_flags;             // [slots][max_batch]
    int *fstart;                      // [slots][max_batch] stream offset of a frame, -1 = dropped
    int *len;                         // [slots] samples of this batch's stream
    // The streams are LANE-INTERLEAVED per group of 64 slots (round 5; postchain.h pc_at): sample t of slot s sits at
    // float ((s >> 6) * pitch + (t >> 2) * 4) * 64 + (s & 63) * 4 + (t & 3) - a wave whose lane l owns slot 64 g + l
    // reads four samples of each of its clients with ONE contiguous 1 KiB access.
    size_t px, pv;                    // pitches (floats per slot, multiples of 4) of X / M1 and of V1 / P / S
    int vo;                           // V1 / P / S: leading pad so that sample 0's row (row L-1) is a multiple of 4
    float *X, *Xn;                    // demodulated audio, rows < D history (D + T + pad); Xn: the NEXT batch's set
    float *M1, *M1n;                  // first moving average, rows < D history
    float *V1, *V1n;                  // DC-blocked stream, rows < L-1 history (L-1 + T + pad)
    float *P, *S;                     // like V1: P = prefix maxima of |V1| per row, then g_t; S = w_t (both at sample t's row vo + L-1 + t)
    float *SM;                        // [groups][sub-blocks][64] maxima of whole sub-blocks (look-ahead longer than one sub-block)
    int sb, nsub;                     // sub-block length (rows), sub-blocks per look-ahead block of L rows
    int32_t *pcm;                     // [slots][max_batch][h] (pcm16: the same rows as int16, in the front half of the buffer)
    int pcm16;                        // PSDR_OPT_POST_CHAIN_PCM16: the output kernels store int16 instead of int32
    // carried state
    float *dc_s1, *dc_s2;             // [slots] running sums
    float *agc_gain;
    int *agc_n0;  // samples pushed since the last reset, saturating at L
    int ma_fused;  // k_pc_ma2 keeps M1's history itself (k_pc_history leaves M1 alone)
    int lanes;     // k_pc_ma2 / k_pc_gain / k_pc_agc: slots per work-group (16, 32 or 64 lanes of its waves in use)
    // the AGC behind chunk maxima (k_pc_cm / k_pc_cscan / k_pc_agc, postchain.h): [groups of 64 slots][nch chunks of 16 floats][64]
    float *CM, *CP, *CS;  // maxima of |V1| per chunk; prefix / suffix maxima of CM inside blocks of L/16 - 1 chunks
    int nch;
    int *falive;          // [groups][max_batch][64] the k-th surviving frame of a slot's stream (k_pc_index)
    unsigned h_magic;     // ceil(2^32 / h): stream position / h by one multiplication
    int direct;           // k_pc_ma2 may read a work-group's new samples from `audio` itself (k_pc_gather4 then skips it)
    int32_t *pcm_dump;    // 16 bytes per thread of a k_pc_agc work-group: where its unconditional stores of row groups without a sample go
    const AgcEntry *agc_tab;  // [slots] the batch's AGC profiles, null: no client of the batch has one (the kernels without the
                              // table are launched: k_pc_want, k_pc_gain<., .>, k_pc_agc<., .> instead of k_pc_want_prof and the
                              // PcWithProfiles instantiations)
};

struct WfClient {
    int level, l, r;
    int active;
    size_t qoff;     // byte offset of `level` inside a frame's level-major int8 buffer
    size_t out_off;  // byte offset of this client's output block
    int det;         // psdr_wf_detector of the batch: k_waterfall_hold writes the rows of the clients with det != 0
    int vec;         // k_waterfall_hold: four consecutive values of the level, from a multiple of four on, are one aligned dword
};

// k_waterfall_hold / k_waterfall_carry (epilogue.h): the waterfall detectors' view of a batch and of the carry, the
// reduction of the run's frames behind its last sent frame.  The carry mirrors a frame's raw record buffers byte for
// byte: [0, lenA) the tiled records (Qt), behind them bytes [qB0, qB0 + lenB) of the level-major buffer (Q) - the levels
// above tiled_lt, widened to whole 16-byte pieces.
struct WfHoldArgs {
    const int8_t *Q, *Qt;
    size_t q_stride, qt_stride;
    size_t lenA, qB0, lenB;
    int8_t *peak;    // [lenA + lenB] element-wise maximum
    uint32_t *sum;   // [lenA + lenB] element-wise sum of (q + 128): no sign to carry, 255 * 2^24 frames fit
    int carry_n;     // frames the carry stands for when the kernel starts
    int skip;        // skip_num
    int nframes;     // frames of the batch
};

}  // namespace psdr

// postplan.h - the FORM of the post-demodulation chain (postchain.h), resolved in one pure function: which kernels a batch
// gets, with what grids, dynamic LDS and streams, from the audio rate, the frame size, the slot count and the options.
// Plain host C++17 (no HIP): postchain.hip allocates and launches from the plan, tests/test_post_plan.py prints it.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "types.h"

namespace psdr {

// what the form depends on
struct PcFacts {
    int audio_rate = 0;
    int n = 0;  // audio FFT size: h = n / 2 samples per frame
    int max_batch = 1;
    int slots = 0;
    bool piped = false;  // the context owns its side stream and the chain's streams exist: the chain is a pipeline across batches
    int opt_pc_agc = 1, opt_pc_pcm16 = 0, opt_pc_streams = 0;  // PSDR_OPT_POST_CHAIN_AGC / _PCM16 / _STREAMS
};

// the tuning overrides (PSDR_PC_* of a tuning build: postchain.hip pc_knobs), each unset by default
constexpr int PC_UNSET = INT_MIN;
struct PcKnobs {
    int lanes = PC_UNSET;       // PSDR_PC_LANES: 16 or 32 slots per recurrence work-group, anything else 64
    int reserve = PC_UNSET;     // PSDR_PC_RESERVE: CUs the passes leave free (rounded down to a multiple of 8)
    int own = PC_UNSET;         // PSDR_PC_OWN: the recurrence waves allocate a whole SIMD's registers, or not
    int fused = PC_UNSET;       // PSDR_PC_FUSED = 0: the five-kernel AGC even where the one-kernel form applies
    int cmw = PC_UNSET;         // PSDR_PC_CMW = 0: no third wave of the moving averages (k_pc_cm over the whole stream)
    int direct = PC_UNSET;      // PSDR_PC_DIRECT = 0: the moving averages read the gathered copy
    int streams = PC_UNSET;     // PSDR_PC_STREAMS: 1 the peak kernels behind the moving averages, 2 both chain streams on
                                // neighbouring queues, 3 the peak kernels on a stream of their own
    int split_peak = PC_UNSET;  // PSDR_PC_SPLIT_PEAK = 0: the prefix maxima stay in front of w_t
    int pick = PC_UNSET;        // PSDR_PC_PICK: the chain's streams chosen by measurement, or not
    int skip = PC_UNSET;        // PSDR_PC_SKIP: bit mask of chain kernels NOT launched - wrong results, a timing bound of what each
                                // costs the step: 1 gather, 2 moving averages, 4 history, 8 sub-block / chunk maxima, 16 prefix
                                // maxima / chunk scans, 32 w_t, 64 gain / k_pc_agc, 128 int16 output / k_pc_zero
};

enum PcVerdict { PC_OK, PC_RATE_TOO_SMALL, PC_RATE_UNSUPPORTED, PC_NO_FRAME };
// the DC blocker's two moving averages (postchain.h):
//   MA2_CMW  k_pc_ma2<true, true>: D = 32, a third wave leaves the chunk maxima of the new samples for k_pc_agc
//   MA2      k_pc_ma2<own>: D = 32, two waves
//   MAD      k_pc_mad<own>: any other power-of-two D >= 16 whose ring of sums fits in LDS (48 kHz: 128, 192 kHz: 512)
//   MA_POW2  k_pc_ma<., true> twice: any other power of two, one wave per average
//   MA_DIV   k_pc_ma<., false> twice: any D
enum PcMa { MA2_CMW, MA2, MAD, MA_POW2, MA_DIV };
// the AGC: chunk maxima + k_pc_agc, or sub-block maxima / prefix maxima / w_t / gain / int16 output
enum PcAgc { AGC_ONE_KERNEL, AGC_FIVE };

struct PcPlan {
    PcVerdict verdict = PC_OK;
    // ---- what the rate and the frame size fix.  The plan is the record of these numbers; PostArgs carries a copy of them to
    // the kernels, written by pc_fill_args below and by nothing else.
    int D = 0, L = 0, h = 0;  // DC delay, AGC look-ahead, samples per frame
    float desired = 0, attack = 0, release = 0;
    int vo = 0;               // V1 / P / S: leading pad that makes sample 0's row a multiple of 4
    size_t px = 0, pv = 0;    // pitches of X / M1 and of V1 / P / S
    int nsub = 0, sb = 0;     // look-ahead peak: sub-blocks per block of L rows, rows of one
    int nch = 0;              // chunks of 16 floats per slot in CM / CP / CS
    unsigned h_magic = 0;     // ceil(2^32 / h)
    size_t Tm = 0;            // longest stream of a batch (max_batch frames)
    bool agc_ok = false;      // the rate / frame size allow k_pc_agc
    // ---- the recurrence kernels' work-groups
    unsigned groups = 0;      // groups of 64 slots
    int lanes = 0;            // slots per work-group of a recurrence kernel
    unsigned rgroups = 0;     // work-groups of each recurrence kernel
    int reserve = 0;          // CUs the FFT passes leave free while the chain is on (a multiple of 8: one per XCD); 0: none
    bool own = false;         // the recurrence waves allocate a whole SIMD's registers
    bool rows4 = false;       // every frame starts on a row group: the lane = slot gather / output (k_pc_gather4, k_pc_out4)
    // ---- the form
    PcMa ma = MA_DIV;
    PcAgc agc = AGC_FIVE;
    bool ma_fused = false;    // k_pc_ma2 keeps M1's history itself (PostArgs::ma_fused)
    bool direct = false;      // k_pc_ma2 may read the demodulator's rows themselves (PostArgs::direct)
    bool att_faster = false;  // attack >= release: the gain step's pick is a min (postchain.h pc_gain_step)
    bool pcm16 = false;
    size_t ma_lds = 0, gain_lds = 0;  // dynamic LDS of the moving averages' / of k_pc_gain's launch
    // ---- the streams: indices into psdr_ctx::pc_s, -1 = the side stream (stage 0 always rides there)
    int s_ma = -1, s_gain = -1, s_peak = -1;  // moving averages + history (+ chunk maxima); gain + output / k_pc_agc; peak kernels
    bool split_peak = false;   // five-kernel form: the prefix maxima ride behind the moving averages, w_t in front of the gain
    bool pick_streams = false; // the one-time set-up chooses pc_s by measurement (pc_pick_streams)
    int skip = 0;              // PcKnobs::skip
};

// The AGC's attack / release coefficient of a time constant in ms at the rate sr, 1 - exp(-1 / (ms * 0.001 * sr)) as
// src/utils/audioprocessing.cpp:13-14 computes it: the products and the quotient in f32, exp() on a float argument is C's
// double exp, and the double result narrows into the float member.  The context's own AGC (pc_resolve below) and every
// per-client profile (agcplan.h) get their coefficients here.
inline float pc_agc_coeff(float ms, float sr) { return (float)(1 - std::exp((double)(-1.0f / (ms * 0.001f * sr)))); }

// look-ahead blocks of L rows that L - 1 history rows and T samples touch
inline size_t pc_nblk(int L, size_t T) { return ((size_t)L - 1 + T + (size_t)L - 1) / (size_t)L; }

inline PcPlan pc_resolve(const PcFacts &f, const PcKnobs &k) {
    PcPlan p;
    const int rate = f.audio_rate;
    if (rate < 750) {
        p.verdict = PC_RATE_TOO_SMALL;
        return p;
    }
    const size_t h = (size_t)std::max(f.n, 0) / 2, Tm = (size_t)f.max_batch * h;
    if (h == 0) {
        p.verdict = PC_NO_FRAME;
        return p;
    }
    p.h = (int)h;
    p.Tm = Tm;
    p.D = rate / 750 * 2;  // DCBlocker(audio_max_sps / 750 * 2), src/signal.cpp:54
    // AGC(0.2f, 50.0f, 300.0f, 200.0f, audio_max_sps), src/signal.cpp:55 and
    // src/utils/audioprocessing.cpp:5-16 (exp() on a float argument is C's double exp)
    const float sr = (float)rate;
    p.L = (int)(size_t)(200.0f * sr / 1000.0f);
    p.desired = 0.2f;
    p.attack = pc_agc_coeff(50.0f, sr);
    p.release = pc_agc_coeff(300.0f, sr);
    p.att_faster = p.attack >= p.release;
    // (D up to 12288 - audio rates up to 4.6 MHz; the AGC look-ahead L has no such limit: k_pc_submax / k_pc_prefix /
    // k_pc_want walk it in 256-row pieces)
    if (p.D < 1 || p.L < 2 || p.D > 12288) {
        p.verdict = PC_RATE_UNSUPPORTED;
        return p;
    }
    // lane-interleaved streams (postchain.h): pitches are multiples of 4 floats per slot, + padding for the blocked kernels'
    // look-ahead
    p.px = ((size_t)p.D + Tm + PSDR_PC_PAD + 3) & ~(size_t)3;
    p.vo = (4 - ((p.L - 1) & 3)) & 3;
    p.pv = ((size_t)p.vo + (size_t)p.L - 1 + Tm + PSDR_PC_PAD + 3) & ~(size_t)3;
    // look-ahead peak: sub-blocks of at most 256 rows of a block of L rows (postchain.h: a wave per sub-block and 64 slots,
    // 16 rows per round trip to memory - beside the FFT passes a round trip is microseconds)
    p.nsub = (p.L + 255) / 256;
    p.sb = (p.L + p.nsub - 1) / p.nsub;
    // the AGC in one kernel (postchain.h k_pc_agc): whole chunks of 16 floats must line up with sample 0's row and with the
    // row groups of a frame; stream position / h by one 32-bit multiplication
    p.agc_ok = (p.L % 16) == 0 && p.L >= 32 && p.vo == 1 && (h % 4) == 0 && h >= 16 && (p.D % 4) == 0 && (Tm + 4096) * h < ((size_t)1 << 32);
    p.nch = (int)((size_t)p.L / 16 + (Tm + 15) / 16 + 8);
    p.h_magic = (unsigned)((((uint64_t)1 << 32) + h - 1) / h);
    p.rows4 = (p.h & 3) == 0 && (p.D & 3) == 0;

    // The recurrence kernels (k_pc_ma2 / k_pc_mad, k_pc_gain, k_pc_agc): 32 slots per work-group (half a wave in use, 512-byte
    // memory operations: 256 clients 3.80-3.90 -> 3.55-3.67 ms per step, level at 16 - profiles/r05_post_chain_lanes.jsonl),
    // whole waves beyond 512 slots.  Their waves own a SIMD each (512 registers allocated) as long as the CUs the passes
    // leave free hold them all: 2 kernels x 2 waves per work-group = one CU per work-group of either; one, two or three
    // CUs per XCD stay free (8: +0.5 % on the plain step, 16: +1 %, 24: +2.5 %).
    p.groups = (unsigned)(((size_t)f.slots + 63) / 64);
    p.lanes = p.groups <= 8 ? 32 : 64;
    if (k.lanes != PC_UNSET) p.lanes = k.lanes == 16 ? 16 : k.lanes == 32 ? 32 : 64;
    p.rgroups = p.groups * (unsigned)(64 / p.lanes);
    p.reserve = (int)std::min(24u, 8u * (1u + p.rgroups / 8u));
    if (k.reserve != PC_UNSET) p.reserve = k.reserve & ~7;
    p.own = (int)p.rgroups <= p.reserve;
    if (k.own != PC_UNSET) p.own = k.own != 0;

    // The AGC as chunk maxima + ONE four-wave kernel (k_pc_agc: V1 read twice, the PCM written once - the five kernels of the
    // other form pass over a stream eleven times) whenever the rate allows it and its work-groups - a whole CU each: four
    // waves that own their SIMD - have the CUs the passes leave free
    bool agc_fused = p.agc_ok && p.own && f.opt_pc_agc != 0 && p.lanes <= 32;
    if (k.fused != PC_UNSET) agc_fused = agc_fused && k.fused != 0;
    p.agc = agc_fused ? AGC_ONE_KERNEL : AGC_FIVE;
    p.pcm16 = f.opt_pc_pcm16 != 0;
    // D = 32: both averages in one loop ...
    p.ma_fused = p.D == 32;
    // ... which may read the demodulator's rows themselves instead of a gathered copy (k_pc_ma2 DIRECT; part of the one-kernel
    // form of the chain, PSDR_OPT_POST_CHAIN_AGC = 1; the demodulation two batches on waits for this batch's stage 1: demod.hip)
    p.direct = p.ma_fused && p.rows4 && f.opt_pc_agc != 0;
    if (k.direct != PC_UNSET) p.direct = p.direct && k.direct != 0;
    // ... and leave the chunk maxima of the new samples from a third wave (k_pc_ma2 CMW) instead of a pass over V1, while the
    // free CUs hold a three-wave work-group of those beside every four-wave one of the AGC (a CU each)
    bool cmw = agc_fused && p.ma_fused && 2 * (int)p.rgroups <= p.reserve;
    if (k.cmw != PC_UNSET) cmw = cmw && k.cmw != 0;
    const bool pow2 = (p.D & (p.D - 1)) == 0;
    const size_t ring_lds = (size_t)p.D * p.lanes * sizeof(float);  // k_pc_mad: wave 1's ring of the last D sums
    if (p.ma_fused)
        p.ma = cmw ? MA2_CMW : MA2;
    else if (pow2 && p.D >= 16 && ring_lds <= 128 * 1024)
        p.ma = MAD;
    else
        p.ma = pow2 ? MA_POW2 : MA_DIV;
    // Dynamic LDS.  Recurrence waves that do NOT own their SIMD are kept off the passes' CUs by LDS instead: a pass's
    // work-group takes 128 KiB of a CU's 160, so a work-group that asks for 34 KiB in all only fits on a CU the passes leave
    // free (ctx.h persistent_grid).  What is asked for at launch is 34 KiB less the kernel's own static LDS: 17 KiB in k_pc_ma2
    // (hand, fin, ohand), 8 KiB in k_pc_gain (hand).  Not when no CU is left free, nor beyond 16 work-groups (they would wait
    // for one another instead), nor for waves that own a SIMD (they fit nowhere else anyway).
    const size_t home_lds = (p.reserve > 0 && p.rgroups <= 16 && !p.own) ? 34 * 1024 : 0;
    p.ma_lds = p.ma == MAD ? ring_lds : (p.ma == MA2 && home_lds) ? home_lds - 17 * 1024 : 0;
    p.gain_lds = home_lds ? home_lds - 8 * 1024 : 0;

    // Streams: stage 0 rides behind the demodulation on the side stream (two short kernels), stage 2 in front of stage 3 on
    // ITS stream (they are a chain anyway), the moving averages on the other.  Hardware queues are what is scarce: with four
    // chain streams the fourth shared a queue with the third (the gain recurrence in front of the next batch's peak), and
    // with three - five busy queues with the main and the side stream - every second launch of the PASSES started 50 - 60 us
    // late (6 - 9 us with four queues, as without the chain): 4 % of the step.
    // WHICH queues matters as much (tools/runs/r05_w.sh, r05_y.sh; rocprofv3 Queue_Id): the chain on queues 4 and 6 leaves the
    // passes' launches alone, on 4 and 5 it delays them as three chain queues do - queue 5 shares its pipe of the command
    // processor with queue 1, the main stream's.  pc_s[0] and pc_s[2] are the ones chosen by that measure (postchain.hip).
    if (f.piped) {
        p.s_ma = 0, p.s_gain = 2, p.s_peak = 2;
        if (k.streams == 3) p.s_peak = 1;
        if (k.streams == 2) p.s_peak = p.s_gain = 1;
        if (k.streams == 1) p.s_peak = p.s_ma;
    }
    // the prefix maxima ride behind the moving averages, w_t in front of the gain recurrence (with 256 clients the gain's
    // stream is the longer one: 0.8 ms of peak kernels + 1.9 + 0.3 against 2.3)
    p.split_peak = f.piped && p.s_peak == p.s_gain;
    if (k.split_peak != PC_UNSET) p.split_peak = p.split_peak && k.split_peak != 0;
    p.pick_streams = f.opt_pc_streams != 0;
    if (k.pick != PC_UNSET) p.pick_streams = k.pick != 0;
    p.skip = k.skip != PC_UNSET ? k.skip : 0;
    return p;
}

// the kernels' copy of the plan's numbers (the buffers, the batch and the slot count are the caller's)
inline void pc_fill_args(PostArgs &a, const PcPlan &p) {
    a.h = p.h, a.D = p.D, a.L = p.L;
    a.desired = p.desired, a.attack = p.attack, a.release = p.release;
    a.px = p.px, a.pv = p.pv, a.vo = p.vo;
    a.nsub = p.nsub, a.sb = p.sb, a.nch = p.nch, a.h_magic = p.h_magic;
    a.lanes = p.lanes, a.ma_fused = p.ma_fused, a.direct = p.direct, a.pcm16 = p.pcm16;
}

}  // namespace psdr

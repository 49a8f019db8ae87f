// blankerplan.h - the wideband impulse blanker on the ingest ring (include/psdr.h: psdr_ring_set_blanker), everything of it that
// is not a launch: the argument check, the plan of one psdr_process_ring call (which halves are new, their slots, which one
// has the mirror, which one uses its own reference level, the new `next`) and the ONE definition of the per-sample power,
// the maximum and the exceed test (the kernels of blanker.h and the host tests run this text).  Plain C++17 (no HIP):
// tests/test_blanker_host.py builds it with the host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

// the power and the comparisons are host code and device code alike
#ifndef PSDR_HOST_DEVICE
#if defined(__HIPCC__)
#define PSDR_HOST_DEVICE __host__ __device__
#else
#define PSDR_HOST_DEVICE
#endif
#endif

// (the chunk's loops are unrolled so that the powers stay in registers on the device)
#if defined(__clang__)
#define NB_UNROLL _Pragma("unroll")
#else
#define NB_UNROLL
#endif

namespace psdr {

constexpr int NB_BLOCK = 256;          // samples per block of the reference level
constexpr int NB_CHUNK = 16;           // bytes a lane of the streaming kernel loads at once
constexpr int NB_TILE = 4096;          // bytes a work-group of the streaming kernel takes per step: 256 chunks
constexpr double NB_DB_MAX = 90.0;     // threshold_db in [0, 90]
constexpr int NB_GUARD_MAX = 255;      // guard in 0..255: a block's zeros depend on its two neighbours at most
enum { NB_U8 = 0, NB_S8 = 1, NB_U16 = 2, NB_S16 = 3, NB_F32 = 4, NB_F64 = 5 };  // psdr_format (include/psdr.h)

// psdr_ring_set_blanker's refusals, in the order they are looked for; on = 0 ignores both values
enum NbVerdict { NB_OK, NB_BAD_DB, NB_BAD_GUARD };
inline NbVerdict nb_check(int on, double threshold_db, int guard) {
    if (!on) return NB_OK;
    if (!std::isfinite(threshold_db) || threshold_db < 0.0 || threshold_db > NB_DB_MAX) return NB_BAD_DB;
    if (guard < 0 || guard > NB_GUARD_MAX) return NB_BAD_GUARD;
    return NB_OK;
}
// kf = (float)pow(10, db / 10): computed in double, rounded once
inline float nb_factor(double threshold_db) { return (float)std::pow(10.0, threshold_db / 10.0); }

PSDR_HOST_DEVICE inline int nb_comp_bytes(int fmt) { return fmt <= NB_S8 ? 1 : (fmt <= NB_S16 ? 2 : (fmt == NB_F32 ? 4 : 8)); }
PSDR_HOST_DEVICE inline int nb_sample_bytes(int fmt, bool real) { return nb_comp_bytes(fmt) * (real ? 1 : 2); }
// the code the converter maps to 0.0, repeated over a 32-bit word: 0x80 for u8, 0x8000 for u16, 0 for everything else
PSDR_HOST_DEVICE inline uint32_t nb_zero_word(int fmt) { return fmt == NB_U8 ? 0x80808080u : (fmt == NB_U16 ? 0x80008000u : 0u); }

// ---- the rule's arithmetic --------------------------------------------------------------------------------------------
// integer formats: a, b are the converter's unscaled integers (behind the MSB flip of u8 / u16); a*a + b*b exactly in unsigned
// 32-bit arithmetic (at most 2^31: s16 at -32768 twice), converted once, round to nearest even
PSDR_HOST_DEVICE inline float nb_power_int(int a, int b) { return (float)((uint32_t)(a * a) + (uint32_t)(b * b)); }
// floats: fl(fl(re*re) + fl(im*im)), no fused contraction
PSDR_HOST_DEVICE inline float nb_power_f32(float re, float im) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float a = re * re;
    const float b = im * im;
    return a + b;
}
PSDR_HOST_DEVICE inline float nb_narrow(double v) { return (float)v; }  // f64 is narrowed first, as pass 1 does
// every maximum: starts from +0.0; a NaN P is never a maximum
PSDR_HOST_DEVICE inline float nb_max(float m, float P) { return (P > m) ? P : m; }
// ... and never exceeds a threshold
PSDR_HOST_DEVICE inline bool nb_exceed(float P, float T) { return P > T; }
// a threshold of 0 (digital silence) or a non-finite one (an Inf half) blanks nothing
PSDR_HOST_DEVICE inline bool nb_threshold_valid(float T) { return T > 0.f && T <= 3.402823466e+38f; }

PSDR_HOST_DEVICE inline int nb_s8(uint32_t w, int k) { return (int)(int8_t)((w >> (8 * k)) & 0xFFu); }
PSDR_HOST_DEVICE inline int nb_s16(uint32_t w, int k) { return (int)(int16_t)((w >> (16 * k)) & 0xFFFFu); }
PSDR_HOST_DEVICE inline float nb_f32(uint32_t w) {
    float f;
    __builtin_memcpy(&f, &w, 4);
    return f;
}
PSDR_HOST_DEVICE inline float nb_f64(uint32_t lo, uint32_t hi) {
    const uint64_t u = (uint64_t)lo | ((uint64_t)hi << 32);
    double d;
    __builtin_memcpy(&d, &u, 8);
    return nb_narrow(d);
}

// The powers of the samples in one 16-byte chunk (w: its four little-endian words), in sample order; returns how many
// there are (16 / nb_sample_bytes).  The branch on the format is uniform over a launch.
PSDR_HOST_DEVICE inline int nb_chunk_powers(const uint32_t w[4], int fmt, bool real, float P[16]) {
    const uint32_t flip = nb_zero_word(fmt);
    switch (fmt) {
    case NB_U8:
    case NB_S8:
        NB_UNROLL
        for (int k = 0; k < 4; k++) {
            const uint32_t v = w[k] ^ flip;
            if (real) {
                NB_UNROLL
                for (int b = 0; b < 4; b++) P[4 * k + b] = nb_power_int(nb_s8(v, b), 0);
            } else {
                P[2 * k] = nb_power_int(nb_s8(v, 0), nb_s8(v, 1));
                P[2 * k + 1] = nb_power_int(nb_s8(v, 2), nb_s8(v, 3));
            }
        }
        return real ? 16 : 8;
    case NB_U16:
    case NB_S16:
        NB_UNROLL
        for (int k = 0; k < 4; k++) {
            const uint32_t v = w[k] ^ flip;
            if (real) {
                P[2 * k] = nb_power_int(nb_s16(v, 0), 0);
                P[2 * k + 1] = nb_power_int(nb_s16(v, 1), 0);
            } else {
                P[k] = nb_power_int(nb_s16(v, 0), nb_s16(v, 1));
            }
        }
        return real ? 8 : 4;
    case NB_F32:
        if (real) {
            NB_UNROLL
            for (int k = 0; k < 4; k++) P[k] = nb_power_f32(nb_f32(w[k]), 0.f);
            return 4;
        }
        P[0] = nb_power_f32(nb_f32(w[0]), nb_f32(w[1]));
        P[1] = nb_power_f32(nb_f32(w[2]), nb_f32(w[3]));
        return 2;
    default:
        if (real) {
            P[0] = nb_power_f32(nb_f64(w[0], w[1]), 0.f);
            P[1] = nb_power_f32(nb_f64(w[2], w[3]), 0.f);
            return 2;
        }
        P[0] = nb_power_f32(nb_f64(w[0], w[1]), nb_f64(w[2], w[3]));
        return 1;
    }
}
// ... their maximum (the streaming kernel's step), formed without the array: the same functions in the same order
PSDR_HOST_DEVICE inline float nb_max4(float m, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int fmt, bool real) {
    const uint32_t flip = nb_zero_word(fmt);
    const uint32_t w[4] = {w0 ^ flip, w1 ^ flip, w2 ^ flip, w3 ^ flip};
    if (fmt <= NB_S8) {
        NB_UNROLL
        for (int k = 0; k < 4; k++) {
            if (real) {
                NB_UNROLL
                for (int b = 0; b < 4; b++) m = nb_max(m, nb_power_int(nb_s8(w[k], b), 0));
            } else {
                m = nb_max(m, nb_power_int(nb_s8(w[k], 0), nb_s8(w[k], 1)));
                m = nb_max(m, nb_power_int(nb_s8(w[k], 2), nb_s8(w[k], 3)));
            }
        }
    } else if (fmt <= NB_S16) {
        NB_UNROLL
        for (int k = 0; k < 4; k++) {
            if (real) {
                m = nb_max(m, nb_power_int(nb_s16(w[k], 0), 0));
                m = nb_max(m, nb_power_int(nb_s16(w[k], 1), 0));
            } else {
                m = nb_max(m, nb_power_int(nb_s16(w[k], 0), nb_s16(w[k], 1)));
            }
        }
    } else if (fmt == NB_F32) {
        if (real) {
            NB_UNROLL
            for (int k = 0; k < 4; k++) m = nb_max(m, nb_power_f32(nb_f32(w[k]), 0.f));
        } else {
            m = nb_max(m, nb_power_f32(nb_f32(w[0]), nb_f32(w[1])));
            m = nb_max(m, nb_power_f32(nb_f32(w[2]), nb_f32(w[3])));
        }
    } else if (real) {
        m = nb_max(m, nb_power_f32(nb_f64(w[0], w[1]), 0.f));
        m = nb_max(m, nb_power_f32(nb_f64(w[2], w[3]), 0.f));
    } else {
        m = nb_max(m, nb_power_f32(nb_f64(w[0], w[1]), nb_f64(w[2], w[3])));
    }
    return m;
}
PSDR_HOST_DEVICE inline float nb_chunk_max(const uint32_t w[4], int fmt, bool real) { return nb_max4(0.f, w[0], w[1], w[2], w[3], fmt, real); }
// One sample's power from its bytes (the marking kernel's step: a sample is 1, 2, 4, 8 or 16 bytes and aligned to its size)
PSDR_HOST_DEVICE inline float nb_sample_power(const unsigned char *s, int fmt, bool real) {
    uint32_t w[4] = {0, 0, 0, 0};
    const int sb = nb_sample_bytes(fmt, real);
    // an integer sample shorter than a word sits in a word of zero CODES, whose power is 0
    w[0] = nb_comp_bytes(fmt) <= 2 ? nb_zero_word(fmt) : 0u;
    if (sb == 1) {
        w[0] = (w[0] & ~0xFFu) | s[0];
    } else if (sb == 2) {
        uint16_t h;
        __builtin_memcpy(&h, s, 2);
        w[0] = (w[0] & ~0xFFFFu) | h;
    } else if (sb == 4) {
        __builtin_memcpy(w, s, 4);
    } else if (sb == 8) {
        __builtin_memcpy(w, s, 8);
    } else {
        __builtin_memcpy(w, s, 16);
    }
    // the sample is the chunk's first: lay it out as a chunk of its kind whose other samples are zero
    if (fmt == NB_F32 && real) return nb_power_f32(nb_f32(w[0]), 0.f);
    if (fmt == NB_F64 && real) return nb_power_f32(nb_f64(w[0], w[1]), 0.f);
    if (fmt == NB_F32) return nb_power_f32(nb_f32(w[0]), nb_f32(w[1]));
    if (fmt == NB_F64) return nb_power_f32(nb_f64(w[0], w[1]), nb_f64(w[2], w[3]));
    const uint32_t v = w[0] ^ nb_zero_word(fmt);
    if (nb_comp_bytes(fmt) == 1) return nb_power_int(nb_s8(v, 0), real ? 0 : nb_s8(v, 1));
    return nb_power_int(nb_s16(v, 0), real ? 0 : nb_s16(v, 1));
}

// ---- the plan of one psdr_process_ring call ---------------------------------------------------------------------------
// What the host carries between calls.  The reference levels live in a device ring of rcap = max_batch + 2 floats: a call
// writes the levels of its new halves behind the level of half next - 1, so the carried level needs no copy.
struct NbState {
    uint64_t next = 0;   // index of the next half to blank; halves below it are skipped
    bool fresh = true;   // switched on since the last call: the reference starts afresh
    int rpos = 0;        // position of R of half next - 1 in the device ring of levels
};
struct NbPlan {
    int nnew = 0;             // new halves: first_new .. first_new + nnew - 1 (0: nothing is launched)
    uint64_t first_new = 0;
    int slot0 = 0;            // slot of the first new half; half j sits in slot (slot0 + j) % nhalves
    int mirror = -1;          // the new half that lands in slot 0 and is written twice (ring slot 0 and the mirror), or -1
    bool own = false;         // the first new half takes its threshold from its own R (switched on, or a jump ahead)
    int r0 = 0;               // ring position of R of the first new half; half j: (r0 + j) % rcap
    NbState after;            // the state behind the call
};
// halves first_half .. first_half + nframes are read (nframes <= max_batch, checked by the caller)
inline NbPlan nb_plan(const NbState &s, uint64_t first_half, int nframes, int nhalves, int rcap) {
    NbPlan p;
    const uint64_t end = first_half + (uint64_t)nframes + 1;  // one past the last half read
    p.own = s.fresh || first_half > s.next;
    p.first_new = p.own ? first_half : s.next;
    p.nnew = end > p.first_new ? (int)(end - p.first_new) : 0;
    p.slot0 = (int)(p.first_new % (uint64_t)nhalves);
    for (int j = 0; j < p.nnew; j++)
        if ((p.slot0 + j) % nhalves == 0) p.mirror = j;  // (at most one: a call never crosses the end of the ring)
    p.r0 = (s.rpos + 1) % rcap;
    p.after.fresh = false;
    p.after.next = p.nnew ? end : (p.own ? first_half : s.next);
    p.after.rpos = (s.rpos + p.nnew) % rcap;
    return p;
}
// ring position of the level half j's threshold is made of: the half before it, or its own
inline int nb_prev_pos(const NbPlan &p, int j, int rcap) { return (j == 0 && p.own) ? p.r0 : (p.r0 + j - 1 + rcap) % rcap; }

}  // namespace psdr

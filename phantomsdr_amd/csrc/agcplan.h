// agcplan.h - the per-client AGC profile (include/psdr.h: psdr_client_set_agc_profile), everything of it that is not a launch:
// the ONE definition of the wanted gain w_t (every kernel of postchain.h that forms w and the host tests run this text), the
// table entry, the presets, the argument validation and agc_profile_plan(), which walks the audio slots behind demod_plan() and
// writes the batch's table.  The coefficient function is postplan.h's pc_agc_coeff, the context's own.  Plain C++17 (no HIP):
// tests/test_agc_profile_host.py builds it with the host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <limits>

#include "demodplan.h"
#include "postplan.h"

// the rule is host code and device code alike
#ifndef PSDR_HOST_DEVICE
#if defined(__HIPCC__)
#define PSDR_HOST_DEVICE __host__ __device__
#else
#define PSDR_HOST_DEVICE
#endif
#endif

namespace psdr {

// ---- the rule -----------------------------------------------------------------------------------------------------------------
// desired / (peak + 1e-10), the reference's wanted gain (src/utils/audioprocessing.cpp:57): one addition and one division, each
// rounded once (nothing here can contract: there is no product)
PSDR_HOST_DEVICE inline float agc_ratio(float desired, float peak) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(desired, __fadd_rn(peak, 1e-10f));
#else
    return desired / (peak + 1e-10f);
#endif
}
// w_t of a slot with a profile: the manual gain whatever the signal, else the reference's wanted gain under the cap (+Inf: none -
// fminf against +Inf is the identity)
PSDR_HOST_DEVICE inline float agc_want(const AgcEntry &e, float peak) { return e.manual ? e.manual_gain : fminf(agc_ratio(e.desired, peak), e.cap); }

// ---- the table entry ----------------------------------------------------------------------------------------------------------
// a slot without a profile
inline AgcEntry agc_entry_none() { return AgcEntry{0.f, 0.f, 0.f, std::numeric_limits<float>::infinity(), 0.f, 0, 0, 0}; }
// an accepted profile at the context's audio rate: every number rounded once to f32
inline AgcEntry agc_entry(const psdr_agc_profile &p, int audio_rate) {
    AgcEntry e = agc_entry_none();
    const float sr = (float)audio_rate;
    e.desired = (float)p.desired;
    e.att = pc_agc_coeff((float)p.attack_ms, sr);
    e.rel = pc_agc_coeff((float)p.release_ms, sr);
    if (p.max_gain > 0) e.cap = (float)p.max_gain;
    e.manual = p.manual ? 1 : 0;
    e.manual_gain = p.manual ? (float)p.manual_gain : 0.f;
    e.on = 1;
    return e;
}

// ---- presets ------------------------------------------------------------------------------------------------------------------
inline bool agc_preset(int kind, psdr_agc_profile *out) {
    if (!out || kind < PSDR_AGC_REFERENCE || kind > PSDR_AGC_SLOW) return false;
    psdr_agc_profile p{};
    p.desired = 0.2;
    p.attack_ms = kind == PSDR_AGC_FAST ? 5.0 : 50.0;
    p.release_ms = kind == PSDR_AGC_FAST ? 100.0 : kind == PSDR_AGC_SLOW ? 2000.0 : 300.0;
    *out = p;
    return true;
}

// ---- validation ---------------------------------------------------------------------------------------------------------------
// psdr_client_set_agc_profile's refusals, in the order they are looked for.  AP_NO_RATE is PSDR_ERR_STATE, every other
// PSDR_ERR_INVALID; a null profile (back to the context's AGC) asks for a known id only.
enum AgcVerdict { AP_OK, AP_BAD_ID, AP_NONFINITE, AP_BAD_DESIRED, AP_BAD_TIME, AP_BAD_CAP, AP_BAD_MANUAL, AP_BAD_MANUAL_GAIN, AP_NO_RATE, AP_ATTACK_SLOWER };
constexpr double AGC_MS_MAX = 10000.0;
inline AgcVerdict agc_profile_check_values(const psdr_agc_profile &p, int audio_rate) {
    // (manual_gain is read only when manual = 1; it must be an f32 number too: a finite double beyond FLT_MAX would round to infinity)
    if (!std::isfinite(p.desired) || !std::isfinite(p.attack_ms) || !std::isfinite(p.release_ms) || !std::isfinite(p.max_gain)) return AP_NONFINITE;
    if (p.manual == 1 && (!std::isfinite(p.manual_gain) || !std::isfinite((float)p.manual_gain))) return AP_NONFINITE;
    if (!(p.desired > 0 && p.desired <= 1)) return AP_BAD_DESIRED;
    if (!(p.attack_ms > 0 && p.attack_ms <= AGC_MS_MAX) || !(p.release_ms > 0 && p.release_ms <= AGC_MS_MAX)) return AP_BAD_TIME;
    if (p.max_gain < 0) return AP_BAD_CAP;
    if (p.manual < 0 || p.manual > 1) return AP_BAD_MANUAL;
    if (p.manual == 1 && p.manual_gain < 0) return AP_BAD_MANUAL_GAIN;
    if (audio_rate <= 0) return AP_NO_RATE;
    // the gain step picks between its two candidates by min / max (postchain.h pc_gain_step, ATT_FASTER): every lane of a wave
    // must have attack at least as fast as release, as the context's own AGC has
    const AgcEntry e = agc_entry(p, audio_rate);
    if (e.att < e.rel) return AP_ATTACK_SLOWER;
    return AP_OK;
}
inline AgcVerdict agc_profile_check(const AudioSlot *slots, size_t S, int id, const psdr_agc_profile *p, int audio_rate) {
    if (id < 0 || (size_t)id >= S || !slots[id].active) return AP_BAD_ID;
    return p ? agc_profile_check_values(*p, audio_rate) : AP_OK;
}
// ... and what an accepted call does to the slot: the setting alone.  No state moves - the gain, the look-ahead fill count and
// the DC sums carry on (AGC::reset stays with psdr_client_set_audio_demodulation)
inline void agc_profile_apply(AudioSlot &s, const psdr_agc_profile *p, int audio_rate) { s.agc = p ? agc_entry(*p, audio_rate) : agc_entry_none(); }

// ---- the batch ----------------------------------------------------------------------------------------------------------------
struct AgcPlan {
    bool any = false;  // a client with a profile has a stream in the batch's chain; else nothing is uploaded and the kernels
                       // without the table are launched
};
// One batch, behind demod_plan(): writes the table (S entries, by slot).  The clients the batch demodulated are those whose
// last_seq is the batch's demod_seq; an IQ client and a paused one keep their setting and have no stream.
inline AgcPlan agc_profile_plan(const AudioSlot *slots, size_t S, uint64_t demod_seq, AgcEntry *table) {
    AgcPlan p;
    for (size_t i = 0; i < S; i++) {
        const AudioSlot &s = slots[i];
        table[i] = s.active ? s.agc : agc_entry_none();
        if (s.active && s.agc.on && !s.paused && s.last_seq == demod_seq && s.b_mode != PSDR_IQ) p.any = true;
    }
    return p;
}

}  // namespace psdr

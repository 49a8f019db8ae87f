// demodplan.h - WHO is demodulated in a batch, in which list and from which state, resolved in one pure function: from the
// audio slots and a few facts to the parameter-ring slot's host image and a plan of what demod.hip copies, zeroes and
// launches.  Plain host C++17 (no HIP): demod.hip enqueues from the plan, tests/test_demod_plan.py prints it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/psdr.h"
#include "types.h"

namespace psdr {

// One section of a client's audio filter as the device table holds it (audiofilterplan.h): the f32 coefficients of
// include/psdr.h's psdr_biquad and, for the blocked evaluation's scan, the powers P[k] = M^(2^k), k = 0..5, of M = A^16 with A =
// [[-a1, 1], [-a2, 0]] the section's state matrix - row-major m00 m01 m10 m11, computed in double and rounded once
struct AfSection {
    float b0 = 0, b1 = 0, b2 = 0, a1 = 0, a2 = 0, pad[3] = {0, 0, 0};
    float P[6][4] = {};
};
static_assert(sizeof(AfSection) == 128, "the device table's layout");

// One entry of the fax decoder's batch table (faxplan.h), which an audio slot keeps whole
struct FaxEntry {
    int slot, mode, width, K, D, NB, start_blocks, phase_lines, max_lines, wp, R, pad;
    uint64_t Lq, origin0;    // the line in 1/65536 sample; phase_col Lq / width
    uint32_t inc, tinc[3];   // the centre's increment, the three tones'
    float rot[2], trot[3][2];
    float s, ratio, shift, nbh;  // v = 0.5 + a s; tone_ratio; white - black; NB H
};

struct AudioSlot {
    bool active = false;
    int l = 0, r = 0;
    double mid = 0;
    int mode = PSDR_USB;
    int state_cur = 0;
    int agc_reset = 2;  // post chain: 1 = AGC::reset pending (set_audio_demodulation), 2 = fresh client
    bool paused = false;  // psdr_client_set_paused: sits out the demodulation batches, all state frozen
    uint64_t last_seq = 0;  // the demodulation batch (ctx->demod_seq) that last included this slot; 0: none yet
    int b_l = 0, b_r = 0;   // the window that batch was demodulated with (psdr_fetch_begin copies it into its FetchSet)
    double b_mid = 0;
    int b_mode = PSDR_USB;  // ... and the mode: a batch demodulated as PSDR_IQ left complex rows (iq.pool) and no audio / PCM; one
                            // demodulated as PSDR_SAM left carrier records and a carrier tail the next SAM batch continues
    uint64_t born = 0;      // psdr_client_add's serial number: a fetched set answers only for the occupant it was filled with
    // psdr_client_set_fine_tune: with the flag on, a USB / LSB / IQ client is a TUNED client (demod.h: k_demod_chain_ft)
    int fine = 0;
    uint32_t ft_phi = 0;    // the rotator's phase at the next tuned batch's first sample (units of 2^-32 turn)
    bool b_tuned = false;   // the last batch took the tuned path (with b_mode: whether the tuned USB / LSB tail continues)
    // psdr_client_set_sam_sideband: a PSDR_SAM client with another value than PSDR_SAM_BOTH is a SIDEBAND SAM client
    // (demod.h: k_demod_chain_sbsam); in every other mode the value is kept and has no effect
    int sam_sb = PSDR_SAM_BOTH;
    int b_sam_sb = PSDR_SAM_BOTH;  // ... of the last batch (with b_mode: whether the sideband baseband tail continues)
    // psdr_client_set_notch: the two manual notches, [first, end) in the coordinates of l / r (0, 0: empty); b_notch: the
    // last batch's snapshot (psdr_read_notches)
    int notch[4] = {0, 0, 0, 0}, b_notch[4] = {0, 0, 0, 0};  // first0, end0, first1, end1
    // psdr_client_set_auto_notch; b_auto: of the last batch (with b_l / b_r / b_mid / b_mode: whether the detector's state continues)
    int auto_notch = 0;
    bool b_auto = false;
    bool auto_fresh = false;  // switched on since the slot's last batch (a paused client may be switched off and on again)
    // psdr_client_set_squelch (squelchplan.h): the level gate's thresholds (f32, in the units of pwr) and frame counts; b_sq_on: the
    // last batch ran with it (psdr_read_squelch); sq_fresh: switched on since the slot's last batch - the state starts from zero
    int sq_on = 0;
    float sq_t_open = 1.f, sq_t_close = 1.f;
    int sq_attack = 1, sq_hang = 0;
    bool b_sq_on = false, sq_fresh = false;
    // psdr_client_set_audio_filter (audiofilterplan.h): af_n sections (0: off) as the table holds them; af_fresh: set since the
    // slot's last filtered batch - the state starts from zero
    int af_n = 0;
    AfSection af_sec[PSDR_AUDIO_FILTER_SECTIONS];
    bool af_fresh = false;
    // psdr_client_set_agc_profile (agcplan.h): the profile as the chain's table holds it, on = 0: none.  A setting and nothing
    // else: no state of the chain starts over with it
    AgcEntry agc = {0.f, 0.f, 0.f, HUGE_VALF, 0.f, 0, 0, 0};
    // psdr_client_set_noise_floor (noiseplan.h): b_nf_on: the last batch ran with it (psdr_read_noise); nf_fresh: switched on
    // since the slot's last batch; nf_l, nf_r: the window the estimator's state belongs to - it starts from zero when any of the
    // three says so.  sq_ref: psdr_client_set_squelch_reference, what the squelch's thresholds are relative to
    int nf_on = 0;
    bool b_nf_on = false, nf_fresh = false;
    int nf_l = 0, nf_r = 0;
    int sq_ref = PSDR_SQ_ABSOLUTE;
    // psdr_client_set_noise_reduction (nrplan.h): the rounded parameters as the table holds them; nr_fresh: switched on since the
    // slot's last listed batch; nr_mode, nr_l, nr_r, nr_m: mode, window and floor(audio_mid) the state belongs to - it starts from
    // zero when any of these says so
    int nr_on = 0;
    float nr_g_min = 1.f, nr_beta = 1.f;
    bool nr_fresh = false;
    int nr_mode = PSDR_USB, nr_l = 0, nr_r = 0, nr_m = 0;
    // psdr_client_set_audio_blanker (anbplan.h): the parameters as the table holds them; anb_fresh, anb_mode, anb_l, anb_r, anb_m:
    // as the noise reduction's
    int anb_on = 0;
    float anb_threshold = 4.5f;
    int anb_width = 7;
    bool anb_fresh = false;
    int anb_mode = PSDR_USB, anb_l = 0, anb_r = 0, anb_m = 0;
    // psdr_client_set_tone_decoder (toneplan.h): the parameters as the table holds them; b_tone_on: the last batch ran with it
    // (psdr_read_tone); tone_fresh, tone_mode, tone_l, tone_r, tone_m: as the noise reduction's
    int tone_on = 0;
    int tone_want = -1, tone_gate = 0, tone_attack = 2, tone_hang = 0;
    float tone_ratio = 1.f, tone_min_level = 0.f;
    bool b_tone_on = false, tone_fresh = false;
    int tone_mode = PSDR_USB, tone_l = 0, tone_r = 0, tone_m = 0;
    // psdr_client_set_cw_decoder (cwplan.h): the parameters as the table holds them - the starting lane, the candidate lanes, the
    // starting dot length, track_speed, the ratio; b_cw_on: the last batch ran with it (psdr_read_cw); cw_fresh, cw_mode, cw_l,
    // cw_r, cw_m: as the tone decoder's
    int cw_on = 0;
    int cw_p0 = 18, cw_u0 = 180, cw_track = 1;
    uint64_t cw_cand = 0;
    float cw_ratio = 1.f;
    bool b_cw_on = false, cw_fresh = false;
    int cw_mode = PSDR_USB, cw_l = 0, cw_r = 0, cw_m = 0;
    // psdr_client_set_rtty_decoder (rttyplan.h): the parameters as the table holds them - the bit window in hops, the bit length
    // in 1/16 hop, usos, the candidate pairs, the ratio, the level's scale, the 32 lanes' increments and rotations; b_rtty_on: the
    // last batch ran with it (psdr_read_rtty); rtty_fresh, rtty_mode, rtty_l, rtty_r, rtty_m: as the tone decoder's
    int rtty_on = 0;
    int rtty_wn = 17, rtty_u = 264, rtty_usos = 1;
    uint32_t rtty_cand = 0;
    float rtty_ratio = 1.f, rtty_lscale = 0.f;
    uint32_t rtty_inc[32] = {};
    float rtty_rot[32][2] = {};
    bool b_rtty_on = false, rtty_fresh = false;
    int rtty_mode = PSDR_USB, rtty_l = 0, rtty_r = 0, rtty_m = 0;
    // psdr_client_set_psk_decoder (pskplan.h): the parameters as the table holds them - the symbol window in hops, the symbol
    // length in 1/16 hop, the candidate lanes, the coherence asked for, the level's scale, the lane spacing, the 16 lanes'
    // increments and rotations; b_psk_on: the last batch ran with it (psdr_read_psk); psk_fresh, psk_mode, psk_l, psk_r, psk_m: as
    // the tone decoder's
    int psk_on = 0;
    int psk_wn = 24, psk_u = 384;
    uint32_t psk_cand = 0;
    float psk_quality = 1.f, psk_lscale = 0.f, psk_df = 0.f;
    uint32_t psk_inc[16] = {};
    float psk_rot[16][2] = {};
    bool b_psk_on = false, psk_fresh = false;
    int psk_mode = PSDR_USB, psk_l = 0, psk_r = 0, psk_m = 0;
    // psdr_client_set_fax_decoder (faxplan.h): the parameters as the table holds them; b_fax_on: the last batch ran with it
    // (psdr_read_fax); fax_fresh, fax_mode, fax_l, fax_r, fax_m: as the tone decoder's
    int fax_on = 0;
    FaxEntry fax = {};
    bool b_fax_on = false, fax_fresh = false;
    int fax_mode = PSDR_USB, fax_l = 0, fax_r = 0, fax_m = 0;
};

// The client parameter ring's slot.  [ClientParams x S][int x S]: the batch's list and, for the post chain, the list index of
// every slot's client.  From ft_ring_off(S) on the tuned clients' list, [ClientParams x nt][FtClient x nt], and behind it
// the sideband SAM clients' list, [ClientParams x nsb][SbClient x nsb], with nt + nsb <= S (no client is on both lists).
// From notch_ring_off(S) on the manual notches of the batch's snapshot, [int4 x S] by slot (DemodArgs::notch_man), and
// k_notch_detect's list of the batch's auto-notch clients, [ClientParams x S].
static_assert(sizeof(SbClient) == sizeof(FtClient), "the two lists share the ring's space behind ft_ring_off");
constexpr size_t NOTCH_ENTRY = 16;  // sizeof(int4): first0, end0, first1, end1
inline size_t ft_ring_off(size_t S) { return (S * (sizeof(ClientParams) + sizeof(int)) + 15) & ~(size_t)15; }
inline size_t notch_ring_off(size_t S) { return (ft_ring_off(S) + S * (sizeof(ClientParams) + sizeof(FtClient)) + 15) & ~(size_t)15; }
inline size_t client_ring_bytes(size_t S) { return notch_ring_off(S) + S * (NOTCH_ENTRY + sizeof(ClientParams)); }

// a tuned client: the fine-tune flag in a mode the rotator means something in (AM, FM, SAM: the flag has no effect)
inline bool tuned_mode(int fine, int mode) { return fine && (mode == PSDR_USB || mode == PSDR_LSB || mode == PSDR_IQ); }
// a sideband SAM client: PSDR_SAM with another sideband than both (in every other mode the value has no effect)
inline bool sb_sam(int mode, int sideband) { return mode == PSDR_SAM && sideband != PSDR_SAM_BOTH; }
// PSDR_SAM (either kind) outside the compile-time plans sums the carrier's kept bins directly (demod.h: sam_carrier_dsum) and
// looks the twiddle up at (d * j) mod n with d, j < n in 32-bit unsigned arithmetic: exact while (n - 1)^2 < 2^32.
// psdr_client_set_audio_demodulation refuses the mode above that; every other mode has no such product.
constexpr int PSDR_SAM_MAX_AUDIO_FFT = 65536;
static_assert((uint64_t)(PSDR_SAM_MAX_AUDIO_FFT - 1) * (uint64_t)(PSDR_SAM_MAX_AUDIO_FFT - 1) <= 0xFFFFFFFFull, "sam_carrier_dsum's index product");
inline bool sam_size_served(int n) { return n < PSDR_SAM_MAX_AUDIO_FFT; }

// What a slot is to a batch - the one place that combines active, paused, mode, fine and sam_sb.  CK_PLAIN: USB / LSB / AM /
// FM, the list of k_demod_chain_fixed; every kind behind it has a list and launches of its own.
enum ClientKind { CK_NONE, CK_PAUSED, CK_PLAIN, CK_SAM, CK_FT_SSB, CK_FT_IQ, CK_SBSAM, CK_IQ, CK_COUNT };
inline ClientKind client_kind(const AudioSlot &s) {
    if (!s.active) return CK_NONE;
    if (s.paused) return CK_PAUSED;
    if (tuned_mode(s.fine, s.mode)) return s.mode == PSDR_IQ ? CK_FT_IQ : CK_FT_SSB;
    if (s.mode == PSDR_IQ) return CK_IQ;
    if (s.mode == PSDR_SAM) return sb_sam(s.mode, s.sam_sb) ? CK_SBSAM : CK_SAM;
    return CK_PLAIN;
}

// the window [l, r) clipped to a sideband of floor(audio_mid) = m: the upper one [max(l, m), r), the lower one
// [l, min(r, m + 1)), neither reaching outside the window (tuned USB / LSB and SAM-U / SAM-L place this range)
inline void placed_range(int &l, int &r, int m, bool upper) {
    if (upper)
        l = std::min(std::max(l, m), r);
    else
        r = m < r ? std::max(m + 1, l) : r;
}

// What a slot carries from batch to batch beside the state every kernel carries along, one rule each: a batch that does not
// continue the last one starts from zero.  (Asked of an unpaused slot, before its b_* snapshot moves on.)
// The SAM carrier tail: the last batch was SAM too, of either kind - a change of sideband does not interrupt it.
inline bool car_tail_from_zero(const AudioSlot &s) { return s.last_seq == 0 || s.b_mode != PSDR_SAM; }
// The tuned USB / LSB tail: the last batch was tuned, in the same mode.
inline bool ft_tail_from_zero(const AudioSlot &s) { return s.last_seq == 0 || !s.b_tuned || s.b_mode != s.mode; }
// The sideband SAM tail (the clipped baseband's): the last batch was SAM with the same sideband.
inline bool sb_tail_from_zero(const AudioSlot &s) { return s.last_seq == 0 || s.b_mode != PSDR_SAM || s.b_sam_sb != s.sam_sb; }
// The notch detector's state: auto-notch was switched (on: a fresh start; off: its entries go), or it is on and the window,
// floor(audio_mid) or the mode are not the last batch's.
inline bool detector_from_zero(const AudioSlot &s) {
    const bool moved = s.last_seq == 0 || s.l != s.b_l || s.r != s.b_r || std::floor(s.mid) != std::floor(s.b_mid) || s.mode != s.b_mode;
    return (s.auto_notch != 0) != s.b_auto || (s.auto_notch && (moved || s.auto_fresh));
}

// what a batch's plan depends on beside the slots
struct DemodFacts {
    int n = 0;        // audio FFT size: h = n / 2 samples per frame
    int nframes = 0;
    bool post_on = false;
    bool have_notch_tab = false;  // the context has the detector's state (its first auto-notch client allocated it)
    bool has_band = false;        // the spectrum is a window of bins [band_first, band_first + band_count)
    uint32_t band_first = 0, band_count = 0;
};

enum DemodVerdict { DP_OK, DP_BAND_OUTSIDE };
struct RingSpan {
    size_t off = 0, bytes = 0;
};
// a kernel's list inside the ring slot, as byte offsets: its ClientParams and its FtClient / SbClient beside them
struct RingList {
    size_t clients = 0, side = 0;
};
struct DemodPlan {
    DemodVerdict verdict = DP_OK;
    int bad_slot = -1, bad_l = 0, bad_r = 0;  // DP_BAND_OUTSIDE: the first slot whose window leaves the band
    // The batch's list: [0, nold) USB / LSB / AM / FM, [nold, nold + nsam) SAM, then ntssb tuned USB / LSB and nsb sideband SAM
    // clients - nact audio clients in all; behind them npaused clients with an empty stream (the post chain's), and from
    // iq_off on the niq untuned IQ clients.  The tuned list holds ntssb USB / LSB then ntiq IQ clients.
    int nold = 0, nsam = 0, ntssb = 0, ntiq = 0, nsb = 0, niq = 0, nact = 0, npaused = 0, ndet = 0, iq_off = 0;
    RingList plain, sam, iq, tssb, tiq, sb, det;
    size_t slot_ci = 0, notch = 0;  // [int x S] list index by slot; [int4 x S] manual notches by slot
    RingSpan copies[5];             // host to device, in this order
    int ncopies = 0;
    // what starts this batch from zero: element offsets into the carrier / tuned / sideband tails, slots of the detector
    std::vector<size_t> car_zero, ft_zero, sb_zero, det_zero;
    bool any_manual = false;  // the manual notch table is part of the batch (DemodArgs::notch_man)
    bool iq_notched = false;  // an untuned IQ client has a notch: k_demod_chain_iq_nz
    bool idle() const { return nact + niq + ntiq == 0; }  // nobody to demodulate: nothing is copied, zeroed or launched
};

// One batch: classifies the S slots, writes the ring slot's host image, moves the slots' carried fields on (state_cur,
// agc_reset, the b_* snapshot, last_seq, auto_fresh, ft_phi) and counts the batch in demod_seq.  A window outside the band
// refuses the batch before anything is touched.
inline DemodPlan demod_plan(AudioSlot *slots, size_t S, uint64_t &demod_seq, const DemodFacts &f, unsigned char *ring_host) {
    DemodPlan p;
    if (f.has_band)
        for (size_t i = 0; i < S; i++) {
            const AudioSlot &s = slots[i];
            // an empty window (a client between psdr_client_add and its first set_audio_range) reads no bin
            if (s.active && !s.paused && s.r > s.l && ((uint32_t)s.l < f.band_first || (uint64_t)s.r > (uint64_t)f.band_first + f.band_count)) {
                p.verdict = DP_BAND_OUTSIDE;
                p.bad_slot = (int)i, p.bad_l = s.l, p.bad_r = s.r;
                return p;
            }
        }
    const size_t h = (size_t)f.n / 2;
    ClientParams *const clients = (ClientParams *)ring_host;
    int *const slot_ci = (int *)(clients + S);
    int *const notch = (int *)(ring_host + notch_ring_off(S));
    ClientParams *const det = (ClientParams *)(ring_host + notch_ring_off(S) + S * NOTCH_ENTRY);
    p.slot_ci = S * sizeof(ClientParams), p.notch = notch_ring_off(S), p.det.clients = p.notch + S * NOTCH_ENTRY;

    // ---- the one walk: every unpaused client's kind, what of its state starts from zero, its notches, its snapshot
    demod_seq++;
    std::vector<int> of[CK_COUNT];  // the slots of each kind, in slot order
    for (size_t i = 0; i < S; i++) {
        AudioSlot &s = slots[i];
        const ClientKind kind = client_kind(s);
        if (kind == CK_NONE) continue;
        of[kind].push_back((int)i);
        if (kind == CK_PAUSED) continue;
        const size_t tail = ((size_t)s.state_cur * S + i) * h;  // (state_cur before this batch flips it)
        if (s.mode == PSDR_SAM && car_tail_from_zero(s)) p.car_zero.push_back(tail);
        if (kind == CK_FT_SSB && ft_tail_from_zero(s)) p.ft_zero.push_back(tail);
        if (kind == CK_SBSAM && sb_tail_from_zero(s)) p.sb_zero.push_back(tail);
        const bool manual = s.notch[1] > s.notch[0] || s.notch[3] > s.notch[2];
        if (manual) {
            if (!p.any_manual) std::fill(notch, notch + 4 * S, 0);
            p.any_manual = true;
            std::copy(s.notch, s.notch + 4, notch + 4 * i);
        }
        if ((manual || s.auto_notch) && kind == CK_IQ) p.iq_notched = true;
        if (f.have_notch_tab) {
            if (detector_from_zero(s)) p.det_zero.push_back(i);
            s.auto_fresh = false;
            if (s.auto_notch) {
                ClientParams &q = det[p.ndet++];
                q = ClientParams{};
                q.l = s.l, q.r = s.r, q.m_floor = (int)std::floor(s.mid), q.mode = s.mode, q.slot = (int)i;
            }
        }
        std::copy(s.notch, s.notch + 4, s.b_notch);
        s.b_auto = s.auto_notch != 0;
        s.last_seq = demod_seq;
        s.b_l = s.l, s.b_r = s.r, s.b_mid = s.mid, s.b_mode = s.mode, s.b_sam_sb = s.sam_sb;
        s.b_tuned = kind == CK_FT_SSB || kind == CK_FT_IQ;
    }
    p.nold = (int)of[CK_PLAIN].size(), p.nsam = (int)of[CK_SAM].size(), p.ntssb = (int)of[CK_FT_SSB].size();
    p.ntiq = (int)of[CK_FT_IQ].size(), p.nsb = (int)of[CK_SBSAM].size(), p.niq = (int)of[CK_IQ].size();
    const int nt = p.ntssb + p.ntiq;
    p.nact = p.nold + p.nsam + p.ntssb + p.nsb;
    p.sam.clients = (size_t)p.nold * sizeof(ClientParams);
    p.tssb.clients = ft_ring_off(S), p.tiq.clients = p.tssb.clients + (size_t)p.ntssb * sizeof(ClientParams);
    p.tssb.side = p.tssb.clients + (size_t)nt * sizeof(ClientParams), p.tiq.side = p.tssb.side + (size_t)p.ntssb * sizeof(FtClient);
    p.sb.clients = p.tssb.clients + (size_t)nt * (sizeof(ClientParams) + sizeof(FtClient));
    p.sb.side = p.sb.clients + (size_t)p.nsb * sizeof(ClientParams);

    // One client of the batch's list: the window and the mode it is demodulated with; its double-buffered state flips.  To the
    // post chain a PSDR_IQ client is a paused one (no audio of its own this batch): a pending AGC reset stays with the slot.
    auto listed = [&](int i) {
        AudioSlot &s = slots[i];
        const bool audio = s.mode != PSDR_IQ;
        ClientParams q{};
        q.l = s.l, q.r = s.r, q.m_floor = (int)std::floor(s.mid), q.mode = s.mode, q.slot = i;
        q.state_cur = s.state_cur;
        s.state_cur ^= 1;
        q.paused = audio ? 0 : 1;
        if (audio && f.post_on) {
            q.agc_reset = s.agc_reset;
            s.agc_reset = 0;
        }
        return q;
    };
    // ... and on a list of its own as the kernels see it: the placed range, the AM / FM placement
    auto placed = [](ClientParams q, bool clip, bool upper) {
        q.mode = PSDR_AM;
        if (clip) placed_range(q.l, q.r, q.m_floor, upper);
        return q;
    };
    // A tuned client's entry k of the tuned list; beside it phase, step and the whole window.  The phase moves on by the
    // batch's samples here, from the snapshot.
    auto list_tuned = [&](int k, const ClientParams &q) {
        AudioSlot &s = slots[q.slot];
        ((ClientParams *)(ring_host + p.tssb.clients))[k] = placed(q, s.mode != PSDR_IQ, s.mode == PSDR_USB);
        FtClient &t = ((FtClient *)(ring_host + p.tssb.side))[k];
        t.step = (uint32_t)std::floor((s.mid - std::floor(s.mid)) * 4294967296.0 / f.n + 0.5);
        t.phi0 = s.ft_phi;
        t.l = q.l, t.r = q.r;
        s.ft_phi += (uint32_t)f.nframes * (uint32_t)(f.n / 2) * t.step;
    };

    // ---- the lists, in their fixed order.  The audio clients (the post chain takes all nact, in any order: it walks the slots
    // through slot_ci): plain, SAM, tuned USB / LSB, sideband SAM
    int k = 0;
    for (int i : of[CK_PLAIN]) clients[k++] = listed(i);
    for (int i : of[CK_SAM]) clients[k++] = listed(i);
    for (int j = 0; j < p.ntssb; j++, k++) list_tuned(j, clients[k] = listed(of[CK_FT_SSB][j]));
    for (int j = 0; j < p.nsb; j++, k++) {
        const AudioSlot &s = slots[of[CK_SBSAM][j]];
        clients[k] = listed(of[CK_SBSAM][j]);
        ((ClientParams *)(ring_host + p.sb.clients))[j] = placed(clients[k], true, s.sam_sb == PSDR_SAM_UPPER);
        ((SbClient *)(ring_host + p.sb.side))[j] = SbClient{clients[k].l, clients[k].r, s.sam_sb, 0};
    }
    if (f.post_on) {
        std::fill(slot_ci, slot_ci + S, -1);
        for (int j = 0; j < p.nact; j++) slot_ci[clients[j].slot] = j;
    }
    // Behind them, for the post chain alone (its double-buffered histories alternate per batch for every listed client, state
    // unchanged), who has a history and no audio of its own this batch, with an empty stream: the paused clients (signal_loop
    // never calls send_audio for a client whose socket is backed up, src/websocket.cpp:170-176; a pending AGC reset stays
    // pending until the client's next batch), the tuned IQ clients as paused copies (the kernels take them from the tuned
    // list), and the untuned IQ clients, who head their kernels' list.  A fresh client (agc_reset == 2) has no history.
    const bool chain = f.post_on && p.nact > 0;
    auto list_paused = [&](const ClientParams &q) {
        slot_ci[q.slot] = p.nact + p.npaused;
        clients[p.nact + p.npaused++] = q;
    };
    if (chain)
        for (int i : of[CK_PAUSED])
            if (slots[i].agc_reset != 2) {
                ClientParams q{};
                q.slot = i, q.state_cur = slots[i].state_cur, q.paused = 1;
                list_paused(q);
            }
    for (int j = 0; j < p.ntiq; j++) {
        const ClientParams q = listed(of[CK_FT_IQ][j]);
        list_tuned(p.ntssb + j, q);
        if (chain && slots[q.slot].agc_reset != 2) list_paused(q);
    }
    if (p.niq > 0) {
        p.iq_off = k = p.nact + p.npaused;
        for (int fresh = 0; fresh < 2; fresh++)
            for (int i : of[CK_IQ])
                if ((slots[i].agc_reset == 2) == (fresh == 1)) {
                    clients[k] = listed(i);
                    if (chain && !fresh) slot_ci[i] = k, p.npaused++;
                    k++;
                }
    }
    p.iq.clients = (size_t)p.iq_off * sizeof(ClientParams);

    // ---- the copies
    if (p.idle()) return p;
    auto copy = [&](size_t off, size_t bytes) { p.copies[p.ncopies++] = RingSpan{off, bytes}; };
    copy(0, f.post_on ? S * (sizeof(ClientParams) + sizeof(int)) : (size_t)(p.nact + p.niq) * sizeof(ClientParams));
    if (nt > 0) copy(p.tssb.clients, (size_t)nt * (sizeof(ClientParams) + sizeof(FtClient)));
    if (p.nsb > 0) copy(p.sb.clients, (size_t)p.nsb * (sizeof(ClientParams) + sizeof(SbClient)));
    if (p.any_manual) copy(p.notch, S * NOTCH_ENTRY);
    if (p.ndet > 0) copy(p.det.clients, (size_t)p.ndet * sizeof(ClientParams));
    return p;
}

}  // namespace psdr

// demod.hip - the audio clients (AudioClient, src/signal.h:53-123) and their batched demodulation: signal_loop +
// AudioClient::send_audio up to the NaN guard (src/websocket.cpp:156-185, src/signal.cpp:102-275) for every client and
// every frame of a batch.  (The read-back of its results: fetch.hip.)
#include "ctx.h"
#include "demod.h"
#include "noise.h"
#include "squelch.h"
#include "audiofilter.h"
#include "nr.h"
#include "anb.h"
#include "tone.h"
#include "cw.h"
#include "rtty.h"
#include "psk.h"
#include "fax.h"

// The context's first client of an optional feature (ctx.h: the structs behind `iq`): what the feature allocates is built whole
// and only then moved in, so a failed call leaves the context as it was.  msg: the failure's text, with the bytes and the
// underlying error.  Under mtx.
template <class Feature>
static int first_use(psdr_ctx *c, Feature &have, const char *msg) {
    if (have) return PSDR_OK;
    HIPCHK(hipSetDevice(c->device));
    Feature fresh;
    if (fresh.alloc(*c)) {
        const std::string why = psdr_last_error();
        return fail(PSDR_ERR_NOMEM, msg, Feature::bytes(*c), why.c_str());
    }
    have = std::move(fresh);
    return PSDR_OK;
}
static int first_tuned(psdr_ctx *c) { return first_use(c, c->ft, "tuned USB / LSB tails (%zu bytes): %s"); }
static int first_sideband(psdr_ctx *c) { return first_use(c, c->sb, "sideband SAM tails (%zu bytes): %s"); }
static int first_auto_notch(psdr_ctx *c) { return first_use(c, c->notch, "auto-notch state (%zu bytes): %s"); }
static int first_noise_reduction(psdr_ctx *c) { return first_use(c, c->nr, "noise reduction state and tables (%zu bytes): %s"); }
static int first_audio_blanker(psdr_ctx *c) { return first_use(c, c->anb, "audio blanker state (%zu bytes): %s"); }
static int first_tone_decoder(psdr_ctx *c) { return first_use(c, c->tone, "tone decoder state, records and tables (%zu bytes): %s"); }
static int first_cw_decoder(psdr_ctx *c) { return first_use(c, c->cw, "CW decoder state, text, records and tables (%zu bytes): %s"); }
static int first_rtty_decoder(psdr_ctx *c) { return first_use(c, c->rtty, "RTTY decoder state, text, records and tables (%zu bytes): %s"); }
static int first_psk_decoder(psdr_ctx *c) { return first_use(c, c->psk, "PSK decoder state, text, records and tables (%zu bytes): %s"); }
static int first_fax_decoder(psdr_ctx *c) { return first_use(c, c->fax, "fax decoder state, line rings, records and tables (%zu bytes): %s"); }
// the detector's state of one slot back to zero: sums, counter, both automatic entries (stream-ordered on `side`)
static int notch_zero(psdr_ctx *c, size_t slot) {
    HIPCHK(hipMemsetAsync(c->notch.acc + slot * (size_t)c->n, 0, (size_t)c->n * sizeof(float), c->side));
    HIPCHK(hipMemsetAsync(c->notch.cnt + slot, 0, sizeof(int), c->side));
    HIPCHK(hipMemsetAsync(c->notch.tab + slot, 0, sizeof(int4), c->side));
    return PSDR_OK;
}
int psdr::check_slot(psdr_ctx *c, int id) {
    if (id < 0 || id >= (int)c->aslots.size() || !c->aslots[id].active)
        return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
    return PSDR_OK;
}
extern "C" int psdr_client_add(psdr_ctx *c, int *id_out) {
    if (!c || !id_out) return fail(PSDR_ERR_INVALID, "null argument");
    if (c->n <= 0) return fail(PSDR_ERR_STATE, "context created with audio_fft_size 0");
    std::lock_guard<std::mutex> lk(c->mtx);
    HIPCHK(hipSetDevice(c->device));
    for (size_t i = 0; i < c->aslots.size(); i++)
        if (!c->aslots[i].active) {
            AudioSlot &s = c->aslots[i];
            if (c->opt_fine_tune) PSDRCHK(first_tuned(c));  // (a new client is a USB client: a tuned one under PSDR_OPT_FINE_TUNE)
            if (c->opt_auto_notch) PSDRCHK(first_auto_notch(c));
            if (c->notch) PSDRCHK(notch_zero(c, i));  // (the previous occupant's automatic entries do not outlive it)
            double nr_depth = 0, nr_beta = 0;
            if (c->opt_nr) {
                nr_preset(c->opt_nr, &nr_depth, &nr_beta);
                PSDRCHK(first_noise_reduction(c));
            }
            double anb_thr = 0;
            int anb_width = 0;
            if (c->opt_anb) {
                anb_preset(c->opt_anb, &anb_thr, &anb_width);
                PSDRCHK(first_audio_blanker(c));
            }
            s = AudioSlot();
            if (c->opt_nr) nr_apply(s, 1, nr_depth, nr_beta);
            if (c->opt_anb) anb_apply(s, 1, anb_thr, anb_width);
            s.active = true;
            s.fine = c->opt_fine_tune;
            s.sam_sb = c->opt_sam_sideband;  // (a new client is a USB client: the value waits for PSDR_SAM)
            s.auto_notch = c->opt_auto_notch;
            s.born = ++c->slot_births;
            // a fresh AudioClient starts from zeroed buffers (src/signal.h:42-51)
            const size_t S = c->aslots.size(), h = (size_t)c->n / 2;
            for (int b = 0; b < 2; b++) {
                HIPCHK(hipMemsetAsync(c->d_real_prev + ((size_t)b * S + i) * h, 0, h * sizeof(float),
                                      c->side));
                HIPCHK(hipMemsetAsync(c->d_bb_tail + ((size_t)b * S + i) * h, 0, h * sizeof(cf),
                                      c->side));
                HIPCHK(hipMemsetAsync(c->d_bb_last + ((size_t)b * S + i), 0, sizeof(cf), c->side));
            }
            *id_out = (int)i;
            return PSDR_OK;
        }
    return fail(PSDR_ERR_NOMEM, "all %zu audio client slots are in use", c->aslots.size());
}
extern "C" int psdr_client_remove(psdr_ctx *c, int id) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    PSDRCHK(check_slot(c, id));
    c->aslots[id].active = false;
    return PSDR_OK;
}
extern "C" int psdr_client_set_audio_range(psdr_ctx *c, int id, int l, double mid, int r) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    PSDRCHK(check_slot(c, id));
    // the reference does not validate here (src/signal.cpp:81-94); a range outside the
    // spectrum would read out of bounds there, so it is refused here
    if (l < 0 || r < l || (size_t)r > c->R || r - l > c->n)
        return fail(PSDR_ERR_INVALID, "range [%d,%d) outside the spectrum or wider than %d", l, r, c->n);
    AudioSlot &s = c->aslots[id];
    s.l = l;
    s.r = r;
    s.mid = mid;
    return PSDR_OK;
}
extern "C" int psdr_client_on_window_message(psdr_ctx *c, int id, int l, double mid, int r) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        PSDRCHK(check_slot(c, id));
    }
    const int R = (int)c->R;  // src/signal.cpp:305-311
    if (l < 0 || l >= R || r < 0 || r >= R || l > r)
        return fail(PSDR_ERR_INVALID, "window [%d,%d] rejected", l, r);
    if (r - l > c->n) return fail(PSDR_ERR_INVALID, "window wider than audio_fft_size");
    return psdr_client_set_audio_range(c, id, l, mid, r);
}
// signal_loop's slow-client rule (src/websocket.cpp:170-176): a client with more than 50 kB queued on its socket gets no
// send_audio call for the frame - nothing of its state moves (src/signal.cpp:200-203, 273-284).  A paused client sits
// out every demodulation batch until it is resumed; its results read as PSDR_ERR_NO_DATA meanwhile.
extern "C" int psdr_client_set_paused(psdr_ctx *c, int id, int paused) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    PSDRCHK(check_slot(c, id));
    c->aslots[id].paused = paused != 0;
    return PSDR_OK;
}
extern "C" int psdr_client_set_audio_demodulation(psdr_ctx *c, int id, int mode) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    PSDRCHK(check_slot(c, id));
    if (mode < PSDR_USB || mode > PSDR_SAM) return fail(PSDR_ERR_INVALID, "unknown mode %d", mode);
    if (mode == PSDR_SAM && !sam_size_served(c->n))
        return fail(PSDR_ERR_UNSUPPORTED, "PSDR_SAM needs audio_fft_size < %d (this context: %d): the carrier's direct sum indexes its twiddles with a 32-bit product", PSDR_SAM_MAX_AUDIO_FFT, c->n);
    // (the mode changes only once everything it needs exists)
    if (mode == PSDR_IQ) PSDRCHK(first_use(c, c->iq, "IQ rows (2 x %zu bytes): %s"));
    if (mode == PSDR_SAM && !c->sam) {
        if (c->cfg.audio_rate <= 0) return fail(PSDR_ERR_STATE, "PSDR_SAM needs audio_rate > 0 (the carrier low-pass is 500 Hz)");
        PSDRCHK(first_use(c, c->sam, "carrier tails and records (%zu bytes): %s"));
    }
    if (tuned_mode(c->aslots[id].fine, mode) && mode != PSDR_IQ) PSDRCHK(first_tuned(c));
    if (sb_sam(mode, c->aslots[id].sam_sb)) PSDRCHK(first_sideband(c));
    c->aslots[id].mode = mode;
    if (c->aslots[id].agc_reset == 0) c->aslots[id].agc_reset = 1;  // src/signal.cpp:316-328: resets the AGC
    return PSDR_OK;
}
extern "C" int psdr_client_set_fine_tune(psdr_ctx *c, int id, int on) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    PSDRCHK(check_slot(c, id));
    AudioSlot &s = c->aslots[id];
    if (tuned_mode(on, s.mode) && s.mode != PSDR_IQ) PSDRCHK(first_tuned(c));
    s.fine = on ? 1 : 0;
    return PSDR_OK;
}
extern "C" int psdr_client_set_sam_sideband(psdr_ctx *c, int id, int sideband) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    PSDRCHK(check_slot(c, id));
    if (sideband < PSDR_SAM_BOTH || sideband > PSDR_SAM_LOWER) return fail(PSDR_ERR_INVALID, "unknown SAM sideband %d", sideband);
    AudioSlot &s = c->aslots[id];
    if (sb_sam(s.mode, sideband)) PSDRCHK(first_sideband(c));
    s.sam_sb = sideband;
    return PSDR_OK;
}
// A manual notch: [first, end) = [floor(centre - width/2 + 0.5), floor(centre + width/2 + 0.5)), at least one bin; host code
// alone (psdr_debug_notch_interval: tests/test_notch_host.py drives it without a device).  The ends are kept inside +-2^30: no spectrum reaches there.
static void notch_interval(double centre, double width, int *first, int *end) {
    const double lim = 1073741824.0;
    const double a = std::min(std::max(std::floor(centre - width / 2 + 0.5), -lim), lim);
    const double b = std::min(std::max(std::floor(centre + width / 2 + 0.5), -lim), lim);
    *first = (int)a;
    *end = b <= a ? (int)a + 1 : (int)b;
}
// (debug entries, beside psdr_debug_trace: exported for the tests, not part of include/psdr.h)
extern "C" int psdr_debug_notch_interval(double centre_bin, double width_bins, int *first, int *end) {
    if (!first || !end) return fail(PSDR_ERR_INVALID, "null argument");
    if (!std::isfinite(centre_bin) || !std::isfinite(width_bins)) return fail(PSDR_ERR_INVALID, "non-finite notch");
    if (width_bins <= 0) {
        *first = *end = 0;
        return PSDR_OK;
    }
    notch_interval(centre_bin, width_bins, first, end);
    return PSDR_OK;
}
extern "C" int psdr_client_set_notch(psdr_ctx *c, int id, int index, double centre_bin, double width_bins) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    PSDRCHK(check_slot(c, id));
    if (index < 0 || index >= PSDR_NOTCH_MANUAL) return fail(PSDR_ERR_INVALID, "notch index %d outside 0..%d", index, PSDR_NOTCH_MANUAL - 1);
    if (!std::isfinite(centre_bin) || !std::isfinite(width_bins)) return fail(PSDR_ERR_INVALID, "non-finite notch");
    if (width_bins > (double)c->n) return fail(PSDR_ERR_INVALID, "notch wider than audio_fft_size %d", c->n);
    AudioSlot &s = c->aslots[id];
    if (width_bins <= 0)
        s.notch[2 * index] = s.notch[2 * index + 1] = 0;
    else
        notch_interval(centre_bin, width_bins, &s.notch[2 * index], &s.notch[2 * index + 1]);
    return PSDR_OK;
}
extern "C" int psdr_client_set_auto_notch(psdr_ctx *c, int id, int on) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    PSDRCHK(check_slot(c, id));
    if (on) PSDRCHK(first_auto_notch(c));
    AudioSlot &s = c->aslots[id];
    if (on && !s.auto_notch) s.auto_fresh = true;
    s.auto_notch = on ? 1 : 0;
    return PSDR_OK;
}
extern "C" int psdr_client_set_squelch(psdr_ctx *c, int id, int on, double open_db, double close_db, int attack_frames, int hang_frames) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    switch (squelch_check(c->aslots.data(), c->aslots.size(), id, on, open_db, close_db, attack_frames, hang_frames)) {
    case SQ_OK: break;
    case SQ_BAD_ID: return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
    case SQ_BAD_DB: return fail(PSDR_ERR_INVALID, "squelch thresholds %g dB / %g dB: finite values inside [-300, 300]", open_db, close_db);
    case SQ_CLOSE_ABOVE_OPEN: return fail(PSDR_ERR_INVALID, "squelch: close_db %g above open_db %g", close_db, open_db);
    case SQ_BAD_ATTACK: return fail(PSDR_ERR_INVALID, "squelch: attack_frames %d outside 1..%d", attack_frames, SQUELCH_FRAMES_MAX);
    case SQ_BAD_HANG: return fail(PSDR_ERR_INVALID, "squelch: hang_frames %d outside 0..%d", hang_frames, SQUELCH_FRAMES_MAX);
    }
    if (on) PSDRCHK(first_use(c, c->squelch, "squelch flags, state and table (%zu bytes): %s"));
    squelch_apply(c->aslots[id], on, open_db, close_db, attack_frames, hang_frames);
    return PSDR_OK;
}
extern "C" int psdr_client_set_noise_floor(psdr_ctx *c, int id, int on) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    switch (noise_floor_check(c->aslots.data(), c->aslots.size(), id, on, c->cfg.audio_rate)) {
    case NF_OK: break;
    case NF_BAD_ID: return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
    case NF_NO_RATE: return fail(PSDR_ERR_STATE, "noise floor: the context's audio_rate %d is not positive", c->cfg.audio_rate);
    case NF_IN_USE: return fail(PSDR_ERR_STATE, "noise floor: client %d's squelch reference is PSDR_SQ_NOISE (psdr_client_set_squelch_reference first)", id);
    }
    if (on) PSDRCHK(first_use(c, c->noise, "noise floor sums, records, rows and table (%zu bytes): %s"));
    noise_floor_apply(c->aslots[id], on);
    return PSDR_OK;
}
extern "C" int psdr_client_set_squelch_reference(psdr_ctx *c, int id, int ref) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    switch (squelch_reference_check(c->aslots.data(), c->aslots.size(), id, ref)) {
    case SR_OK: break;
    case SR_BAD_ID: return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
    case SR_BAD_VALUE: return fail(PSDR_ERR_INVALID, "unknown squelch reference %d", ref);
    case SR_NOISE_OFF: return fail(PSDR_ERR_STATE, "PSDR_SQ_NOISE: client %d's noise floor is off (psdr_client_set_noise_floor first)", id);
    }
    squelch_reference_apply(c->aslots[id], ref);
    return PSDR_OK;
}
extern "C" int psdr_client_set_audio_filter(psdr_ctx *c, int id, int nsections, const psdr_biquad *sections) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    switch (audio_filter_check(c->aslots.data(), c->aslots.size(), id, nsections, sections)) {
    case AF_OK: break;
    case AF_BAD_ID: return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
    case AF_BAD_COUNT: return fail(PSDR_ERR_INVALID, "audio filter: %d sections outside 0..%d", nsections, PSDR_AUDIO_FILTER_SECTIONS);
    case AF_NULL: return fail(PSDR_ERR_INVALID, "audio filter: %d sections and a null pointer", nsections);
    case AF_NONFINITE: return fail(PSDR_ERR_INVALID, "audio filter: a coefficient that is not a finite f32 number");
    case AF_UNSTABLE: return fail(PSDR_ERR_INVALID, "audio filter: a section that is not stable (|a2| < 1 and |a1| < 1 + a2)");
    case AF_POLE: return fail(PSDR_ERR_INVALID, "audio filter: a pole radius above %g", AF_POLE_MAX);
    }
    if (nsections > 0) PSDRCHK(first_use(c, c->af, "audio filter state and table (%zu bytes): %s"));
    audio_filter_apply(c->aslots[id], nsections, sections);
    return PSDR_OK;
}
extern "C" int psdr_client_set_noise_reduction(psdr_ctx *c, int id, int on, double depth_db, double beta) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    switch (nr_check(c->aslots.data(), c->aslots.size(), id, on, depth_db, beta, c->cfg.audio_rate)) {
    case NR_OK: break;
    case NR_BAD_ID: return fail(PSDR_ERR_INVALID, "noise reduction: id %d outside 0..%d", id, (int)c->aslots.size() - 1);
    case NR_INACTIVE: return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
    case NR_IQ: return fail(PSDR_ERR_INVALID, "noise reduction: client %d is a PSDR_IQ client, which has no audio rows", id);
    case NR_NONFINITE: return fail(PSDR_ERR_INVALID, "noise reduction: depth_db or beta is not a finite number");
    case NR_BAD_DEPTH: return fail(PSDR_ERR_INVALID, "noise reduction: depth_db %g outside [%g, %g]", depth_db, NR_DEPTH_MIN, NR_DEPTH_MAX);
    case NR_BAD_BETA: return fail(PSDR_ERR_INVALID, "noise reduction: beta %g outside [%g, %g]", beta, NR_BETA_MIN, NR_BETA_MAX);
    case NR_NO_RATE: return fail(PSDR_ERR_STATE, "noise reduction: the context's audio_rate %d is not positive", c->cfg.audio_rate);
    }
    if (on) PSDRCHK(first_noise_reduction(c));
    nr_apply(c->aslots[id], on, depth_db, beta);
    return PSDR_OK;
}
extern "C" int psdr_noise_reduction_preset(int kind, double *depth_db, double *beta) {
    if (!depth_db || !beta) return fail(PSDR_ERR_INVALID, "null argument");
    if (!nr_preset(kind, depth_db, beta)) return fail(PSDR_ERR_INVALID, "noise reduction preset: unknown kind %d", kind);
    return PSDR_OK;
}
// (a debug entry, beside psdr_debug_audio_filter_ptrs: exported for the tests, not part of include/psdr.h)  out[0..1]: the noise
// reduction's table and state (null until the context's first such client)
extern "C" int psdr_debug_noise_reduction_ptrs(psdr_ctx *c, const void *out[2]) {
    if (!c || !out) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    out[0] = c->nr.tab.d.get(), out[1] = c->nr.state.get();
    return PSDR_OK;
}
extern "C" int psdr_client_set_audio_blanker(psdr_ctx *c, int id, int on, double threshold, int width) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    switch (anb_check(c->aslots.data(), c->aslots.size(), id, on, threshold, width)) {
    case ANB_OK: break;
    case ANB_BAD_ID: return fail(PSDR_ERR_INVALID, "audio blanker: id %d outside 0..%d", id, (int)c->aslots.size() - 1);
    case ANB_INACTIVE: return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
    case ANB_IQ: return fail(PSDR_ERR_INVALID, "audio blanker: client %d is a PSDR_IQ client, which has no audio rows", id);
    case ANB_NONFINITE: return fail(PSDR_ERR_INVALID, "audio blanker: threshold is not a finite number");
    case ANB_BAD_THRESHOLD: return fail(PSDR_ERR_INVALID, "audio blanker: threshold %g outside [%g, %g]", threshold, ANB_THR_MIN, ANB_THR_MAX);
    case ANB_BAD_WIDTH: return fail(PSDR_ERR_INVALID, "audio blanker: width %d is not an odd number in %d..%d", width, ANB_WIDTH_MIN, ANB_WMAX);
    }
    if (on) PSDRCHK(first_audio_blanker(c));
    anb_apply(c->aslots[id], on, threshold, width);
    return PSDR_OK;
}
extern "C" int psdr_audio_blanker_preset(int kind, double *threshold, int *width) {
    if (!threshold || !width) return fail(PSDR_ERR_INVALID, "null argument");
    if (!anb_preset(kind, threshold, width)) return fail(PSDR_ERR_INVALID, "audio blanker preset: unknown kind %d", kind);
    return PSDR_OK;
}
// the totals of the client's blanker state; psdr_read_audio's rule for who has something to read
extern "C" int psdr_read_audio_blanker(psdr_ctx *c, int id, uint64_t *impulses, uint64_t *samples) {
    if (!c || !impulses || !samples) return fail(PSDR_ERR_INVALID, "null argument");
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        if (id < 0 || (size_t)id >= c->aslots.size()) return fail(PSDR_ERR_INVALID, "audio blanker: id %d outside 0..%d", id, (int)c->aslots.size() - 1);
        const AudioSlot &s = c->aslots[id];
        if (!s.active) return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
        if (c->demod_seq == 0 || s.last_seq != c->demod_seq) return fail(PSDR_ERR_NO_DATA, "client %d was not part of the last demodulation batch", id);
        if (s.b_mode == PSDR_IQ) return fail(PSDR_ERR_NO_DATA, "client %d was demodulated as PSDR_IQ in the last batch", id);
        if (!s.anb_on || s.anb_fresh || !c->anb) return fail(PSDR_ERR_NO_DATA, "client %d had no audio blanker in the last demodulation batch", id);
    }
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    uint64_t v[2] = {0, 0};
    HIPCHK(hipMemcpy(v, &(c->anb.state + (size_t)id)->impulses, sizeof(v), hipMemcpyDeviceToHost));
    *impulses = v[0], *samples = v[1];
    return PSDR_OK;
}
// (a debug entry, beside psdr_debug_noise_reduction_ptrs: exported for the tests, not part of include/psdr.h)  out[0..1]: the audio
// blanker's table and state (null until the context's first such client)
extern "C" int psdr_debug_audio_blanker_ptrs(psdr_ctx *c, const void *out[2]) {
    if (!c || !out) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    out[0] = c->anb.tab.d.get(), out[1] = c->anb.state.get();
    return PSDR_OK;
}
extern "C" int psdr_client_set_tone_decoder(psdr_ctx *c, int id, const psdr_tone_config *cfg) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    switch (tone_check(c->aslots.data(), c->aslots.size(), id, cfg, c->cfg.audio_rate)) {
    case TONE_OK: break;
    case TONE_BAD_ID: return fail(PSDR_ERR_INVALID, "tone decoder: id %d outside 0..%d", id, (int)c->aslots.size() - 1);
    case TONE_INACTIVE: return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
    case TONE_IQ: return fail(PSDR_ERR_INVALID, "tone decoder: client %d is a PSDR_IQ client, which has no audio rows", id);
    case TONE_BAD_WANT: return fail(PSDR_ERR_INVALID, "tone decoder: want %d outside %d..%d", cfg->want, PSDR_TONE_ANY, TONE_N - 1);
    case TONE_BAD_GATE: return fail(PSDR_ERR_INVALID, "tone decoder: gate %d outside 0..1", cfg->gate);
    case TONE_BAD_SNR: return fail(PSDR_ERR_INVALID, "tone decoder: snr_db %g is not a finite number inside [%g, %g]", cfg->snr_db, TONE_SNR_MIN, TONE_SNR_MAX);
    case TONE_BAD_LEVEL: return fail(PSDR_ERR_INVALID, "tone decoder: min_level %g is not a finite number at or above 0", cfg->min_level);
    case TONE_BAD_ATTACK: return fail(PSDR_ERR_INVALID, "tone decoder: attack_blocks %d outside 1..%d", cfg->attack_blocks, TONE_BLOCKS_MAX);
    case TONE_BAD_HANG: return fail(PSDR_ERR_INVALID, "tone decoder: hang_blocks %d outside 0..%d", cfg->hang_blocks, TONE_BLOCKS_MAX);
    case TONE_BAD_RATE: return fail(PSDR_ERR_STATE, "tone decoder: the context's audio_rate %d is outside [%d, %d]", c->cfg.audio_rate, TONE_RATE_MIN, TONE_RATE_MAX);
    }
    if (cfg) PSDRCHK(first_tone_decoder(c));
    tone_apply(c->aslots[id], cfg);
    return PSDR_OK;
}
extern "C" int psdr_tone_defaults(double audio_rate, psdr_tone_config *out) {
    if (!out) return fail(PSDR_ERR_INVALID, "null argument");
    if (!tone_defaults(audio_rate, out)) return fail(PSDR_ERR_INVALID, "tone decoder defaults: audio_rate %g outside [%d, %d]", audio_rate, TONE_RATE_MIN, TONE_RATE_MAX);
    return PSDR_OK;
}
extern "C" int psdr_tone_table(const double **hz, int *n) {
    if (!hz || !n) return fail(PSDR_ERR_INVALID, "null argument");
    *hz = TONE_HZ, *n = TONE_N;
    return PSDR_OK;
}
extern "C" int psdr_client_set_cw_decoder(psdr_ctx *c, int id, const psdr_cw_config *cfg) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    switch (cw_check(c->aslots.data(), c->aslots.size(), id, cfg, c->cfg.audio_rate)) {
    case CW_OK: break;
    case CW_BAD_ID: return fail(PSDR_ERR_INVALID, "CW decoder: id %d outside 0..%d", id, (int)c->aslots.size() - 1);
    case CW_INACTIVE: return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
    case CW_IQ: return fail(PSDR_ERR_INVALID, "CW decoder: client %d is a PSDR_IQ client, which has no audio rows", id);
    case CW_BAD_PITCH: return fail(PSDR_ERR_INVALID, "CW decoder: pitch_hz %g is not a finite number inside [%g, %g]", cfg->pitch_hz, CW_PITCH_MIN, CW_PITCH_MAX);
    case CW_BAD_SEARCH: return fail(PSDR_ERR_INVALID, "CW decoder: search_hz %g is not a finite number inside [%g, %g]", cfg->search_hz, CW_SEARCH_MIN, CW_SEARCH_MAX);
    case CW_BAD_WPM: return fail(PSDR_ERR_INVALID, "CW decoder: wpm %g is not a finite number inside [%g, %g]", cfg->wpm, CW_WPM_MIN, CW_WPM_MAX);
    case CW_BAD_TRACK: return fail(PSDR_ERR_INVALID, "CW decoder: track_speed %d outside 0..1", cfg->track_speed);
    case CW_BAD_SNR: return fail(PSDR_ERR_INVALID, "CW decoder: snr_db %g is not a finite number inside [%g, %g]", cfg->snr_db, CW_SNR_MIN, CW_SNR_MAX);
    case CW_BAD_RATE: return fail(PSDR_ERR_STATE, "CW decoder: the context's audio_rate %d is outside [%d, %d]", c->cfg.audio_rate, CW_RATE_MIN, CW_RATE_MAX);
    }
    if (cfg) PSDRCHK(first_cw_decoder(c));
    cw_apply(c->aslots[id], cfg, c->cfg.audio_rate);
    return PSDR_OK;
}
extern "C" int psdr_cw_defaults(double audio_rate, psdr_cw_config *out) {
    if (!out) return fail(PSDR_ERR_INVALID, "null argument");
    if (!cw_defaults(audio_rate, out)) return fail(PSDR_ERR_INVALID, "CW decoder defaults: audio_rate %g outside [%d, %d]", audio_rate, CW_RATE_MIN, CW_RATE_MAX);
    return PSDR_OK;
}
extern "C" int psdr_client_set_rtty_decoder(psdr_ctx *c, int id, const psdr_rtty_config *cfg) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    switch (rtty_check(c->aslots.data(), c->aslots.size(), id, cfg, c->cfg.audio_rate)) {
    case RTTY_OK: break;
    case RTTY_BAD_ID: return fail(PSDR_ERR_INVALID, "RTTY decoder: id %d outside 0..%d", id, (int)c->aslots.size() - 1);
    case RTTY_INACTIVE: return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
    case RTTY_IQ: return fail(PSDR_ERR_INVALID, "RTTY decoder: client %d is a PSDR_IQ client, which has no audio rows", id);
    case RTTY_BAD_MARK: return fail(PSDR_ERR_INVALID, "RTTY decoder: mark_hz %g is not a finite number inside [%g, %g]", cfg->mark_hz, RTTY_MARK_MIN, RTTY_MARK_MAX);
    case RTTY_BAD_SHIFT: return fail(PSDR_ERR_INVALID, "RTTY decoder: shift_hz %g is not a finite number of magnitude inside [%g, %g]", cfg->shift_hz, RTTY_SHIFT_MIN, RTTY_SHIFT_MAX);
    case RTTY_BAD_BAUD: return fail(PSDR_ERR_INVALID, "RTTY decoder: baud %g is not a finite number inside [%g, %g]", cfg->baud, RTTY_BAUD_MIN, RTTY_BAUD_MAX);
    case RTTY_BAD_USOS: return fail(PSDR_ERR_INVALID, "RTTY decoder: usos %d outside 0..1", cfg->usos);
    case RTTY_BAD_SEARCH: return fail(PSDR_ERR_INVALID, "RTTY decoder: search_hz %g is not a finite number inside [%g, %g]", cfg->search_hz, RTTY_SEARCH_MIN, RTTY_SEARCH_MAX);
    case RTTY_BAD_SNR: return fail(PSDR_ERR_INVALID, "RTTY decoder: snr_db %g is not a finite number inside [%g, %g]", cfg->snr_db, RTTY_SNR_MIN, RTTY_SNR_MAX);
    case RTTY_BAD_RATE: return fail(PSDR_ERR_STATE, "RTTY decoder: the context's audio_rate %d is outside [%d, %d]", c->cfg.audio_rate, RTTY_RATE_MIN, RTTY_RATE_MAX);
    case RTTY_BAD_BAND: return fail(PSDR_ERR_STATE, "RTTY decoder: the tones %g and %g Hz with %g Hz to either side do not lie inside [%g Hz, %g of the audio_rate %d]", cfg->mark_hz, cfg->mark_hz + cfg->shift_hz, RTTY_EDGE, RTTY_BOTTOM, RTTY_TOP, c->cfg.audio_rate);
    }
    if (cfg) PSDRCHK(first_rtty_decoder(c));
    rtty_apply(c->aslots[id], cfg, c->cfg.audio_rate);
    return PSDR_OK;
}
extern "C" int psdr_rtty_defaults(double audio_rate, psdr_rtty_config *out) {
    if (!out) return fail(PSDR_ERR_INVALID, "null argument");
    if (!rtty_defaults(audio_rate, out)) return fail(PSDR_ERR_INVALID, "RTTY decoder defaults: audio_rate %g outside [%d, %d]", audio_rate, RTTY_RATE_MIN, RTTY_RATE_MAX);
    return PSDR_OK;
}
extern "C" int psdr_client_set_psk_decoder(psdr_ctx *c, int id, const psdr_psk_config *cfg) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    switch (psk_check(c->aslots.data(), c->aslots.size(), id, cfg, c->cfg.audio_rate)) {
    case PSK_OK: break;
    case PSK_BAD_ID: return fail(PSDR_ERR_INVALID, "PSK decoder: id %d outside 0..%d", id, (int)c->aslots.size() - 1);
    case PSK_INACTIVE: return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
    case PSK_IQ: return fail(PSDR_ERR_INVALID, "PSK decoder: client %d is a PSDR_IQ client, which has no audio rows", id);
    case PSK_BAD_CARRIER: return fail(PSDR_ERR_INVALID, "PSK decoder: carrier_hz %g is not a finite number inside [%g, %g]", cfg->carrier_hz, PSK_CARRIER_MIN, PSK_CARRIER_MAX);
    case PSK_BAD_BAUD: return fail(PSDR_ERR_INVALID, "PSK decoder: baud %g is neither %g nor %g", cfg->baud, PSK_BAUD_31, PSK_BAUD_63);
    case PSK_BAD_SEARCH: return fail(PSDR_ERR_INVALID, "PSK decoder: search_hz %g is not a finite number inside [0, %g), half the baud rate", cfg->search_hz, cfg->baud / 2);
    case PSK_BAD_QUALITY: return fail(PSDR_ERR_INVALID, "PSK decoder: quality %g is not a finite number inside (0, 1)", cfg->quality);
    case PSK_BAD_RATE: return fail(PSDR_ERR_STATE, "PSK decoder: the context's audio_rate %d is outside [%d, %d]", c->cfg.audio_rate, PSK_RATE_MIN, PSK_RATE_MAX);
    case PSK_BAD_BAND: return fail(PSDR_ERR_STATE, "PSK decoder: the lanes from %g to %g Hz do not lie inside [%g Hz, %g of the audio_rate %d]", cfg->carrier_hz + psk_lane_hz(0, cfg->baud), cfg->carrier_hz + psk_lane_hz(PSK_LANES - 1, cfg->baud), PSK_BOTTOM, PSK_TOP, c->cfg.audio_rate);
    }
    if (cfg) PSDRCHK(first_psk_decoder(c));
    psk_apply(c->aslots[id], cfg, c->cfg.audio_rate);
    return PSDR_OK;
}
extern "C" int psdr_psk_defaults(double audio_rate, psdr_psk_config *out) {
    if (!out) return fail(PSDR_ERR_INVALID, "null argument");
    if (!psk_defaults(audio_rate, out)) return fail(PSDR_ERR_INVALID, "PSK decoder defaults: audio_rate %g outside [%d, %d]", audio_rate, PSK_RATE_MIN, PSK_RATE_MAX);
    return PSDR_OK;
}
extern "C" int psdr_client_set_fax_decoder(psdr_ctx *c, int id, const psdr_fax_config *cfg) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    switch (fax_check(c->aslots.data(), c->aslots.size(), id, cfg, c->cfg.audio_rate)) {
    case FAX_OK: break;
    case FAX_BAD_ID: return fail(PSDR_ERR_INVALID, "fax decoder: id %d outside 0..%d", id, (int)c->aslots.size() - 1);
    case FAX_INACTIVE: return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
    case FAX_IQ: return fail(PSDR_ERR_INVALID, "fax decoder: client %d is a PSDR_IQ client, which has no audio rows", id);
    case FAX_BAD_MODE: return fail(PSDR_ERR_INVALID, "fax decoder: mode %d is neither PSDR_FAX_AUTO nor PSDR_FAX_FREE", cfg->mode);
    case FAX_BAD_TONES: return fail(PSDR_ERR_INVALID, "fax decoder: black_hz %g and white_hz %g are not finite numbers inside [%g, %g] that lie %g to %g apart", cfg->black_hz, cfg->white_hz, FAX_TONE_MIN, FAX_TONE_MAX, FAX_SHIFT_MIN, FAX_SHIFT_MAX);
    case FAX_BAD_LPM: return fail(PSDR_ERR_INVALID, "fax decoder: lpm %g is none of 60, 90, 120 and 240", cfg->lpm);
    case FAX_BAD_WIDTH: return fail(PSDR_ERR_INVALID, "fax decoder: width %d outside [%d, %d]", cfg->width, FAX_WIDTH_MIN, FAX_WIDTH_MAX);
    case FAX_BAD_SLANT: return fail(PSDR_ERR_INVALID, "fax decoder: slant_ppm %g is not a finite number inside [%g, %g]", cfg->slant_ppm, -FAX_SLANT_MAX, FAX_SLANT_MAX);
    case FAX_BAD_PHASE_COL: return fail(PSDR_ERR_INVALID, "fax decoder: phase_col %d outside [0, width %d)", cfg->phase_col, cfg->width);
    case FAX_BAD_RATIO: return fail(PSDR_ERR_INVALID, "fax decoder: tone_ratio %g is not a finite number inside (0, 1)", cfg->tone_ratio);
    case FAX_BAD_START: return fail(PSDR_ERR_INVALID, "fax decoder: start_blocks %d outside [2, 64]", cfg->start_blocks);
    case FAX_BAD_PHASE_LINES: return fail(PSDR_ERR_INVALID, "fax decoder: phase_lines %d outside [2, 32]", cfg->phase_lines);
    case FAX_BAD_MAX_LINES: return fail(PSDR_ERR_INVALID, "fax decoder: max_lines %d is negative", cfg->max_lines);
    case FAX_BAD_RATE: return fail(PSDR_ERR_STATE, "fax decoder: the context's audio_rate %d is outside [%d, %d]", c->cfg.audio_rate, FAX_RATE_MIN, FAX_RATE_MAX);
    case FAX_BAD_BAND: return fail(PSDR_ERR_STATE, "fax decoder: the higher tone %g Hz plus %g does not lie under %g of the audio_rate %d", std::max(cfg->black_hz, cfg->white_hz), FAX_GUARD, FAX_TOP, c->cfg.audio_rate);
    case FAX_BAD_PIXEL: return fail(PSDR_ERR_STATE, "fax decoder: at lpm %g and audio_rate %d a pixel of width %d would not hold 1 to %d samples", cfg->lpm, c->cfg.audio_rate, cfg->width, FAX_PIXEL_MAX);
    }
    if (cfg) PSDRCHK(first_fax_decoder(c));
    fax_apply(c->aslots[id], cfg, c->cfg.audio_rate, psdr_ctx::FaxDecoder::max_samples(*c));
    return PSDR_OK;
}
extern "C" int psdr_fax_defaults(double audio_rate, psdr_fax_config *out) {
    if (!out) return fail(PSDR_ERR_INVALID, "null argument");
    if (!fax_defaults(audio_rate, out)) return fail(PSDR_ERR_INVALID, "fax decoder defaults: audio_rate %g outside [%d, %d]", audio_rate, FAX_RATE_MIN, FAX_RATE_MAX);
    return PSDR_OK;
}
extern "C" int psdr_client_set_agc_profile(psdr_ctx *c, int id, const psdr_agc_profile *p) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    const int rate = c->cfg.audio_rate;
    switch (agc_profile_check(c->aslots.data(), c->aslots.size(), id, p, rate)) {
    case AP_OK: break;
    case AP_BAD_ID: return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
    case AP_NONFINITE: return fail(PSDR_ERR_INVALID, "AGC profile: a field that is not a finite number");
    case AP_BAD_DESIRED: return fail(PSDR_ERR_INVALID, "AGC profile: desired %g outside (0, 1]", p->desired);
    case AP_BAD_TIME: return fail(PSDR_ERR_INVALID, "AGC profile: attack %g ms / release %g ms outside (0, %g]", p->attack_ms, p->release_ms, AGC_MS_MAX);
    case AP_BAD_CAP: return fail(PSDR_ERR_INVALID, "AGC profile: max_gain %g below 0", p->max_gain);
    case AP_BAD_MANUAL: return fail(PSDR_ERR_INVALID, "AGC profile: manual %d outside 0..1", (int)p->manual);
    case AP_BAD_MANUAL_GAIN: return fail(PSDR_ERR_INVALID, "AGC profile: manual_gain %g below 0", p->manual_gain);
    case AP_NO_RATE: return fail(PSDR_ERR_STATE, "AGC profile: the context's audio_rate %d is not positive", rate);
    case AP_ATTACK_SLOWER:
        return fail(PSDR_ERR_INVALID, "AGC profile: attack %g ms is slower than release %g ms (the gain step needs attack >= release)", p->attack_ms, p->release_ms);
    }
    if (p) PSDRCHK(first_use(c, c->agc_prof, "AGC profile table (%zu bytes): %s"));
    agc_profile_apply(c->aslots[id], p, rate);
    return PSDR_OK;
}
extern "C" int psdr_agc_preset(int kind, psdr_agc_profile *out) {
    if (!out) return fail(PSDR_ERR_INVALID, "null argument");
    if (!agc_preset(kind, out)) return fail(PSDR_ERR_INVALID, "AGC preset: unknown kind %d", kind);
    return PSDR_OK;
}
// (a debug entry, beside psdr_debug_notch_ptrs: exported for the tests, not part of include/psdr.h)  out[0]: the AGC profiles'
// table (null until the context's first profile), out[1]: PostArgs::agc_tab of the last chain batch
extern "C" int psdr_debug_agc_profile_ptrs(psdr_ctx *c, const void *out[2]) {
    if (!c || !out) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    out[0] = c->agc_prof.tab.d.get(), out[1] = c->post.agc_tab;
    return PSDR_OK;
}
// (a debug entry, beside psdr_debug_notch_ptrs: exported for the tests, not part of include/psdr.h)  out[0..1]: the audio filter's
// table and state (null until the context's first filter client)
extern "C" int psdr_debug_audio_filter_ptrs(psdr_ctx *c, const void *out[2]) {
    if (!c || !out) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    out[0] = c->af.tab.d.get(), out[1] = c->af.state.get();
    return PSDR_OK;
}
// (... and whether the last chain batch's moving averages read the audio rows themselves, k_pc_ma2 DIRECT: the form in which the
// chain reads what k_audio_filter has just written without a gathered copy between them)
extern "C" int psdr_debug_post_direct(psdr_ctx *c, int *direct) {
    if (!c || !direct) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    *direct = c->post_direct ? 1 : 0;
    return PSDR_OK;
}
extern "C" int psdr_audio_filter_design(int kind, double audio_rate, double f0, double q, psdr_biquad *out) {
    switch (audio_filter_design(kind, audio_rate, f0, q, out)) {
    case AD_OK: break;
    case AD_NULL: return fail(PSDR_ERR_INVALID, "null argument");
    case AD_BAD_KIND: return fail(PSDR_ERR_INVALID, "audio filter design: unknown kind %d", kind);
    case AD_BAD_RATE: return fail(PSDR_ERR_INVALID, "audio filter design: audio_rate %g", audio_rate);
    case AD_BAD_F0: return fail(PSDR_ERR_INVALID, "audio filter design: f0 %g outside (0, %g)", f0, audio_rate / 2);
    case AD_BAD_Q: return fail(PSDR_ERR_INVALID, "audio filter design: q %g", q);
    case AD_REFUSED: return fail(PSDR_ERR_INVALID, "audio filter design: kind %d at f0 %g, q %g, rate %g gives a section psdr_client_set_audio_filter refuses", kind, f0, q, audio_rate);
    }
    return PSDR_OK;
}
// out[0..2]: the detector's table, sums and counters (null until the context's first auto-notch client); out[3..4]:
// DemodArgs::notch_man / notch_auto of the last demodulation batch
extern "C" int psdr_debug_notch_ptrs(psdr_ctx *c, const void *out[5]) {
    if (!c || !out) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mtx);
    out[0] = c->notch.tab.get(), out[1] = c->notch.acc.get(), out[2] = c->notch.cnt.get();
    out[3] = c->dbg_notch_man, out[4] = c->dbg_notch_auto;
    return PSDR_OK;
}

// The one-kernel path (demod.h): a family of chain kernels is its two compile-time plans, 360 = 8*9*5 and 720 = 8*9*10
template <class... X>
struct ChainFamily {
    void (*k360)(DemodArgs, int, int, X...);
    void (*k720)(DemodArgs, int, int, X...);
};
static const ChainFamily<> CHAIN_FIXED{k_demod_chain_fixed<360, 8, 9, 5>, k_demod_chain_fixed<720, 8, 9, 10>};
static const ChainFamily<cf *> CHAIN_IQ{k_demod_chain_iq<360, 8, 9, 5>, k_demod_chain_iq<720, 8, 9, 10>};
static const ChainFamily<cf *> CHAIN_IQ_NZ{k_demod_chain_iq_nz<360, 8, 9, 5>, k_demod_chain_iq_nz<720, 8, 9, 10>};  // IQ lists with a notched client
static const ChainFamily<SamArgs> CHAIN_SAM{k_demod_chain_sam<360, 8, 9, 5>, k_demod_chain_sam<720, 8, 9, 10>};
static const ChainFamily<FtArgs> CHAIN_FT_SSB{k_demod_chain_ft<360, 8, 9, 5, true>, k_demod_chain_ft<720, 8, 9, 10, true>};
static const ChainFamily<FtArgs> CHAIN_FT_IQ{k_demod_chain_ft<360, 8, 9, 5, false>, k_demod_chain_ft<720, 8, 9, 10, false>};
static const ChainFamily<SbArgs> CHAIN_SBSAM{k_demod_chain_sbsam<360, 8, 9, 5>, k_demod_chain_sbsam<720, 8, 9, 10>};
// frames per chain for `cnt` clients: long chains repeat fewer transforms (1 or 2 per chain), short ones give few
// clients enough waves
// (256 clients x 256 frames, same box: K = 4 / 8 / 16 / 32 -> 5.81 / 5.77 / 5.93 / 6.04 us per frame, the
// two-kernel path 5.99)
// (round 4, 512-frame launches: with 256 clients and more, chains of 16 still leave 8192 waves and repeat half as
// many warm-up transforms: 93.4 -> 94.6 GS/s on the 256-client shape, same box, interleaved twice)
static int chain_k(const psdr_ctx *c, int cnt, int nframes) {
    if (c->demod_chain_k > 0) return c->demod_chain_k;
    int K = cnt >= 256 && (unsigned)cnt * (unsigned)((nframes + 15) / 16) >= 8192u ? 16 : 8;
    while (K > 4 && (unsigned)cnt * (unsigned)((nframes + K - 1) / K) < 1024u) K >>= 1;
    return K;
}
// One wave per chain of K consecutive frames (K = 0: chain_k's choice) of each of the `cnt` clients listed in aa.clients.
// W waves = items per work-group (W360 at n = 360, one at 720) share the twiddle table in LDS; each has a transform buffer
// and `wave_lds` bytes more - inside the 15 KiB an FFT pass leaves free on a CU.
template <class... X>
static hipError_t launch_chain(psdr_ctx *c, const ChainFamily<X...> &fam, DemodArgs aa, int cnt, int K, unsigned W360, size_t wave_lds, X... extra) {
    if (K <= 0) K = chain_k(c, cnt, aa.nframes);
    const unsigned W = c->idft_kind == IDFT_FIXED360 ? W360 : 1u;
    const unsigned items = (unsigned)cnt * (unsigned)((aa.nframes + K - 1) / K);
    const size_t lds = (size_t)(1 + W) * c->n * sizeof(cf) + W * wave_lds;
    void *args[] = {&aa, &cnt, &K, &extra...};
    return hipLaunchKernel((const void *)(c->idft_kind == IDFT_FIXED360 ? fam.k360 : fam.k720), dim3((items + W - 1) / W), dim3(64 * W), args, lds, c->side);
}
// The overlap-add behind the IDFT kernels: one wave per (client, group of PSDR_OLA_FG frames)
template <class... X>
static hipError_t launch_ola(psdr_ctx *c, void (*k)(DemodArgs, int, X...), DemodArgs aa, int cnt, X... extra) {
    const unsigned items = (unsigned)cnt * (unsigned)((aa.nframes + PSDR_OLA_FG - 1) / PSDR_OLA_FG);
    void *args[] = {&aa, &cnt, &extra...};
    return hipLaunchKernel((const void *)k, dim3((items + 3) / 4), dim3(256), args, 0, c->side);
}

// What every list's launches of a batch share: the spectrum and its layout, the transform's plan, the result rows and the carried
// state (each list sets `clients`, demod_impl the notch tables).
// band != nullptr: `spec` is a window of bins [band[0], band[0] + band[1]) per frame - linear, or (band_tiled) one
// band region of a banded spectrum (SpecLayout mode 4)
static DemodArgs demod_args(psdr_ctx *c, const cf *spec, size_t spec_stride, int nframes, uint64_t first_frame_num, const uint32_t *band,
                            bool band_tiled) {
    DemodArgs a{};
    a.spec = spec;
    a.spec_stride = spec_stride;
    a.is_real = c->is_real ? 1 : 0;
    a.lay = c->lay;
    if (band) {
        a.lay = SpecLayout{};
        a.lay.k0 = (int)band[0];
        if (band_tiled) {
            a.lay.mode = 4;
            a.lay.m1 = c->M1;
            a.lay.l2m1 = c->log2M1;
            a.lay.L = c->M2;
            a.lay.l2L = c->log2M2;
            a.lay.Lw = (int)(band[1] >> c->log2M1);
            a.lay.c2_0 = (int)(band[0] >> c->log2M1);
        }
    }
    a.n = c->n;
    a.nframes = nframes;
    a.max_batch = c->max_batch;
    a.first_frame_num = first_frame_num;
    a.Wn = c->d_Wn;
    a.nstages = c->nstages;
    for (int i = 0; i < c->nstages; i++) a.radix[i] = c->radix[i];
    a.stage_tab = c->d_stage_tab;
    a.ypost = c->d_ypost;
    a.pwr = c->d_pwr;
    a.gscratch = c->d_gscratch;
    a.lds_mode = c->lds_mode;
    a.audio = c->d_audio;
    a.nan_flags = c->d_nan;
    a.real_prev = c->d_real_prev;
    a.bb_tail = c->d_bb_tail;
    a.bb_last = c->d_bb_last;
    a.slots = (int)c->aslots.size();
    a.ssb_mark = c->d_ssb_mark;
    a.mark_epoch = (unsigned)(c->demod_seq % 0xFFFFFFFFull) + 1u;  // never 0
    a.replay = 0;
    return a;
}
// what a plan's byte offset names inside the ring slot's device copy
template <class T>
static const T *ring_at(const unsigned char *d_ring, size_t off) {
    return (const T *)(d_ring + off);
}

// One batch as it is fixed under mtx: demod_plan (demodplan.h) says who is demodulated, in which list of the ring slot and from
// which state; the squelch's, the audio filter's and the AGC profiles' plans say what follows the demodulation, and fill the ring
// slot's image of their tables.
struct BatchPlan {
    int ring = 0;
    unsigned char *h_ring = nullptr, *d_ring = nullptr;  // the ring slot's two copies
    DemodPlan p;
    NoisePlan nf;
    SquelchPlan sq;
    AfPlan af;
    NrPlan nr;
    AnbPlan anb;
    TonePlan tone;
    CwPlan cw;
    RttyPlan rtty;
    PskPlan psk;
    FaxPlan fax;
    AgcPlan ag;
    bool chain = false;  // the post chain follows: it is on, and somebody is in it
    // of the optional features: the rows of the result set this batch writes and the detector's table - null where the context has
    // none yet (they appear under mtx, once, and stay)
    cf *iq_rows = nullptr, *car_rows = nullptr;
    int *sq_rows = nullptr;
    float *nf_rows = nullptr;
    int4 *notch_tab = nullptr;
};
static int batch_plan(psdr_ctx *c, int nframes, const uint32_t *band, BatchPlan &b) {
    b.ring = c->client_ring.acquire();
    if (b.ring < 0) return fail(PSDR_ERR_HIP, "client parameter ring: event wait failed");
    b.h_ring = (unsigned char *)c->client_ring.host(b.ring), b.d_ring = (unsigned char *)c->client_ring.dev(b.ring);
    DemodFacts f;
    f.n = c->n, f.nframes = nframes;
    if (band) f.has_band = true, f.band_first = band[0], f.band_count = band[1];
    std::lock_guard<std::mutex> lk(c->mtx);  // (the band is checked under the same lock that fixes the windows of the batch)
    AudioSlot *slots = c->aslots.data();
    const size_t S = c->aslots.size();
    const int set = c->out_set ^ 1;
    b.iq_rows = c->iq.pool[set], b.car_rows = c->sam.pool[set], b.sq_rows = c->squelch.pool[set], b.nf_rows = c->noise.pool[set], b.notch_tab = c->notch.tab;
    f.post_on = c->post_on, f.have_notch_tab = b.notch_tab != nullptr;
    b.p = demod_plan(slots, S, c->demod_seq, f, b.h_ring);
    if (b.p.verdict == DP_BAND_OUTSIDE) {
        c->client_ring.unacquire();
        return fail(PSDR_ERR_INVALID, "client %d: window [%d, %d) outside the band [%u, %u)", b.p.bad_slot, b.p.bad_l, b.p.bad_r, band[0],
                    band[0] + band[1]);
    }
    b.chain = f.post_on && b.p.nact > 0;
    if (c->noise) b.nf = noise_plan(slots, S, c->demod_seq, c->noise.tab.host(b.ring));
    if (c->squelch) b.sq = squelch_plan(slots, S, c->demod_seq, b.chain, c->squelch.tab.host(b.ring));
    if (c->af) b.af = audio_filter_plan(slots, S, c->demod_seq, c->af.tab.host(b.ring));
    if (c->nr) b.nr = nr_plan(slots, S, c->demod_seq, c->nr.tab.host(b.ring), nr_a_up(c->cfg.audio_rate));
    if (c->anb) b.anb = anb_plan(slots, S, c->demod_seq, c->anb.tab.host(b.ring));
    if (c->tone) b.tone = tone_plan(slots, S, c->demod_seq, b.chain, c->tone.tab.host(b.ring));
    if (c->cw) b.cw = cw_plan(slots, S, c->demod_seq, c->cw.tab.host(b.ring));
    if (c->rtty) b.rtty = rtty_plan(slots, S, c->demod_seq, c->rtty.tab.host(b.ring));
    if (c->psk) b.psk = psk_plan(slots, S, c->demod_seq, c->psk.tab.host(b.ring));
    if (c->fax) b.fax = fax_plan(slots, S, c->demod_seq, c->fax.tab.host(b.ring));
    if (c->agc_prof && b.chain) b.ag = agc_profile_plan(slots, S, c->demod_seq, c->agc_prof.tab.host(b.ring));
    return PSDR_OK;
}
// What `side` holds in front of the batch's first kernel: the states that start from zero, the flip to the other result set, the
// ring slot and the tables.
static int batch_begin(psdr_ctx *c, const BatchPlan &b) {
    const DemodPlan &p = b.p;
    // the gates that start from (closed, 0): squelch_plan has taken sq_fresh off these slots, so the zeroing is enqueued before
    // anything below can fail the batch (`side` orders it behind the last batch's k_squelch and in front of this one's)
    for (size_t slot : b.sq.zero) HIPCHK(hipMemsetAsync(c->squelch.state + slot, 0, sizeof(SquelchState), c->side));
    // ... and the audio filters that start from zero, by the same rule (audio_filter_plan has taken af_fresh off these slots)
    for (size_t slot : b.af.zero)
        HIPCHK(hipMemsetAsync(c->af.state + slot * 2 * PSDR_AUDIO_FILTER_SECTIONS, 0, 2 * PSDR_AUDIO_FILTER_SECTIONS * sizeof(float), c->side));
    // ... and the noise reductions that start from zero (nr_plan has taken nr_fresh off these slots)
    for (size_t slot : b.nr.zero) HIPCHK(hipMemsetAsync(c->nr.state + slot, 0, sizeof(NrState), c->side));
    // ... and the audio blankers (anb_plan has taken anb_fresh off these slots)
    for (size_t slot : b.anb.zero) HIPCHK(hipMemsetAsync(c->anb.state + slot, 0, sizeof(AnbState), c->side));
    // ... and the tone decoders: state and history ring (tone_plan has taken tone_fresh off these slots)
    for (size_t slot : b.tone.zero) {
        HIPCHK(hipMemsetAsync(c->tone.state + slot, 0, sizeof(ToneState), c->side));
        HIPCHK(hipMemsetAsync(c->tone.hist + slot * (size_t)c->tone.ring * TONE_LANES, 0, (size_t)c->tone.ring * TONE_LANES * sizeof(ToneC), c->side));
    }
    // ... and the CW decoders: state and text ring (cw_plan has taken cw_fresh off these slots)
    for (size_t slot : b.cw.zero) {
        HIPCHK(hipMemsetAsync(c->cw.state + slot, 0, sizeof(CwState), c->side));
        HIPCHK(hipMemsetAsync(c->cw.text + slot * (size_t)CW_TEXT, 0, CW_TEXT, c->side));
    }
    // ... and the RTTY decoders: state and text ring (rtty_plan has taken rtty_fresh off these slots)
    for (size_t slot : b.rtty.zero) {
        HIPCHK(hipMemsetAsync(c->rtty.state + slot, 0, sizeof(RttyState), c->side));
        HIPCHK(hipMemsetAsync(c->rtty.text + slot * (size_t)RTTY_TEXT, 0, RTTY_TEXT, c->side));
    }
    // ... and the PSK decoders: state and text ring (psk_plan has taken psk_fresh off these slots)
    for (size_t slot : b.psk.zero) {
        HIPCHK(hipMemsetAsync(c->psk.state + slot, 0, sizeof(PskState), c->side));
        HIPCHK(hipMemsetAsync(c->psk.text + slot * (size_t)PSK_TEXT, 0, PSK_TEXT, c->side));
    }
    // ... and the fax decoders: the state (the ring's lines are counted from it: fax_plan has taken fax_fresh off these slots)
    for (size_t slot : b.fax.zero) HIPCHK(hipMemsetAsync(c->fax.state + slot, 0, sizeof(FaxState), c->side));
    // ... and the noise floors that start from zero: sums and record (noise_plan has taken nf_fresh off these slots)
    for (size_t slot : b.nf.zero) {
        HIPCHK(hipMemsetAsync(c->noise.acc + slot * (size_t)c->n, 0, (size_t)c->n * sizeof(float), c->side));
        HIPCHK(hipMemsetAsync(c->noise.state + slot, 0, sizeof(NoiseState), c->side));
    }
    // this batch's results go to the OTHER set (the copies of the last batch to the host may still be reading theirs); what
    // read this set two batches ago must have landed
    c->out_set ^= 1;
    c->d_audio = c->audio_pool[c->out_set], c->d_pwr = c->pwr_pool[c->out_set], c->d_nan = c->nan_pool[c->out_set];
    c->d_iq = b.iq_rows, c->d_car = b.car_rows, c->d_sq = b.sq_rows, c->d_nf = b.nf_rows;
    PSDRCHK(fetch_guard_wait(c, c->side, c->guard_audio[c->out_set]));
    c->guard_audio[c->out_set] = nullptr;
    // ... and the post chain's moving averages of that batch, which read its audio rows themselves (postchain.h k_pc_ma2
    // DIRECT) on a stream of their own, up to two steps behind the passes (psdr_set_post_chain drains: the chain has
    // been on for every batch since chain_seq started to count)
    if (c->post_on && c->post_direct && c->chain_seq >= 2 && c->pc_s[0] && c->side != c->stream)
        HIPCHK(hipStreamWaitEvent(c->side, c->pc.ev[1][(c->chain_seq - 2) % psdr_ctx::PC_SETS], 0));
    for (int i = 0; i < p.ncopies; i++)
        HIPCHK(hipMemcpyAsync(b.d_ring + p.copies[i].off, b.h_ring + p.copies[i].off, p.copies[i].bytes, hipMemcpyHostToDevice, c->side));
    // what starts from zero (car_zero names the slots of both kinds of SAM client: they share the carrier tail)
    if (p.ntssb > 0 && !c->ft) return fail(PSDR_ERR_STATE, "tuned USB / LSB clients without their tails");
    if (p.nsb > 0 && (!c->sb || !c->sam)) return fail(PSDR_ERR_STATE, "sideband SAM clients without their tails");
    const size_t tail_bytes = ((size_t)c->n / 2) * sizeof(cf);
    for (size_t slot : p.det_zero) PSDRCHK(notch_zero(c, slot));
    for (size_t off : p.car_zero) HIPCHK(hipMemsetAsync(c->sam.car_tail + off, 0, tail_bytes, c->side));
    for (size_t off : p.ft_zero) HIPCHK(hipMemsetAsync(c->ft.tail + off, 0, tail_bytes, c->side));
    for (size_t off : p.sb_zero) HIPCHK(hipMemsetAsync(c->sb.tail + off, 0, tail_bytes, c->side));
    if (b.sq.any()) HIPCHK(c->squelch.tab.upload(b.ring, (size_t)(b.sq.nsq + b.sq.ncopy), c->side));
    if (b.nf.any()) HIPCHK(c->noise.tab.upload(b.ring, (size_t)b.nf.n, c->side));
    if (b.af.any()) HIPCHK(c->af.tab.upload(b.ring, (size_t)b.af.n, c->side));
    if (b.nr.any()) HIPCHK(c->nr.tab.upload(b.ring, (size_t)b.nr.n, c->side));
    if (b.anb.any()) HIPCHK(c->anb.tab.upload(b.ring, (size_t)b.anb.n, c->side));
    if (b.tone.any()) HIPCHK(c->tone.tab.upload(b.ring, (size_t)(b.tone.n + b.tone.ncopy), c->side));
    if (b.cw.any()) HIPCHK(c->cw.tab.upload(b.ring, (size_t)b.cw.n, c->side));
    if (b.rtty.any()) HIPCHK(c->rtty.tab.upload(b.ring, (size_t)b.rtty.n, c->side));
    if (b.psk.any()) HIPCHK(c->psk.tab.upload(b.ring, (size_t)b.psk.n, c->side));
    if (b.fax.any()) HIPCHK(c->fax.tab.upload(b.ring, (size_t)b.fax.n, c->side));
    return PSDR_OK;
}

static bool fixed_plan(const psdr_ctx *c) { return c->idft_kind == IDFT_FIXED360 || c->idft_kind == IDFT_FIXED720; }
// the transform alone, into ypost, of the `cnt` clients listed in aa.clients (every path but the chain kernels')
static int launch_idft(psdr_ctx *c, const DemodArgs &aa, int cnt) {
    const unsigned items = (unsigned)cnt * (unsigned)aa.nframes;
    switch (c->idft_kind) {
    case IDFT_FIXED360:
    case IDFT_FIXED720: {
        // compile-time plans (demod.h): 360 = 8*9*5, 720 = 8*9*10; W items per work-group in
        // the 15 KiB of LDS an FFT pass leaves free on a CU
        const unsigned W = c->idft_kind == IDFT_FIXED360 ? 4u : 1u;
        const size_t lds = (size_t)(1 + W) * c->n * sizeof(cf);
        if (c->idft_kind == IDFT_FIXED360)
            hipLaunchKernelGGL((k_demod_idft_fixed<360, 8, 9, 5>), dim3((items + W - 1) / W), dim3(64 * W), lds,
                               c->side, aa, cnt);
        else
            hipLaunchKernelGGL((k_demod_idft_fixed<720, 8, 9, 10>), dim3((items + W - 1) / W), dim3(64 * W), lds,
                               c->side, aa, cnt);
        break;
    }
    case IDFT_WAVE: {
        // one wave per (client, frame), no work-group barriers (demod.h)
        const size_t lds = (size_t)(2 * PSDR_IDFT_WAVES + 1) * c->n * sizeof(cf);
        hipLaunchKernelGGL(k_demod_idft_wave, dim3((items + PSDR_IDFT_WAVES - 1) / PSDR_IDFT_WAVES),
                           dim3(64 * PSDR_IDFT_WAVES), lds, c->side, aa, cnt);
        break;
    }
    default:
        if (c->idft_lds > 64 * 1024 && c->lds_attr_done.insert((const void *)k_demod_idft).second)
            HIPCHK(hipFuncSetAttribute((const void *)k_demod_idft, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->idft_lds));
        hipLaunchKernelGGL(k_demod_idft, dim3(cnt, aa.nframes), dim3(c->idft_threads), c->idft_lds, c->side,
                           aa);
    }
    return PSDR_OK;
}
// the plain list (USB, LSB, AM, FM): the `nold` clients listed in a.clients
static int launch_plain(psdr_ctx *c, const DemodArgs &a, int nold, bool can_be_nonfinite) {
    bool ola_done = false;
    {
        ProfScope ps(c, K_IDFT, c->side);
        if (fixed_plan(c) && c->demod_chain) {
            // transform + overlap-add + demodulation in one kernel, one wave per chain of K consecutive frames of a
            // client (demod.h)
            HIPCHK(launch_chain(c, CHAIN_FIXED, a, nold, 0, 4u, 0));
            if (can_be_nonfinite) {
                DemodArgs ar = a;
                ar.replay = 1;
                HIPCHK(launch_chain(c, CHAIN_FIXED, ar, nold, a.nframes, 4u, 0));  // one chain = the whole batch
            }
            ola_done = true;
        } else {
            PSDRCHK(launch_idft(c, a, nold));
        }
        HIPCHK(hipGetLastError());
    }
    if (!ola_done) {
        ProfScope ps(c, K_OLA, c->side);
        HIPCHK(launch_ola(c, k_demod_ola, a, nold));
        if (can_be_nonfinite) hipLaunchKernelGGL(k_demod_ola_seq, dim3(((unsigned)nold + 3) / 4), dim3(256), 0, c->side, a, nold);
        HIPCHK(hipGetLastError());
    }
    return PSDR_OK;
}
// a list with launches of its own (PSDR_SAM, PSDR_IQ, ...): its chain kernel, or the transform and its overlap-add kernel
template <class Fam, class Ola, class Extra>
static int serve(psdr_ctx *c, const Fam &fam, Ola ola, const DemodArgs &aa, int cnt, unsigned W360, size_t wave_lds, Extra extra) {
    if (fixed_plan(c) && c->demod_chain) {
        ProfScope ps(c, K_IDFT, c->side);
        HIPCHK(launch_chain(c, fam, aa, cnt, 0, W360, wave_lds, extra));
        return PSDR_OK;
    }
    {
        ProfScope ps(c, K_IDFT, c->side);
        PSDRCHK(launch_idft(c, aa, cnt));
        HIPCHK(hipGetLastError());
    }
    ProfScope ps(c, K_OLA, c->side);
    HIPCHK(launch_ola(c, ola, aa, cnt, extra));
    return PSDR_OK;
}
// The batch's lists in their order on `side`: plain, SAM, IQ, tuned SSB, tuned IQ, sideband SAM.  a: the batch's arguments with
// the plain list's clients
static int launch_lists(psdr_ctx *c, const BatchPlan &b, const DemodArgs &a, bool can_be_nonfinite) {
    const DemodPlan &p = b.p;
    // a list with launches of its own: the batch's arguments with its clients
    auto of_list = [&](const RingList &l) {
        DemodArgs al = a;
        al.clients = ring_at<ClientParams>(b.d_ring, l.clients);
        return al;
    };
    if (p.nold > 0) PSDRCHK(launch_plain(c, a, p.nold, can_be_nonfinite));
    const size_t tail_bytes = ((size_t)c->n / 2) * sizeof(cf);
    SamArgs sa{};
    if (p.nsam + p.nsb > 0) {
        sa.car_tail = c->sam.car_tail;
        sa.car_rec = c->d_car;
        sa.cutoff = (int)((int64_t)500 * c->n / c->cfg.audio_rate);  // src/signal.cpp:217-220
        sa.hz_per_rad = (float)((double)c->cfg.audio_rate / (2.0 * M_PI));
    }
    // the PSDR_SAM clients: the tail of the active list, launches of their own behind the others' (demod.h)
    // (a wave's carrier tail lives in n/2 words of LDS behind the transform buffers: two waves per work-group at
    // n = 360, 11.25 KiB, and one at 720, 14.1 KiB - inside the 15 KiB an FFT pass leaves free on a CU)
    if (p.nsam > 0) PSDRCHK(serve(c, CHAIN_SAM, k_demod_ola_sam, of_list(p.sam), p.nsam, 2u, tail_bytes, sa));
    // the PSDR_IQ clients: launches of their own behind the others', on the same stream (demod.h)
    if (p.niq > 0) PSDRCHK(serve(c, p.iq_notched ? CHAIN_IQ_NZ : CHAIN_IQ, k_demod_ola_iq, of_list(p.iq), p.niq, 4u, 0, c->d_iq));
    // the tuned clients: their own list, launches of their own behind the others' (demod.h)
    FtArgs fa{};
    fa.tail = c->ft.tail;
    fa.iq = c->d_iq;
    if (p.ntssb > 0) {
        fa.ft = ring_at<FtClient>(b.d_ring, p.tssb.side);
        PSDRCHK(serve(c, CHAIN_FT_SSB, k_demod_ola_ft<true>, of_list(p.tssb), p.ntssb, 4u, 0, fa));
    }
    if (p.ntiq > 0) {
        fa.ft = ring_at<FtClient>(b.d_ring, p.tiq.side);
        PSDRCHK(serve(c, CHAIN_FT_IQ, k_demod_ola_ft<false>, of_list(p.tiq), p.ntiq, 4u, 0, fa));
    }
    if (p.nsb > 0) {
        // the sideband SAM clients: their own list, launches of their own behind all the others' (demod.h); LDS as SAM's
        SbArgs sba{};
        sba.sa = sa;
        sba.sb = ring_at<SbClient>(b.d_ring, p.sb.side);
        sba.tail = c->sb.tail;
        PSDRCHK(serve(c, CHAIN_SBSAM, k_demod_ola_sbsam, of_list(p.sb), p.nsb, 2u, tail_bytes, sba));
    }
    return PSDR_OK;
}
// Behind the batch's last demodulation kernel - the auto-notch detector: it writes the table those have just read (demod.h)
static int launch_detector(psdr_ctx *c, const BatchPlan &b, const DemodArgs &a) {
    NotchArgs na{};
    na.det = ring_at<ClientParams>(b.d_ring, b.p.det.clients);
    na.acc = c->notch.acc;
    na.cnt = c->notch.cnt;
    na.tab = b.notch_tab;
    na.period = std::max(1, c->cfg.audio_rate / c->n);
    hipLaunchKernelGGL(k_notch_detect, dim3((unsigned)b.p.ndet), dim3(64), 0, c->side, a, b.p.ndet, na);
    HIPCHK(hipGetLastError());
    return PSDR_OK;
}
// ... the noise floor: it reads the batch's raw spectrum and writes the frames' noise power, which the squelch behind it reads
static int launch_noise_floor(psdr_ctx *c, const BatchPlan &b, const DemodArgs &a) {
    NoiseArgs na{};
    na.list = c->noise.tab.dev(b.ring), na.nlist = b.nf.n;
    na.acc = c->noise.acc, na.state = c->noise.state;
    na.W = c->d_nf;
    na.period = noise_period(c->cfg.audio_rate, c->n);
    hipLaunchKernelGGL(k_noise_floor, dim3((unsigned)na.nlist), dim3(64), 0, c->side, a, na);
    HIPCHK(hipGetLastError());
    return PSDR_OK;
}
// ... the squelch, in front of the chain: it reads pwr and the NaN flags.  *chain_drop: what stays out of the chain's streams
static int launch_squelch(psdr_ctx *c, const BatchPlan &b, int nframes, const int **chain_drop) {
    SquelchArgs qa{};
    qa.list = c->squelch.tab.dev(b.ring), qa.nlist = b.sq.nsq + b.sq.ncopy;
    qa.pwr = c->d_pwr, qa.nan_flags = c->d_nan;
    qa.open = c->d_sq, qa.drop = b.chain ? c->squelch.drop.get() : nullptr;
    qa.state = c->squelch.state;
    qa.noise = b.sq.any_ref ? c->d_nf : nullptr;
    qa.nframes = nframes, qa.max_batch = c->max_batch;
    ProfScope ps(c, K_SQUELCH, c->side);
    hipLaunchKernelGGL(k_squelch, dim3((unsigned)qa.nlist), dim3(64), 0, c->side, qa);
    HIPCHK(hipGetLastError());
    if (b.chain) *chain_drop = c->squelch.drop;  // ... the NaN guard's frames and the closed ones
    return PSDR_OK;
}
// ... the tone decoder, behind the squelch and in front of everything that rewrites rows: it reads the listed clients' rows as the
// demodulator left them and writes the frames' records.  *chain_drop: with gated clients in a chain batch the chain reads the
// decoder's drop flags - what it would have read, and the closed frames
static int launch_tone_decoder(psdr_ctx *c, const BatchPlan &b, int nframes, const int **chain_drop) {
    ToneArgs ta{};
    ta.list = c->tone.tab.dev(b.ring), ta.nlist = b.tone.n + b.tone.ncopy;
    ta.tab = c->tone.plan;
    ta.audio = c->d_audio, ta.nan_flags = c->d_nan;
    ta.state = c->tone.state, ta.hist = c->tone.hist, ta.rec = c->tone.rec;
    ta.prev_drop = *chain_drop, ta.drop = b.tone.gated ? c->tone.drop.get() : nullptr;
    ta.nframes = nframes, ta.max_batch = c->max_batch, ta.h = c->n / 2, ta.ring = c->tone.ring;
    ProfScope ps(c, K_AUDIO_TONE, c->side);
    HIPCHK(audio_tone_launch(ta, c->side));
    if (b.tone.gated) *chain_drop = c->tone.drop;
    return PSDR_OK;
}
// ... the CW decoder, at the tone decoder's reading point: it reads the listed clients' rows as the demodulator left them and
// writes the frames' records and the clients' text
static int launch_cw_decoder(psdr_ctx *c, const BatchPlan &b, int nframes) {
    CwArgs ca{};
    ca.list = c->cw.tab.dev(b.ring), ca.nlist = b.cw.n;
    ca.tab = c->cw.plan;
    ca.audio = c->d_audio, ca.nan_flags = c->d_nan;
    ca.state = c->cw.state, ca.text = c->cw.text, ca.rec = c->cw.rec;
    ca.nframes = nframes, ca.max_batch = c->max_batch, ca.h = c->n / 2;
    ProfScope ps(c, K_AUDIO_CW, c->side);
    HIPCHK(audio_cw_launch(ca, c->side));
    return PSDR_OK;
}
// ... the RTTY decoder, at the same reading point: it reads the listed clients' rows as the demodulator left them and writes the
// frames' records and the clients' text
static int launch_rtty_decoder(psdr_ctx *c, const BatchPlan &b, int nframes) {
    RttyArgs ra{};
    ra.list = c->rtty.tab.dev(b.ring), ra.nlist = b.rtty.n;
    ra.tab = c->rtty.plan;
    ra.audio = c->d_audio, ra.nan_flags = c->d_nan;
    ra.state = c->rtty.state, ra.text = c->rtty.text, ra.rec = c->rtty.rec;
    ra.nframes = nframes, ra.max_batch = c->max_batch, ra.h = c->n / 2;
    ProfScope ps(c, K_AUDIO_RTTY, c->side);
    HIPCHK(audio_rtty_launch(ra, c->side));
    return PSDR_OK;
}
// ... the PSK31 decoder, at the same reading point: it reads the listed clients' rows as the demodulator left them and writes the
// frames' records and the clients' text
static int launch_psk_decoder(psdr_ctx *c, const BatchPlan &b, int nframes) {
    PskArgs pa{};
    pa.list = c->psk.tab.dev(b.ring), pa.nlist = b.psk.n;
    pa.tab = c->psk.plan;
    pa.audio = c->d_audio, pa.nan_flags = c->d_nan;
    pa.state = c->psk.state, pa.text = c->psk.text, pa.rec = c->psk.rec;
    pa.nframes = nframes, pa.max_batch = c->max_batch, pa.h = c->n / 2;
    ProfScope ps(c, K_AUDIO_PSK, c->side);
    HIPCHK(audio_psk_launch(pa, c->side));
    return PSDR_OK;
}
// ... the radiofax decoder, at the same reading point: it reads the listed clients' rows as the demodulator left them and writes the
// frames' records and the clients' kept lines
static int launch_fax_decoder(psdr_ctx *c, const BatchPlan &b, int nframes) {
    FaxArgs fa{};
    fa.list = c->fax.tab.dev(b.ring), fa.nlist = b.fax.n;
    fa.tab = c->fax.plan;
    fa.audio = c->d_audio, fa.nan_flags = c->d_nan;
    fa.state = c->fax.state, fa.ring = c->fax.ring, fa.meta = c->fax.meta, fa.rec = c->fax.rec;
    fa.nframes = nframes, fa.max_batch = c->max_batch, fa.h = c->n / 2, fa.rmax = c->fax.rmax;
    ProfScope ps(c, K_AUDIO_FAX, c->side);
    HIPCHK(audio_fax_launch(fa, c->side));
    return PSDR_OK;
}
// ... the audio blanker, in front of the noise reduction, the audio filter and the chain: it works on the listed clients' rows in
// place
static int launch_audio_blanker(psdr_ctx *c, const BatchPlan &b, int nframes) {
    AnbArgs ba{};
    ba.list = c->anb.tab.dev(b.ring), ba.nlist = b.anb.n;
    ba.audio = c->d_audio, ba.nan_flags = c->d_nan;
    ba.state = c->anb.state;
    ba.nframes = nframes, ba.max_batch = c->max_batch, ba.h = c->n / 2;
    ProfScope ps(c, K_AUDIO_NB, c->side);
    HIPCHK(audio_nb_launch(ba, c->side));
    return PSDR_OK;
}
// ... the noise reduction, in front of the audio filter and the chain: it works on the listed clients' rows in place
static int launch_noise_reduction(psdr_ctx *c, const BatchPlan &b, int nframes) {
    NrArgs na{};
    na.list = c->nr.tab.dev(b.ring), na.nlist = b.nr.n;
    na.tab = c->nr.plan;
    na.audio = c->d_audio, na.nan_flags = c->d_nan;
    na.state = c->nr.state;
    na.nframes = nframes, na.max_batch = c->max_batch, na.h = c->n / 2;
    ProfScope ps(c, K_AUDIO_NR, c->side);
    HIPCHK(audio_nr_launch(na, c->side));
    return PSDR_OK;
}
// ... the audio filter, in front of the chain: it filters the listed clients' rows in place (k_squelch reads pwr and flags, not
// rows: their order does not matter)
static int launch_audio_filter(psdr_ctx *c, const BatchPlan &b, int nframes) {
    AudioFilterArgs fa{};
    fa.list = c->af.tab.dev(b.ring), fa.nlist = b.af.n;
    fa.audio = c->d_audio, fa.nan_flags = c->d_nan;
    fa.state = c->af.state;
    fa.nframes = nframes, fa.max_batch = c->max_batch, fa.h = c->n / 2;
    ProfScope ps(c, K_AUDIO_FILTER, c->side);
    HIPCHK(audio_filter_launch(fa, c->side));
    return PSDR_OK;
}
// The batch's end: the post chain, if it follows, and the ring slot's release behind its last reader
static int batch_end(psdr_ctx *c, const BatchPlan &b, const ClientParams *d_clients, int nframes, const int *chain_drop) {
    hipStream_t last_user = c->side;
    if (b.chain) {
        // the AGC profiles of the batch's snapshot, in front of the chain (whose stages all start behind `side`)
        if (b.ag.any) HIPCHK(c->agc_prof.tab.upload(b.ring, c->aslots.size(), c->side));
        PSDRCHK(post_chain_enqueue(c, d_clients, ring_at<int>(b.d_ring, b.p.slot_ci), b.p.nact, b.p.npaused, nframes, chain_drop,
                                   b.ag.any ? c->agc_prof.tab.dev(b.ring) : nullptr, &last_user));
    }
    HIPCHK(c->client_ring.release(b.ring, last_user));
    return side_done(c);
}

// One batch: plans it, then copies, zeroes and launches what the plans name.
static int demod_impl(psdr_ctx *c, const cf *spec, size_t spec_stride, int nframes, uint64_t first_frame_num,
                      const uint32_t *band = nullptr, bool band_tiled = false) {
    if (c->n <= 0) return fail(PSDR_ERR_STATE, "context created with audio_fft_size 0");
    HIPCHK(hipSetDevice(c->device));
    BatchPlan b;
    PSDRCHK(batch_plan(c, nframes, band, b));
    c->last_demod_frames = nframes;
    if (b.p.idle()) return PSDR_OK;
    PSDRCHK(batch_begin(c, b));
    DemodArgs a = demod_args(c, spec, spec_stride, nframes, first_frame_num, band, band_tiled);
    a.clients = ring_at<ClientParams>(b.d_ring, b.p.plain.clients);
    a.notch_man = b.p.any_manual ? ring_at<int4>(b.d_ring, b.p.notch) : nullptr;
    a.notch_auto = b.notch_tab;
    c->dbg_notch_man = a.notch_man, c->dbg_notch_auto = a.notch_auto;
    // the frame-ordered second walk of marked USB / LSB slots (demod.h: DemodArgs::ssb_mark) can only find work where
    // non-finite values can arise: float input formats, or a spectrum that comes from the caller
    PSDRCHK(launch_lists(c, b, a, c->cfg.input_format >= PSDR_FMT_F32 || spec != c->d_spec));
    if (b.p.ndet > 0) PSDRCHK(launch_detector(c, b, a));
    const int *chain_drop = c->d_nan;  // what stays out of the chain's streams: the NaN guard's frames ...
    if (b.nf.any()) PSDRCHK(launch_noise_floor(c, b, a));
    if (b.sq.any()) PSDRCHK(launch_squelch(c, b, nframes, &chain_drop));
    if (b.tone.any()) PSDRCHK(launch_tone_decoder(c, b, nframes, &chain_drop));
    if (b.cw.any()) PSDRCHK(launch_cw_decoder(c, b, nframes));
    if (b.rtty.any()) PSDRCHK(launch_rtty_decoder(c, b, nframes));
    if (b.psk.any()) PSDRCHK(launch_psk_decoder(c, b, nframes));
    if (b.fax.any()) PSDRCHK(launch_fax_decoder(c, b, nframes));
    if (b.anb.any()) PSDRCHK(launch_audio_blanker(c, b, nframes));
    if (b.nr.any()) PSDRCHK(launch_noise_reduction(c, b, nframes));
    if (b.af.any()) PSDRCHK(launch_audio_filter(c, b, nframes));
    return batch_end(c, b, a.clients, nframes, chain_drop);
}

static int check_nframes(const psdr_ctx *c, int nframes) {
    if (nframes < 1 || nframes > c->max_batch)
        return fail(PSDR_ERR_INVALID, "nframes %d outside [1, max_batch=%d]", nframes, c->max_batch);
    return PSDR_OK;
}
extern "C" int psdr_demod_batch(psdr_ctx *c, uint64_t first_frame_num) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (c->last_nframes < 1) return fail(PSDR_ERR_STATE, "demod_batch before process_batch/execute");
    return demod_impl(c, c->d_spec, c->spec_stride, c->last_nframes, first_frame_num);
}
extern "C" int psdr_demod_batch_from(psdr_ctx *c, const float *d_spec, size_t frame_stride_bins,
                                     int nframes, uint64_t first_frame_num) {
    if (!c || !d_spec) return fail(PSDR_ERR_INVALID, "null argument");
    PSDRCHK(check_nframes(c, nframes));
    if (frame_stride_bins < (c->is_real ? c->N / 2 + 1 : c->N))
        return fail(PSDR_ERR_INVALID, "frame stride smaller than one spectrum");
    return demod_impl(c, (const cf *)d_spec, frame_stride_bins, nframes, first_frame_num);
}
extern "C" int psdr_demod_batch_from_band(psdr_ctx *c, const float *d_band, size_t frame_stride_bins, uint32_t first_bin,
                                          uint32_t nbins, int nframes, uint64_t first_frame_num) {
    if (!c || !d_band) return fail(PSDR_ERR_INVALID, "null argument");
    PSDRCHK(check_nframes(c, nframes));
    if (nbins < 1 || frame_stride_bins < nbins) return fail(PSDR_ERR_INVALID, "frame stride smaller than the band");
    const uint32_t band[2] = {first_bin, nbins};
    return demod_impl(c, (const cf *)d_band, frame_stride_bins, nframes, first_frame_num, band);
}
extern "C" int psdr_demod_batch_from_band_region(psdr_ctx *c, const float *d_region, size_t frame_stride_bins, uint32_t first_bin,
                                                 uint32_t nbins, int nframes, uint64_t first_frame_num) {
    if (!c || !d_region) return fail(PSDR_ERR_INVALID, "null argument");
    if (c->is_real || c->M2 != 1024) return fail(PSDR_ERR_UNSUPPORTED, "band regions: IQ frames with 1024-point rows only");
    PSDRCHK(check_nframes(c, nframes));
    const uint32_t m1 = (uint32_t)c->M1;
    if (nbins < m1 || (nbins & (m1 - 1)) || (first_bin & (m1 - 1)) || first_bin >= (uint32_t)c->M)
        return fail(PSDR_ERR_INVALID, "band region [%u, +%u): whole columns of %u bins", first_bin, nbins, m1);
    if (frame_stride_bins < nbins) return fail(PSDR_ERR_INVALID, "frame stride smaller than the band");
    const uint32_t band[2] = {first_bin, nbins};
    return demod_impl(c, (const cf *)d_region, frame_stride_bins, nframes, first_frame_num, band, true);
}

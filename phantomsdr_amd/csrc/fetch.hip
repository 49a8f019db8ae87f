// fetch.hip - the served end of the path: the results of the last demodulation batch (and of the last waterfall batch) to
// host memory.  (src/websocket.cpp:156-185 makes one pass over signal_slices per frame and every send_audio ends in host
// memory: src/signal.cpp:283-291 -> src/audio.cpp:26-44; send_waterfall: src/waterfall.cpp:44-51.  Per-client
// psdr_read_audio pays a synchronisation and three copies per client and frame.)
// psdr_fetch_begin ENQUEUES the copies of the batch into one of a ring of PSDR_FETCH_SETS pinned host sets on a copy
// stream, behind the kernels that produce them, and returns; psdr_fetch_end waits for the oldest fetch in flight and makes
// its set the one psdr_fetched_* read.  Between the two the caller enqueues the NEXT batch: the copies run beside its FFT
// passes.  The device-side result buffers exist once: the next batch's demodulation, waterfall gather and PCM output wait
// (in stream order, no host wait) for the newest fetch's copies.  What a fetch copies, in which order and form, the ring's
// arithmetic and whose rows a slot of a set holds are decided in fetchplan.h; here: checks, snapshot, allocations, HIP calls.
#include "ctx.h"

int psdr::fetch_guard_wait(psdr_ctx *c, hipStream_t st, hipEvent_t ev) {
    (void)c;
    if (ev) HIPCHK(hipStreamWaitEvent(st, ev, 0));
    return PSDR_OK;
}

using FetchSet = psdr_ctx::FetchSet;
enum RowKind { ROWS_ANY, ROWS_AUDIO, ROWS_IQ };  // what a call asks a slot for: a batch demodulated as PSDR_IQ holds complex
                                                 // rows and no audio / PCM, any other batch no IQ rows

// ---- psdr_fetch_begin / _end / _batch ----------------------------------------------------------------------------------
// the fetch has landed (its events have completed on the host): nothing left for a writer to wait for
static int retire(psdr_ctx *c, FetchSet &fs) {
    HIPCHK(hipEventSynchronize(fs.done));
    if (fs.has_pcm) HIPCHK(hipEventSynchronize(fs.ev_pcm));
    fs.inflight = false;
    c->fetch_inflight--;
    if (c->guard_wf == fs.ev_wf) c->guard_wf = nullptr;
    for (int i = 0; i < 2; i++) {
        if (c->guard_audio[i] == fs.ev_audio) c->guard_audio[i] = nullptr;
        if (c->guard_pcm[i] == fs.ev_pcm) c->guard_pcm[i] = nullptr;
    }
    return PSDR_OK;
}
// grow-only: the old rows are given up only once the new buffer exists, the capacity moves only then
template <typename T>
static int grow(HostBuf<T> &buf, size_t &cap, size_t want, size_t elems_each) {
    if (want <= cap) return PSDR_OK;
    PSDRCHK(buf.alloc(want * elems_each));
    cap = want;
    return PSDR_OK;
}
extern "C" int psdr_fetch_begin(psdr_ctx *c, unsigned what) {
    // 1. the call against the context's state
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (what == 0 || (what & ~(PSDR_FETCH_AUDIO | PSDR_FETCH_PCM | PSDR_FETCH_WATERFALL | PSDR_FETCH_IQ))) return fail(PSDR_ERR_INVALID, "PSDR_FETCH_* bits 0x%x", what);
    const bool want_audio = fetch_wants_audio(what);
    if (want_audio && c->n <= 0) return fail(PSDR_ERR_STATE, "context created with audio_fft_size 0");
    FetchFacts f;
    f.what = what, f.S = c->aslots.size(), f.mb = (size_t)c->max_batch, f.F = (size_t)c->last_demod_frames, f.h = (size_t)c->n / 2, f.pcm16 = c->pcm_is16;
    if (want_audio && (f.F == 0 || c->demod_seq == 0)) return fail(PSDR_ERR_STATE, "no demodulated batch to fetch");
    if ((what & PSDR_FETCH_PCM) && !c->post_on) return fail(PSDR_ERR_STATE, "PSDR_FETCH_PCM: post chain not enabled (psdr_set_post_chain)");
    HIPCHK(hipSetDevice(c->device));
    if (!c->fetch_stream) PSDRCHK(c->fetch_stream.create());
    if ((what & PSDR_FETCH_PCM) && !c->fetch_stream_pcm) PSDRCHK(c->fetch_stream_pcm.create());
    if (!c->ev_fetch_src) PSDRCHK(c->ev_fetch_src.create());
    FetchSet &fs = c->fset[c->fetch_fill];
    if (fs.inflight) PSDRCHK(retire(c, fs));  // every set in flight: the oldest one has to land first (its results are given up: psdr_fetch_end was not called)
    c->fetch_cur = ring_cur_after_begin(c->fetch_cur, c->fetch_fill);  // (the set psdr_fetched_* read: its pointers die now)
    // 2. who holds which slot, and what the last batches did for it
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        fs.win.resize(f.S);
        fs.slots.resize(f.S);
        for (size_t i = 0; i < f.S; i++) {
            const AudioSlot &sl = c->aslots[i];
            fs.slots[i] = FetchSlot{sl.active, sl.last_seq == c->demod_seq, sl.b_mode, sl.b_sq_on};
            FetchWin &w = fs.win[i];
            w.last_seq = sl.active ? sl.last_seq : 0;
            w.born = sl.born;
            w.l = sl.b_l, w.r = sl.b_r, w.mid = sl.b_mid, w.mode = sl.b_mode;
            w.sq = fetch_in_span(what, fs.slots[i], SPAN_SQ);
        }
        // the noise power rows travel as the squelch flags do, with any of the audio bits: one span, planned beside fetch_plan
        fs.nf_on.assign(f.S, 0);
        fs.nf.at = FetchSpan{};
        if (want_audio && c->noise) {
            noise_fetch_span(c->aslots.data(), f.S, c->demod_seq, &fs.nf.at.lo, &fs.nf.at.n);
            for (size_t i = 0; i < f.S; i++) fs.nf_on[i] = c->aslots[i].active && c->aslots[i].last_seq == c->demod_seq && c->aslots[i].b_nf_on;
        }
        fs.wfm.assign(c->wslots.begin(), c->wslots.end());
    }
    // 3. the copies
    const FetchPlan p = fetch_plan(f, fs.slots.data(), fs.wfm.data(), fs.wfm.size());
    // 4. what they land in (each block on its own: a failed allocation leaves nothing half-initialised behind for the next call)
    for (Event *e : {&fs.done, &fs.ev_wf, &fs.ev_audio, &fs.ev_pcm})
        if (!*e) PSDRCHK(e->create());
    if (want_audio && !fs.pwr) PSDRCHK(fs.pwr.alloc(f.S * f.mb));
    if (want_audio && !fs.nan) PSDRCHK(fs.nan.alloc(f.S * f.mb));
    if ((what & PSDR_FETCH_AUDIO) && !fs.audio) PSDRCHK(fs.audio.alloc(f.S * f.mb * f.h));
    if ((what & PSDR_FETCH_PCM) && !fs.pcm) PSDRCHK(fs.pcm.alloc(f.S * f.mb * f.h));
    PSDRCHK(grow(fs.iq.buf, fs.iq.cap, (size_t)p.span[SPAN_IQ].n, f.mb * f.h));
    PSDRCHK(grow(fs.car.buf, fs.car.cap, (size_t)p.span[SPAN_CAR].n, f.mb));
    PSDRCHK(grow(fs.sq.buf, fs.sq.cap, (size_t)p.span[SPAN_SQ].n, f.mb));
    PSDRCHK(grow(fs.nf.buf, fs.nf.cap, (size_t)fs.nf.at.n, f.mb));
    PSDRCHK(grow(fs.wf, fs.wf_cap, p.wf_bytes, 1));
    fs.iq.at = p.span[SPAN_IQ], fs.car.at = p.span[SPAN_CAR], fs.sq.at = p.span[SPAN_SQ];
    fs.iq_bytes = p.iq_bytes;
    // 5. enqueue: behind the demodulation and the waterfall gather of the last batch (both on `side`) ...
    const hipStream_t st[2] = {c->fetch_stream, c->fetch_stream_pcm};
    void *const dst[FB_COUNT] = {fs.wf.get(), fs.pwr.get(), fs.nan.get(), fs.audio.get(), fs.iq.buf.get(), fs.car.buf.get(), fs.sq.buf.get(), fs.pcm.get()};
    const void *const src[FB_COUNT] = {c->d_wfout.get(), c->d_pwr, c->d_nan, c->d_audio, c->d_iq, c->d_car, c->d_sq, c->post.pcm};
    const size_t elem[FB_COUNT] = {1, sizeof(float), sizeof(int), sizeof(float), sizeof(cf), sizeof(cf), sizeof(int), f.pcm16 ? sizeof(int16_t) : sizeof(int32_t)};
    auto enqueue = [&](const FetchCopy &k) -> int {
        const char *from = static_cast<const char *>(src[k.buf]) + k.src_off * elem[k.buf];
        if (k.pitched)
            HIPCHK(hipMemcpy2DAsync(dst[k.buf], k.pitch, from, k.pitch, k.width, k.rows, hipMemcpyDeviceToHost, st[k.stream]));
        else
            HIPCHK(hipMemcpyAsync(dst[k.buf], from, k.rows * k.pitch, hipMemcpyDeviceToHost, st[k.stream]));
        if (k.after == FE_WF) {
            HIPCHK(hipEventRecord(fs.ev_wf, st[k.stream]));
            c->guard_wf = fs.ev_wf;
        } else if (k.after == FE_AUDIO) {  // (the pools of the spans' rows alternate with the audio's: ev_audio guards them too)
            HIPCHK(hipEventRecord(fs.ev_audio, st[k.stream]));
            c->guard_audio[c->out_set] = fs.ev_audio;
        } else if (k.after == FE_PCM) {
            HIPCHK(hipEventRecord(fs.ev_pcm, st[k.stream]));
            c->guard_pcm[c->pcm_set] = fs.ev_pcm;
        }
        return PSDR_OK;
    };
    HIPCHK(hipEventRecord(c->ev_fetch_src, c->side));
    HIPCHK(hipStreamWaitEvent(st[0], c->ev_fetch_src, 0));
    for (int i = 0; i < p.n0; i++) {
        if (p.copy[i].after == FE_AUDIO && fs.nf.at.n > 0) {  // in front of the last of the audio copies: ev_audio guards the W rows' pool too
            const FetchCopy k = fetch_rows(f, FB_PWR, (size_t)fs.nf.at.lo, (size_t)fs.nf.at.n, 1, sizeof(float));
            if (k.pitched)
                HIPCHK(hipMemcpy2DAsync(fs.nf.buf.get(), k.pitch, c->d_nf + k.src_off, k.pitch, k.width, k.rows, hipMemcpyDeviceToHost, st[0]));
            else
                HIPCHK(hipMemcpyAsync(fs.nf.buf.get(), c->d_nf + k.src_off, k.rows * k.pitch, hipMemcpyDeviceToHost, st[0]));
        }
        PSDRCHK(enqueue(p.copy[i]));
    }
    HIPCHK(hipEventRecord(fs.done, st[0]));
    fs.has_pcm = false;
    if (p.has_pcm) {
        // ... the PCM behind the chain's output kernel of that batch (up to two steps after the passes) on a copy stream of
        // ITS OWN: on the one stream the next batch's waterfall rows and audio would queue behind a copy that waits for
        // the chain - and the gather / demodulation that wait for THOSE copies with them (256 clients: +33 % on the step)
        HIPCHK(hipStreamWaitEvent(st[1], c->ev_fetch_src, 0));
        if (c->chain_seq > 0 && c->pc_s[0] && c->side != c->stream)
            HIPCHK(hipStreamWaitEvent(st[1], c->pc.ev[3][(c->chain_seq - 1) % psdr_ctx::PC_SETS], 0));
        fs.pcm16 = f.pcm16;  // (PSDR_OPT_POST_CHAIN_PCM16: the rows are int16 - the same buffers, half the bytes)
        PSDRCHK(enqueue(p.copy[p.n0]));
        fs.has_pcm = true;
    }
    fs.inflight = true;
    fs.what = what;
    fs.frames = p.frames;
    fs.seq = p.carries_seq ? c->demod_seq : 0;
    c->fetch_fill = ring_next(c->fetch_fill);
    c->fetch_inflight++;
    return PSDR_OK;
}
extern "C" int psdr_fetch_end(psdr_ctx *c) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (c->fetch_inflight <= 0) return fail(PSDR_ERR_STATE, "psdr_fetch_end without a psdr_fetch_begin in flight");
    const int k = ring_oldest(c->fetch_fill, c->fetch_inflight);
    FetchSet &fs = c->fset[k];
    if (!fs.inflight) return fail(PSDR_ERR_STATE, "psdr_fetch_end: the fetch ring is out of step");
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(retire(c, fs));
    c->fetch_cur = k;
    return PSDR_OK;
}
extern "C" int psdr_fetch_batch(psdr_ctx *c) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (c->n <= 0) return fail(PSDR_ERR_STATE, "context created with audio_fft_size 0");
    if (c->last_demod_frames == 0 || c->demod_seq == 0) return fail(PSDR_ERR_STATE, "no demodulated batch to fetch");
    // the synchronous form: everything there is, and the device drained (errors of the batch surface here)
    while (c->fetch_inflight > 0) PSDRCHK(psdr_fetch_end(c));
    PSDRCHK(drain(c));
    PSDRCHK(psdr_fetch_begin(c, PSDR_FETCH_AUDIO | (c->post_on ? PSDR_FETCH_PCM : 0u) | PSDR_FETCH_WATERFALL | (c->d_iq ? PSDR_FETCH_IQ : 0u)));
    return psdr_fetch_end(c);
}

// ---- psdr_fetched_*: answers from the set the last psdr_fetch_end completed -----------------------------------------------
static int fetched_set(psdr_ctx *c, const FetchSet **out) {
    if (c->fetch_cur < 0) return fail(PSDR_ERR_STATE, "psdr_fetch_batch() / psdr_fetch_end() first");
    *out = &c->fset[c->fetch_cur];
    return PSDR_OK;
}
// A slot whose client attached AFTER the batch was demodulated holds the previous occupant's results (or nothing): the
// reference's per-client task would not exist for that frame either (src/websocket.cpp:156-185 walks signal_slices at the
// time of the frame).  PSDR_ERR_NO_DATA.
static int slot_in_fetched_set(psdr_ctx *c, const FetchSet *fs, int id, RowKind kind) {
    if ((size_t)id >= fs->win.size() || !fetched_member(fs->win[id], fs->seq, c->aslots[id].born))
        return fail(PSDR_ERR_NO_DATA, "client %d was not part of the fetched batch", id);
    if (kind != ROWS_ANY && !iq_kind_matches(fs->win[id].mode, kind == ROWS_IQ))
        return fail(PSDR_ERR_NO_DATA, kind == ROWS_IQ ? "client %d was not demodulated as PSDR_IQ in the fetched batch" : "client %d was demodulated as PSDR_IQ in the fetched batch: psdr_fetched_iq", id);
    return PSDR_OK;
}
// the start of every per-client answer, under mtx once: the slot, the current set, that it carries what is asked for (`need`:
// PSDR_FETCH_* bits beyond a demodulated batch; pcm16: ... as int16 rows), the client's part in the batch as `kind`
static int fetched_begin(psdr_ctx *c, int id, const char *carries, unsigned need, bool pcm16, RowKind kind, const FetchSet **out) {
    std::lock_guard<std::mutex> lk(c->mtx);
    PSDRCHK(check_slot(c, id));
    PSDRCHK(fetched_set(c, out));
    const FetchSet *fs = *out;
    if (fs->seq == 0 || (fs->what & need) != need) return fail(PSDR_ERR_STATE, "the fetched batch carries no %s", carries);
    if (pcm16 && !fs->pcm16) return fail(PSDR_ERR_STATE, "the fetched PCM rows are int32 (PSDR_OPT_POST_CHAIN_PCM16 was 0 for that batch): psdr_fetched_audio");
    return slot_in_fetched_set(c, fs, id, kind);
}
static int fetched_frame(const FetchSet *fs, int frame) {
    if (frame < 0 || frame >= fs->frames) return fail(PSDR_ERR_INVALID, "frame %d not in the fetched batch of %d", frame, fs->frames);
    return PSDR_OK;
}
extern "C" int psdr_fetched_window(psdr_ctx *c, int id, int *l, double *audio_mid, int *r) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    const FetchSet *fs = nullptr;
    PSDRCHK(fetched_begin(c, id, "audio (PSDR_FETCH_AUDIO / _PCM)", 0, false, ROWS_ANY, &fs));
    if (l) *l = fs->win[id].l;
    if (audio_mid) *audio_mid = fs->win[id].mid;
    if (r) *r = fs->win[id].r;
    return PSDR_OK;
}
extern "C" int psdr_fetched_audio(psdr_ctx *c, int id, int frame, const float **audio, float *pwr, int32_t *nan_flag,
                                  const int32_t **pcm) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    const FetchSet *fs = nullptr;
    PSDRCHK(fetched_begin(c, id, "audio (PSDR_FETCH_AUDIO / _PCM)", 0, false, ROWS_AUDIO, &fs));
    PSDRCHK(fetched_frame(fs, frame));
    const size_t h = (size_t)c->n / 2, row = fetch_row(id, (size_t)c->max_batch, frame);
    if (audio) *audio = (fs->what & PSDR_FETCH_AUDIO) ? fs->audio + row * h : nullptr;
    if (pwr) *pwr = fs->pwr[row];
    if (nan_flag) *nan_flag = fs->nan[row];
    if (pcm) *pcm = ((fs->what & PSDR_FETCH_PCM) && !fs->pcm16) ? fs->pcm + row * h : nullptr;  // (int16 rows: psdr_fetched_pcm16)
    return PSDR_OK;
}
extern "C" int psdr_fetched_pcm16(psdr_ctx *c, int id, int frame, const int16_t **pcm) {
    if (!c || !pcm) return fail(PSDR_ERR_INVALID, "null argument");
    const FetchSet *fs = nullptr;
    PSDRCHK(fetched_begin(c, id, "PCM (PSDR_FETCH_PCM)", PSDR_FETCH_PCM, true, ROWS_AUDIO, &fs));
    PSDRCHK(fetched_frame(fs, frame));
    *pcm = reinterpret_cast<const int16_t *>(fs->pcm.get()) + fetch_row(id, (size_t)c->max_batch, frame) * ((size_t)c->n / 2);
    return PSDR_OK;
}
extern "C" int psdr_fetched_iq(psdr_ctx *c, int id, int frame, const float **iq, float *pwr, int32_t *nan_flag) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    const FetchSet *fs = nullptr;
    PSDRCHK(fetched_begin(c, id, "audio (PSDR_FETCH_AUDIO / _PCM / _IQ)", 0, false, ROWS_IQ, &fs));
    PSDRCHK(fetched_frame(fs, frame));
    const size_t h = (size_t)c->n / 2, mb = (size_t)c->max_batch, row = fetch_row(id, mb, frame);
    // (an IQ slot of a set fetched with PSDR_FETCH_IQ lies inside the span by construction)
    const bool have = (fs->what & PSDR_FETCH_IQ) && fs->iq.at.holds(id);
    if (iq) *iq = have ? reinterpret_cast<const float *>(fs->iq.buf.get() + span_row(fs->iq.at, id, mb, frame) * h) : nullptr;
    if (pwr) *pwr = fs->pwr[row];
    if (nan_flag) *nan_flag = fs->nan[row];
    return PSDR_OK;
}
extern "C" int psdr_fetched_carrier(psdr_ctx *c, int id, int frame, float *level, float *offset_hz) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    const FetchSet *fs = nullptr;
    PSDRCHK(fetched_begin(c, id, "audio (PSDR_FETCH_AUDIO / _PCM / _IQ)", 0, false, ROWS_AUDIO, &fs));
    if (fs->win[id].mode != PSDR_SAM || !fs->car.at.holds(id)) return fail(PSDR_ERR_NO_DATA, "client %d was not demodulated as PSDR_SAM in the fetched batch", id);
    PSDRCHK(fetched_frame(fs, frame));
    const cf rec = fs->car.buf[span_row(fs->car.at, id, (size_t)c->max_batch, frame)];
    if (level) *level = rec.x;
    if (offset_hz) *offset_hz = rec.y;
    return PSDR_OK;
}
extern "C" int psdr_fetched_squelch(psdr_ctx *c, int id, int frame, int32_t *open) {
    if (!c || !open) return fail(PSDR_ERR_INVALID, "null argument");
    const FetchSet *fs = nullptr;
    PSDRCHK(fetched_begin(c, id, "audio (PSDR_FETCH_AUDIO / _PCM / _IQ)", 0, false, ROWS_ANY, &fs));
    PSDRCHK(fetched_frame(fs, frame));
    // (a slot that ran with squelch lies inside the span by construction; any other reads open)
    const bool have = fs->win[id].sq && fs->sq.at.holds(id);
    *open = have ? fs->sq.buf[span_row(fs->sq.at, id, (size_t)c->max_batch, frame)] : 1;
    return PSDR_OK;
}
extern "C" int psdr_fetched_noise(psdr_ctx *c, int id, int frame, float *w) {
    if (!c || !w) return fail(PSDR_ERR_INVALID, "null argument");
    const FetchSet *fs = nullptr;
    PSDRCHK(fetched_begin(c, id, "audio (PSDR_FETCH_AUDIO / _PCM / _IQ)", 0, false, ROWS_ANY, &fs));
    PSDRCHK(fetched_frame(fs, frame));
    // (a slot that ran with the noise floor lies inside the span by construction; any other reads 0)
    const bool have = (size_t)id < fs->nf_on.size() && fs->nf_on[id] && fs->nf.at.holds(id);
    *w = have ? fs->nf.buf[span_row(fs->nf.at, id, (size_t)c->max_batch, frame)] : 0.f;
    return PSDR_OK;
}
extern "C" int psdr_fetched_iq_span(psdr_ctx *c, int *first_slot, int *nslots, size_t *bytes) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    const FetchSet *fs = nullptr;
    PSDRCHK(fetched_set(c, &fs));
    if (!(fs->what & PSDR_FETCH_IQ)) return fail(PSDR_ERR_STATE, "the fetched batch carries no IQ rows (PSDR_FETCH_IQ)");
    if (first_slot) *first_slot = fs->iq.at.lo;
    if (nslots) *nslots = fs->iq.at.n;
    if (bytes) *bytes = fs->iq_bytes;
    return PSDR_OK;
}
extern "C" int psdr_fetched_waterfall(psdr_ctx *c, int id, const int8_t **rows, int *nsent_out, int *level_out, int *l_out, int *r_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    const FetchSet *fs = nullptr;
    PSDRCHK(fetched_set(c, &fs));
    if (!(fs->what & PSDR_FETCH_WATERFALL)) return fail(PSDR_ERR_STATE, "the fetched batch carries no waterfall rows (PSDR_FETCH_WATERFALL)");
    if (id < 0 || (size_t)id >= fs->wfm.size() || !fs->wfm[id].active) return fail(PSDR_ERR_NO_DATA, "waterfall client %d was not part of the fetched batch", id);
    const WfSlot &w = fs->wfm[id];
    if (rows) *rows = w.nsent > 0 ? fs->wf + w.out_off : nullptr;
    if (nsent_out) *nsent_out = w.nsent;
    if (level_out) *level_out = w.b_level;
    if (l_out) *l_out = w.b_l;
    if (r_out) *r_out = w.b_r;
    return PSDR_OK;
}

// ---- psdr_read_*: one client's rows of the last batch, synchronously --------------------------------------------------------
// the same rule for the last batch: a slot whose client attached after it holds somebody else's rows.  Under mtx.
static int slot_in_last_batch(psdr_ctx *c, int id, RowKind kind) {
    if (c->demod_seq == 0 || c->aslots[id].last_seq != c->demod_seq)
        return fail(PSDR_ERR_NO_DATA, "client %d was not part of the last demodulation batch", id);
    if (kind != ROWS_ANY && !iq_kind_matches(c->aslots[id].b_mode, kind == ROWS_IQ))
        return fail(PSDR_ERR_NO_DATA, kind == ROWS_IQ ? "client %d was not demodulated as PSDR_IQ in the last batch" : "client %d was demodulated as PSDR_IQ in the last batch: psdr_read_iq", id);
    return PSDR_OK;
}
// the start of every read, under mtx once: the slot, (need_post: the post chain,) a batch, room for its frames (nframes < 0:
// the call has no rows), the client's part in it as `kind` (sam: ... as PSDR_SAM); `snapshot` takes what else the call needs
// from the slot.  *nframes_out is written once the batch is known to fit.
template <typename Snapshot>
static int read_begin(psdr_ctx *c, int id, bool need_post, int nframes, int *nframes_out, RowKind kind, bool sam, size_t *F_out, Snapshot snapshot) {
    std::lock_guard<std::mutex> lk(c->mtx);
    PSDRCHK(check_slot(c, id));
    if (need_post && !c->post_on) return fail(PSDR_ERR_STATE, "post chain not enabled (psdr_set_post_chain)");
    const size_t F = (size_t)c->last_demod_frames;
    if (F == 0) return fail(PSDR_ERR_STATE, "no demodulated batch to read");
    if (nframes >= 0 && nframes < (int)F) return fail(PSDR_ERR_INVALID, "buffers hold %d frames, the last batch has %zu", nframes, F);
    if (nframes_out) *nframes_out = (int)F;
    PSDRCHK(slot_in_last_batch(c, id, kind));
    if (sam && (c->aslots[id].b_mode != PSDR_SAM || !c->d_car)) return fail(PSDR_ERR_NO_DATA, "client %d was not demodulated as PSDR_SAM in the last batch", id);
    snapshot(c->aslots[id]);
    *F_out = F;
    return PSDR_OK;
}
static int read_begin(psdr_ctx *c, int id, bool need_post, int nframes, int *nframes_out, RowKind kind, bool sam, size_t *F_out) {
    return read_begin(c, id, need_post, nframes, nframes_out, kind, sam, F_out, [](const AudioSlot &) {});
}
extern "C" int psdr_read_pcm(psdr_ctx *c, int id, int nframes, int32_t *pcm, int *nframes_out) {
    if (!c || !pcm) return fail(PSDR_ERR_INVALID, "null argument");
    size_t F = 0;
    PSDRCHK(read_begin(c, id, true, nframes, nframes_out, ROWS_AUDIO, false, &F));
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    const size_t h = (size_t)c->n / 2, first = fetch_row(id, (size_t)c->max_batch, 0) * h;
    if (c->pcm_is16) {  // PSDR_OPT_POST_CHAIN_PCM16: the rows are int16 on the device; this call still delivers the reference's int32 buffer
        std::vector<int16_t> tmp(F * h);
        HIPCHK(hipMemcpy(tmp.data(), reinterpret_cast<const int16_t *>(c->post.pcm) + first, F * h * sizeof(int16_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < F * h; i++) pcm[i] = tmp[i];
    } else {
        HIPCHK(hipMemcpy(pcm, c->post.pcm + first, F * h * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return PSDR_OK;
}
// rows, pwr and NaN flags of one slot (psdr_read_audio / psdr_read_iq): any pointer may be null
template <typename T>
static int read_rows(psdr_ctx *c, int id, size_t F, const T *d_rows, void *rows, float *pwr, int32_t *nan_flags) {
    const size_t h = (size_t)c->n / 2, first = fetch_row(id, (size_t)c->max_batch, 0);
    if (rows) HIPCHK(hipMemcpyAsync(rows, d_rows + first * h, F * h * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    if (pwr) HIPCHK(hipMemcpyAsync(pwr, c->d_pwr + first, F * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (nan_flags) HIPCHK(hipMemcpyAsync(nan_flags, c->d_nan + first, F * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PSDR_OK;
}
extern "C" int psdr_read_audio(psdr_ctx *c, int id, int nframes, float *audio, float *pwr, int32_t *nan_flags,
                               int *nframes_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    size_t F = 0;
    PSDRCHK(read_begin(c, id, false, nframes, nframes_out, ROWS_AUDIO, false, &F));
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    return read_rows(c, id, F, c->d_audio, audio, pwr, nan_flags);
}
extern "C" int psdr_read_iq(psdr_ctx *c, int id, int nframes, float *iq, float *pwr, int32_t *nan_flags, int *nframes_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    size_t F = 0;
    PSDRCHK(read_begin(c, id, false, nframes, nframes_out, ROWS_IQ, false, &F));
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    return read_rows(c, id, F, c->d_iq, iq, pwr, nan_flags);
}
extern "C" int psdr_read_carrier(psdr_ctx *c, int id, int nframes, float *level, float *offset_hz, int *nframes_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    size_t F = 0;
    PSDRCHK(read_begin(c, id, false, nframes, nframes_out, ROWS_AUDIO, true, &F));
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    std::vector<cf> rec(F);
    HIPCHK(hipMemcpyAsync(rec.data(), c->d_car + fetch_row(id, (size_t)c->max_batch, 0), F * sizeof(cf), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t f = 0; f < F; f++) {
        if (level) level[f] = rec[f].x;
        if (offset_hz) offset_hz[f] = rec[f].y;
    }
    return PSDR_OK;
}
extern "C" int psdr_read_squelch(psdr_ctx *c, int id, int nframes, int32_t *open, int *nframes_out) {
    if (!c || !open) return fail(PSDR_ERR_INVALID, "null argument");
    size_t F = 0;
    bool on = false;
    PSDRCHK(read_begin(c, id, false, nframes, nframes_out, ROWS_ANY, false, &F, [&](const AudioSlot &s) { on = s.b_sq_on; }));
    if (!on) {  // the batch ran without squelch for this client: every frame is heard (the host snapshot answers)
        std::fill(open, open + F, 1);
        return PSDR_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    HIPCHK(hipMemcpy(open, c->d_sq + fetch_row(id, (size_t)c->max_batch, 0), F * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PSDR_OK;
}
// the tone decoder's records of the last batch; any of the three arrays may be null
extern "C" int psdr_read_tone(psdr_ctx *c, int id, int nframes, int32_t *tone, float *level, int32_t *open, int *nframes_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    size_t F = 0;
    bool on = false;
    PSDRCHK(read_begin(c, id, false, nframes, nframes_out, ROWS_AUDIO, false, &F, [&](const AudioSlot &s) { on = s.b_tone_on && (bool)c->tone; }));
    if (!on) return fail(PSDR_ERR_NO_DATA, "client %d had no tone decoder in the last demodulation batch", id);
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    std::vector<ToneRec> rec(F);
    HIPCHK(hipMemcpy(rec.data(), c->tone.rec + fetch_row(id, (size_t)c->max_batch, 0), F * sizeof(ToneRec), hipMemcpyDeviceToHost));
    for (size_t f = 0; f < F; f++) {
        if (tone) tone[f] = rec[f].tone;
        if (level) level[f] = rec[f].level;
        if (open) open[f] = rec[f].open;
    }
    return PSDR_OK;
}
// the CW decoder's records of the last batch; any of the five arrays may be null
extern "C" int psdr_read_cw(psdr_ctx *c, int id, int nframes, uint32_t *nchars, float *wpm, float *pitch_hz, float *level, int32_t *key, int *nframes_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    size_t F = 0;
    bool on = false;
    PSDRCHK(read_begin(c, id, false, nframes, nframes_out, ROWS_AUDIO, false, &F, [&](const AudioSlot &s) { on = s.b_cw_on && (bool)c->cw; }));
    if (!on) return fail(PSDR_ERR_NO_DATA, "client %d had no CW decoder in the last demodulation batch", id);
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    std::vector<CwRec> rec(F);
    HIPCHK(hipMemcpy(rec.data(), c->cw.rec + fetch_row(id, (size_t)c->max_batch, 0), F * sizeof(CwRec), hipMemcpyDeviceToHost));
    for (size_t f = 0; f < F; f++) {
        if (nchars) nchars[f] = rec[f].nchars;
        if (wpm) wpm[f] = rec[f].wpm;
        if (pitch_hz) pitch_hz[f] = rec[f].pitch_hz;
        if (level) level[f] = rec[f].level;
        if (key) key[f] = rec[f].key;
    }
    return PSDR_OK;
}
// the CW decoder's text since the state last started, from the slot's ring
extern "C" int psdr_read_cw_text(psdr_ctx *c, int id, uint64_t from, char *out, size_t cap, size_t *n_out, uint64_t *total_out) {
    if (!c || (!out && cap)) return fail(PSDR_ERR_INVALID, "null argument");
    bool pending = false;
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        if (id < 0 || (size_t)id >= c->aslots.size()) return fail(PSDR_ERR_INVALID, "CW text: id %d outside 0..%d", id, (int)c->aslots.size() - 1);
        const AudioSlot &s = c->aslots[id];
        if (!s.active) return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
        if (!s.cw_on || !c->cw) return fail(PSDR_ERR_NO_DATA, "client %d has no CW decoder", id);
        pending = s.cw_fresh;
    }
    uint64_t total = 0;
    std::vector<uint8_t> ring;
    if (!pending) {
        HIPCHK(hipSetDevice(c->device));
        PSDRCHK(drain(c));
        CwState st;
        HIPCHK(hipMemcpy(&st, c->cw.state + (size_t)id, sizeof(CwState), hipMemcpyDeviceToHost));
        total = st.nchars;
        if (from < total && total - from <= (uint64_t)CW_TEXT) {
            ring.resize(CW_TEXT);
            HIPCHK(hipMemcpy(ring.data(), c->cw.text + (size_t)id * CW_TEXT, CW_TEXT, hipMemcpyDeviceToHost));
        }
    }
    if (from > total) return fail(PSDR_ERR_INVALID, "CW text: from %llu is beyond the text's %llu characters", (unsigned long long)from, (unsigned long long)total);
    if (total - from > (uint64_t)CW_TEXT)
        return fail(PSDR_ERR_NO_DATA, "CW text: from %llu is older than the last %d of %llu characters", (unsigned long long)from, CW_TEXT, (unsigned long long)total);
    const size_t n = std::min((size_t)(total - from), cap);
    for (size_t j = 0; j < n; j++) out[j] = (char)ring[(from + j) % CW_TEXT];
    if (n_out) *n_out = n;
    if (total_out) *total_out = total;
    return PSDR_OK;
}
// the RTTY decoder's records of the last batch; any of the six arrays may be null
extern "C" int psdr_read_rtty(psdr_ctx *c, int id, int nframes, uint32_t *nchars, uint32_t *errors, float *offset_hz, float *level, float *quality, int32_t *present,
                              int *nframes_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    size_t F = 0;
    bool on = false;
    PSDRCHK(read_begin(c, id, false, nframes, nframes_out, ROWS_AUDIO, false, &F, [&](const AudioSlot &s) { on = s.b_rtty_on && (bool)c->rtty; }));
    if (!on) return fail(PSDR_ERR_NO_DATA, "client %d had no RTTY decoder in the last demodulation batch", id);
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    std::vector<RttyRec> rec(F);
    HIPCHK(hipMemcpy(rec.data(), c->rtty.rec + fetch_row(id, (size_t)c->max_batch, 0), F * sizeof(RttyRec), hipMemcpyDeviceToHost));
    for (size_t f = 0; f < F; f++) {
        if (nchars) nchars[f] = rec[f].nchars;
        if (errors) errors[f] = rec[f].errors;
        if (offset_hz) offset_hz[f] = rec[f].offset_hz;
        if (level) level[f] = rec[f].level;
        if (quality) quality[f] = rec[f].quality;
        if (present) present[f] = rec[f].present;
    }
    return PSDR_OK;
}
// the RTTY decoder's text since the state last started, from the slot's ring
extern "C" int psdr_read_rtty_text(psdr_ctx *c, int id, uint64_t from, char *out, size_t cap, size_t *n_out, uint64_t *total_out) {
    if (!c || (!out && cap)) return fail(PSDR_ERR_INVALID, "null argument");
    bool pending = false;
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        if (id < 0 || (size_t)id >= c->aslots.size()) return fail(PSDR_ERR_INVALID, "RTTY text: id %d outside 0..%d", id, (int)c->aslots.size() - 1);
        const AudioSlot &s = c->aslots[id];
        if (!s.active) return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
        if (!s.rtty_on || !c->rtty) return fail(PSDR_ERR_NO_DATA, "client %d has no RTTY decoder", id);
        pending = s.rtty_fresh;
    }
    uint64_t total = 0;
    std::vector<uint8_t> ring;
    if (!pending) {
        HIPCHK(hipSetDevice(c->device));
        PSDRCHK(drain(c));
        std::vector<RttyState> st(1);
        HIPCHK(hipMemcpy(st.data(), c->rtty.state + (size_t)id, sizeof(RttyState), hipMemcpyDeviceToHost));
        total = st[0].nchars;
        if (from < total && total - from <= (uint64_t)RTTY_TEXT) {
            ring.resize(RTTY_TEXT);
            HIPCHK(hipMemcpy(ring.data(), c->rtty.text + (size_t)id * RTTY_TEXT, RTTY_TEXT, hipMemcpyDeviceToHost));
        }
    }
    if (from > total) return fail(PSDR_ERR_INVALID, "RTTY text: from %llu is beyond the text's %llu characters", (unsigned long long)from, (unsigned long long)total);
    if (total - from > (uint64_t)RTTY_TEXT)
        return fail(PSDR_ERR_NO_DATA, "RTTY text: from %llu is older than the last %d of %llu characters", (unsigned long long)from, RTTY_TEXT, (unsigned long long)total);
    const size_t n = std::min((size_t)(total - from), cap);
    for (size_t j = 0; j < n; j++) out[j] = (char)ring[(from + j) % RTTY_TEXT];
    if (n_out) *n_out = n;
    if (total_out) *total_out = total;
    return PSDR_OK;
}
// the PSK decoder's records of the last batch; any of the six arrays may be null
extern "C" int psdr_read_psk(psdr_ctx *c, int id, int nframes, uint32_t *nchars, uint32_t *errors, float *offset_hz, float *level, float *quality, int32_t *present,
                              int *nframes_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    size_t F = 0;
    bool on = false;
    PSDRCHK(read_begin(c, id, false, nframes, nframes_out, ROWS_AUDIO, false, &F, [&](const AudioSlot &s) { on = s.b_psk_on && (bool)c->psk; }));
    if (!on) return fail(PSDR_ERR_NO_DATA, "client %d had no PSK decoder in the last demodulation batch", id);
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    std::vector<PskRec> rec(F);
    HIPCHK(hipMemcpy(rec.data(), c->psk.rec + fetch_row(id, (size_t)c->max_batch, 0), F * sizeof(PskRec), hipMemcpyDeviceToHost));
    for (size_t f = 0; f < F; f++) {
        if (nchars) nchars[f] = rec[f].nchars;
        if (errors) errors[f] = rec[f].errors;
        if (offset_hz) offset_hz[f] = rec[f].offset_hz;
        if (level) level[f] = rec[f].level;
        if (quality) quality[f] = rec[f].quality;
        if (present) present[f] = rec[f].present;
    }
    return PSDR_OK;
}
// the PSK decoder's text since the state last started, from the slot's ring
extern "C" int psdr_read_psk_text(psdr_ctx *c, int id, uint64_t from, char *out, size_t cap, size_t *n_out, uint64_t *total_out) {
    if (!c || (!out && cap)) return fail(PSDR_ERR_INVALID, "null argument");
    bool pending = false;
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        if (id < 0 || (size_t)id >= c->aslots.size()) return fail(PSDR_ERR_INVALID, "PSK text: id %d outside 0..%d", id, (int)c->aslots.size() - 1);
        const AudioSlot &s = c->aslots[id];
        if (!s.active) return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
        if (!s.psk_on || !c->psk) return fail(PSDR_ERR_NO_DATA, "client %d has no PSK decoder", id);
        pending = s.psk_fresh;
    }
    uint64_t total = 0;
    std::vector<uint8_t> ring;
    if (!pending) {
        HIPCHK(hipSetDevice(c->device));
        PSDRCHK(drain(c));
        std::vector<PskState> st(1);
        HIPCHK(hipMemcpy(st.data(), c->psk.state + (size_t)id, sizeof(PskState), hipMemcpyDeviceToHost));
        total = st[0].nchars;
        if (from < total && total - from <= (uint64_t)PSK_TEXT) {
            ring.resize(PSK_TEXT);
            HIPCHK(hipMemcpy(ring.data(), c->psk.text + (size_t)id * PSK_TEXT, PSK_TEXT, hipMemcpyDeviceToHost));
        }
    }
    if (from > total) return fail(PSDR_ERR_INVALID, "PSK text: from %llu is beyond the text's %llu characters", (unsigned long long)from, (unsigned long long)total);
    if (total - from > (uint64_t)PSK_TEXT)
        return fail(PSDR_ERR_NO_DATA, "PSK text: from %llu is older than the last %d of %llu characters", (unsigned long long)from, PSK_TEXT, (unsigned long long)total);
    const size_t n = std::min((size_t)(total - from), cap);
    for (size_t j = 0; j < n; j++) out[j] = (char)ring[(from + j) % PSK_TEXT];
    if (n_out) *n_out = n;
    if (total_out) *total_out = total;
    return PSDR_OK;
}
// the fax decoder's records of the last batch; any of the six arrays may be null
extern "C" int psdr_read_fax(psdr_ctx *c, int id, int nframes, uint32_t *nlines, int32_t *state, uint32_t *image, int32_t *ioc, float *offset_hz, float *tone_quality,
                             int *nframes_out) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    size_t F = 0;
    bool on = false;
    PSDRCHK(read_begin(c, id, false, nframes, nframes_out, ROWS_AUDIO, false, &F, [&](const AudioSlot &s) { on = s.b_fax_on && (bool)c->fax; }));
    if (!on) return fail(PSDR_ERR_NO_DATA, "client %d had no fax decoder in the last demodulation batch", id);
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    std::vector<FaxRec> rec(F);
    HIPCHK(hipMemcpy(rec.data(), c->fax.rec + fetch_row(id, (size_t)c->max_batch, 0), F * sizeof(FaxRec), hipMemcpyDeviceToHost));
    for (size_t f = 0; f < F; f++) {
        if (nlines) nlines[f] = rec[f].nlines;
        if (state) state[f] = rec[f].state;
        if (image) image[f] = rec[f].image;
        if (ioc) ioc[f] = rec[f].ioc;
        if (offset_hz) offset_hz[f] = rec[f].offset_hz;
        if (tone_quality) tone_quality[f] = rec[f].tone_quality;
    }
    return PSDR_OK;
}
// the fax decoder's kept lines since the state last started, from the slot's ring
extern "C" int psdr_read_fax_lines(psdr_ctx *c, int id, uint64_t from, uint8_t *pix, uint32_t *meta, size_t cap_lines, size_t *n_out, uint64_t *total_out, int *width_out) {
    if (!c || ((!pix || !meta) && cap_lines)) return fail(PSDR_ERR_INVALID, "null argument");
    bool pending = false;
    int width = 0, R = 0;
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        if (id < 0 || (size_t)id >= c->aslots.size()) return fail(PSDR_ERR_INVALID, "fax lines: id %d outside 0..%d", id, (int)c->aslots.size() - 1);
        const AudioSlot &s = c->aslots[id];
        if (!s.active) return fail(PSDR_ERR_INVALID, "no audio client with id %d", id);
        if (!s.fax_on || !c->fax) return fail(PSDR_ERR_NO_DATA, "client %d has no fax decoder", id);
        pending = s.fax_fresh;
        width = s.fax.width, R = s.fax.R;
    }
    uint64_t total = 0;
    std::vector<uint8_t> ring;
    std::vector<uint32_t> rmeta;
    if (!pending) {
        HIPCHK(hipSetDevice(c->device));
        PSDRCHK(drain(c));
        std::vector<FaxState> st(1);
        HIPCHK(hipMemcpy(st.data(), c->fax.state + (size_t)id, sizeof(FaxState), hipMemcpyDeviceToHost));
        total = st[0].z.nlines;
        if (from < total && total - from <= (uint64_t)R) {
            ring.resize((size_t)R * width), rmeta.resize(R);
            HIPCHK(hipMemcpy(ring.data(), c->fax.ring + (size_t)id * c->fax.rmax * FAX_WIDTH_MAX, ring.size(), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(rmeta.data(), c->fax.meta + (size_t)id * c->fax.rmax, rmeta.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
    }
    if (from > total) return fail(PSDR_ERR_INVALID, "fax lines: from %llu is beyond the image's %llu lines", (unsigned long long)from, (unsigned long long)total);
    if (total - from > (uint64_t)R)
        return fail(PSDR_ERR_NO_DATA, "fax lines: from %llu is older than the last %d of %llu lines", (unsigned long long)from, R, (unsigned long long)total);
    const size_t n = std::min((size_t)(total - from), cap_lines);
    for (size_t j = 0; j < n; j++) {
        const size_t r = (size_t)((from + j) % (uint64_t)R);
        memcpy(pix + j * width, ring.data() + r * width, width);
        meta[j] = rmeta[r];
    }
    if (n_out) *n_out = n;
    if (total_out) *total_out = total;
    if (width_out) *width_out = width;
    return PSDR_OK;
}
extern "C" int psdr_read_noise(psdr_ctx *c, int id, int nframes, float *w, int *nframes_out) {
    if (!c || !w) return fail(PSDR_ERR_INVALID, "null argument");
    size_t F = 0;
    bool on = false;
    PSDRCHK(read_begin(c, id, false, nframes, nframes_out, ROWS_ANY, false, &F, [&](const AudioSlot &s) { on = s.b_nf_on; }));
    if (!on) {  // the batch ran without the noise floor for this client (the host snapshot answers)
        std::fill(w, w + F, 0.f);
        return PSDR_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    PSDRCHK(drain(c));
    HIPCHK(hipMemcpy(w, c->d_nf + fetch_row(id, (size_t)c->max_batch, 0), F * sizeof(float), hipMemcpyDeviceToHost));
    return PSDR_OK;
}
extern "C" int psdr_read_notches(psdr_ctx *c, int id, int first[4], int end[4]) {
    if (!c || !first || !end) return fail(PSDR_ERR_INVALID, "null argument");
    size_t F = 0;
    int man[4];
    bool have_tab = false;
    PSDRCHK(read_begin(c, id, false, -1, nullptr, ROWS_ANY, false, &F, [&](const AudioSlot &s) {
        for (int k = 0; k < 4; k++) man[k] = s.b_notch[k];
        have_tab = (bool)c->notch;
    }));
    int4 t = make_int4(0, 0, 0, 0);
    if (have_tab) {  // the table as the batch's detector left it: in force from the next batch on
        HIPCHK(hipSetDevice(c->device));
        PSDRCHK(drain(c));
        HIPCHK(hipMemcpy(&t, c->notch.tab + id, sizeof(int4), hipMemcpyDeviceToHost));
    }
    first[0] = man[0], end[0] = man[1], first[1] = man[2], end[1] = man[3];
    first[2] = t.x, end[2] = t.y, first[3] = t.z, end[3] = t.w;
    return PSDR_OK;
}
extern "C" int psdr_audio_device_ptr(psdr_ctx *c, int id, const float **d_audio, const float **d_pwr) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (id < 0 || id >= (int)c->aslots.size()) return fail(PSDR_ERR_INVALID, "bad id %d", id);
    const size_t first = fetch_row(id, (size_t)c->max_batch, 0);
    if (d_audio) *d_audio = c->d_audio + first * ((size_t)c->n / 2);
    if (d_pwr) *d_pwr = c->d_pwr + first;
    return PSDR_OK;
}
extern "C" int psdr_iq_device_ptr(psdr_ctx *c, int id, const float **d_iq, const float **d_pwr) {
    if (!c) return fail(PSDR_ERR_INVALID, "null argument");
    if (id < 0 || id >= (int)c->aslots.size()) return fail(PSDR_ERR_INVALID, "bad id %d", id);
    if (!c->d_iq) return fail(PSDR_ERR_NO_DATA, "no batch with a PSDR_IQ client has been demodulated");
    const size_t first = fetch_row(id, (size_t)c->max_batch, 0);
    if (d_iq) *d_iq = reinterpret_cast<const float *>(c->d_iq + first * ((size_t)c->n / 2));
    if (d_pwr) *d_pwr = c->d_pwr + first;
    return PSDR_OK;
}

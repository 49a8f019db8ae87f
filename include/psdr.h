/*
 * psdr.h — C-ABI of the MI355X-native spectrum-distributor DSP core (libpsdr_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of PhantomSDR (citations are
 * file:line under the reference tree):
 *
 *   Level 1  replaces the `class FFT` plug-in (src/fft.h:33-63; siblings FFTW
 *            src/fft_impl.cpp:80-183, cuFFT src/fft_cuda.cu).  A ~60-line
 *            `class hipFFT : public FFT` (phantomsdr_amd/host/hip_fft.h) forwards to it.
 *   Level 2  replaces the per-frame fan-out + per-client DSP:
 *            broadcast_server::signal_loop / waterfall_loop (src/websocket.cpp:156-185,
 *            207-236), AudioClient::send_audio up to the NaN guard
 *            (src/signal.cpp:102-275) and WaterfallClient::send_waterfall
 *            (src/waterfall.cpp:44-51), batched over frames and clients on the GPU.
 *
 * Conventions: plain pointers and sizes only; every function returns PSDR_OK (0) or a
 * negative psdr_status and never throws; psdr_last_error() gives the text for the
 * calling thread.  A context is single-producer (load/execute/process/demod from one
 * thread, like the reference's fft_thread, src/fft.cpp:14); client add/set/remove may
 * come from any thread (internal mutex = the reference's signal_slice_mtx,
 * src/signal.cpp:88).  The HIP library is the only implementation: there is no CPU
 * fallback behind this ABI.
 */
#ifndef PSDR_H
#define PSDR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psdr_ctx psdr_ctx;

typedef enum psdr_status {
    PSDR_OK = 0,
    PSDR_ERR_INVALID = -1,     /* bad argument / rejected range */
    PSDR_ERR_NO_DEVICE = -2,   /* no HIP device (cuFFT ctor throws, src/fft_cuda.cu:8-13) */
    PSDR_ERR_HIP = -3,         /* a HIP runtime call failed */
    PSDR_ERR_STATE = -4,       /* call order violated (e.g. execute before load) */
    PSDR_ERR_NOMEM = -5,
    PSDR_ERR_UNSUPPORTED = -6, /* size outside what the kernels are built for */
    PSDR_ERR_NO_DATA = -7      /* the client slot was not part of the batch whose results are asked for */
} psdr_status;

/* input.driver.format, src/spectrumserver.cpp:349-364 / src/samplereader.cpp:72-81 */
typedef enum psdr_format {
    PSDR_FMT_U8 = 0,
    PSDR_FMT_S8 = 1,
    PSDR_FMT_U16 = 2,
    PSDR_FMT_S16 = 3,
    PSDR_FMT_F32 = 4,
    PSDR_FMT_F64 = 5
} psdr_format;

/* demodulation_mode, src/client.h:43 */
/* PSDR_IQ (no counterpart in the reference's enum: its raw SIGNAL shortcut and its PLL over this baseband,
 * src/signal.cpp:110-115, 242-252, are disabled there): the client's output is the complex baseband itself, see
 * psdr_read_iq below.  PSDR_SAM: synchronous AM - AM's baseband detected against the recovered carrier (the reference's
 * HAS_LIQUID carrier transform, src/signal.cpp:205-222, without its PLL), see psdr_read_carrier below */
typedef enum psdr_mode { PSDR_USB = 0, PSDR_LSB = 1, PSDR_AM = 2, PSDR_FM = 3, PSDR_IQ = 4, PSDR_SAM = 5 } psdr_mode;

typedef struct psdr_config {
    uint32_t struct_size;        /* = sizeof(psdr_config) */
    uint32_t fft_size;           /* N, power of two (FFT::FFT size, src/fft_impl.cpp:63): IQ 2^12..2^22, real 2^13..2^23 */
    int32_t is_real;             /* plan_r2c vs plan_c2c (src/fft.cpp:25-29) */
    int32_t downsample_levels;   /* src/spectrumserver.cpp:186-190; 1..log2(R)+1 (R = N IQ, N/2 real) */
    int32_t brightness_offset;   /* src/fft_impl.cpp:69 */
    int32_t additional_size;     /* set_output_additional_size(), src/spectrumserver.cpp:214 */
    int32_t audio_fft_size;      /* n = ceil(audio_sps*N/sps/4)*4, src/websocket.cpp:133 */
    int32_t audio_rate;          /* audio_max_sps (AM carrier cutoff, AGC/DC) */
    int32_t input_format;        /* psdr_format of the raw ring used by psdr_process_batch */
    int32_t device;              /* HIP device ordinal */
    int32_t max_batch;           /* frames per psdr_process_batch call (>=1) */
    int32_t max_clients;         /* audio client slots */
    int32_t max_waterfall_clients;
    int32_t skip_num;            /* waterfall sent when frame_num % skip_num == 0 (src/fft.cpp:33,102) */
    int32_t waterfall_size;      /* min_waterfall_fft = input.waterfall_size (src/spectrumserver.cpp:56): default
                                    width of a new waterfall client (src/websocket.cpp:198) and target of the
                                    level search (src/waterfall.cpp:62-79).  0 = R >> (downsample_levels-1),
                                    which equals it whenever waterfall_size is a power of two */
} psdr_config;

const char *psdr_last_error(void);
const char *psdr_version(void);
/* ABI number of this header: bumped whenever a signature or a struct changes incompatibly.  A caller built against another
 * header should compare psdr_abi_version() (the library's) with the PSDR_ABI_VERSION it was compiled with.
 *   2 (library 0.2, round 4): psdr_group_client_set_audio_range(g, int *gid, ...), gid = (rank << 16) | slot
 *   3 (library 0.3, round 5/6): psdr_group_client_set_audio_range takes the gid BY VALUE and gids are stable handles;
 *     psdr_fetch_begin / _end / psdr_fetched_waterfall added (additions alone do not bump the number) */
#define PSDR_ABI_VERSION 3
int psdr_abi_version(void);

/* ---- lifetime -------------------------------------------------------------------- */
int psdr_create(const psdr_config *cfg, psdr_ctx **out);
void psdr_destroy(psdr_ctx *ctx);

/* ---- Level 1: the FFT plug-in (src/fft.h:33-63) ----------------------------------- */
/* FFT::malloc / FFT::free (src/fft.h:36-37; cuFFT twin src/fft_cuda.cu:22-28): pinned,
 * host-writable buffer of nfloats floats.  ctx may be NULL (the reference allocates its
 * half-frame buffers before planning, src/fft.cpp:17-29). */
int psdr_host_alloc(psdr_ctx *ctx, size_t nfloats, float **out);
int psdr_host_free(psdr_ctx *ctx, float *buf);
/* FFT::load_real_input / load_complex_input (src/fft.h:45-46, src/fft_impl.cpp:131-143):
 * a1 = older half-frame, a2 = newer, each N/2 samples (IQ: N floats each). */
int psdr_load_real_input(psdr_ctx *ctx, const float *a1, const float *a2);
int psdr_load_complex_input(psdr_ctx *ctx, const float *a1, const float *a2);
/* FFT::execute (src/fft.h:47, src/fft_impl.cpp:144-174): window, FFT, /N, power, int8
 * pyramid for the loaded frame.  Synchronous like the reference (src/fft_cuda.cu:175). */
int psdr_execute(psdr_ctx *ctx);
/* FFT::get_output_buffer (src/fft.h:43): host pointer, natural k order, N + additional
 * complex bins (IQ, the wrap copy of src/fft.cpp:91-98 already applied) or N/2+1 (real);
 * valid until the next execute/process call. */
int psdr_get_output_buffer(psdr_ctx *ctx, float **out);
/* FFT::get_quantized_buffer (src/fft.h:44): host pointer to the int8 pyramid, levels
 * back to back (level i at offset sum_{t<i} R>>t, src/websocket.cpp:233). */
int psdr_get_quantized_buffer(psdr_ctx *ctx, int8_t **out);

/* ---- device memory helpers (raw sample ring lives in HBM) ------------------------- */
int psdr_dev_alloc(psdr_ctx *ctx, size_t bytes, void **out);
int psdr_dev_free(psdr_ctx *ctx, void *p);
int psdr_memcpy_h2d(psdr_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int psdr_memcpy_d2h(psdr_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int psdr_synchronize(psdr_ctx *ctx);
/* bytes of one raw half-frame in cfg.input_format (N/2 samples, x2 components for IQ) */
size_t psdr_half_frame_bytes(const psdr_ctx *ctx);

/* ---- streaming ingest: the sample reader's double buffering (src/fft.cpp:56-67 reads half k+2
 * while frame (k, k+1) is transformed; src/samplereader.cpp:42-70) on the device ------------------
 * The context owns a ring of `nhalves` raw half-frames in HBM.  psdr_ring_write_async() copies one
 * half-frame from (pinned) host memory into slot `half_index % nhalves` on a dedicated COPY stream and
 * returns at once; psdr_process_ring() transforms frames first_half .. first_half+nframes-1 (frame f
 * = halves f, f+1; the frames of one call must not cross the end of the ring - first_half % nhalves +
 * nframes <= nhalves, the last frame's second half may be slot 0 again: size the ring as a multiple of the
 * batch) after waiting, on the device, for the copies
 * of exactly the halves it reads - so the PCIe transfer of later halves overlaps the transform of
 * earlier ones.  A slot may be rewritten as soon as the psdr_process_ring() call that read it has
 * been issued (the copy waits for that batch on the device).  The source buffer must stay valid
 * until psdr_ring_wait(ctx, half_index) (or any synchronising call) returns. */
int psdr_ring_create(psdr_ctx *ctx, int nhalves);
int psdr_ring_write_async(psdr_ctx *ctx, uint64_t half_index, const void *host_half);
int psdr_ring_wait(psdr_ctx *ctx, uint64_t half_index);
int psdr_process_ring(psdr_ctx *ctx, uint64_t first_half, int nframes);

/* ---- wideband impulse blanker on the ring, ahead of the forward FFT (no counterpart in the reference: its browser-side
 * blanker, jsdsp/lib/NB.c, works on the 12 kHz audio, where an impulse is already as long as the client's filter) ----------
 * An impulse from a power line, an electric fence or a switching supply is a few samples long at the input rate; behind an
 * N-point frame it is a raised floor in every bin, for every audio client and every waterfall row.  The raw ring is the
 * only place where it is still short.  Opt-in per context: a context that never calls psdr_ring_set_blanker allocates,
 * launches and computes exactly what it did without it.  The rule, per half-frame H of N/2 samples:
 *   power      P_i, one f32 per sample.  Integer formats: the converter's unscaled integers a, b (behind the MSB flip of u8 /
 *              u16), a*a + b*b (real input: a*a) exactly in unsigned 32-bit arithmetic (at most 2^31), converted once to f32,
 *              round to nearest even.  f32: fl(fl(re*re) + fl(im*im)), nothing fused.  f64: narrowed to f32 first, as the first
 *              FFT pass does.  Every maximum is m = (P > m) ? P : m from +0.0: a NaN P is never a maximum and never above a
 *              threshold.
 *   reference  the half is cut into blocks of 256 consecutive samples (at least 8).  M_b = the maximum of P over block b,
 *              R_H = the minimum of M_b over the half's blocks: a few impulses raise a few M_b and leave the minimum alone.
 *              For complex Gaussian noise of mean power mu, R sits around 4 - 6 mu: threshold_db is relative to R, NOT to
 *              the mean power.
 *   threshold  kf = (float)pow(10, threshold_db / 10); T_H = kf * R_(H-1), one f32 product: the level comes from the RAW
 *              samples of the half before.  If half H - 1 was not blanked by this context directly before H (the first half
 *              after switching on, a jump ahead in first_half), R_(H-1) := R_H.  T_H = 0 (digital silence) or not finite (an
 *              Inf half): nothing in half H is blanked.
 *   blanking   exceed_j = (P_j > T_H) on the raw samples; sample i of half H is zeroed if and only if some j of the SAME half
 *              with |i - j| <= guard exceeds (the guard is clipped to the half).  Both components are zeroed, to the code the
 *              converter maps to 0.0: 0 for signed formats, +0.0 for floats, 0x80 for u8, 0x8000 for u16.
 * Each half is blanked exactly once, in place, inside the psdr_process_ring call that first reads it: on the context's stream,
 * behind the waits for the half's copy and in front of the first FFT pass.  The half in slot 0 exists twice (slot 0 and its
 * mirror behind the last slot): both copies get the same bytes.  The library keeps the index of the next half to blank: halves
 * below it are skipped (a call that re-reads old halves), a call whose first half lies above it restarts the reference.  Any
 * split of the same stream into psdr_process_ring calls gives the same ring bytes, counts and levels.
 * psdr_ring_set_blanker: frame-loop thread only, like the ring calls; takes force at the next psdr_process_ring; switching on
 * starts the reference afresh.  threshold_db finite in [0, 90], guard in 0..255 (on = 0 ignores both) - anything else is
 * PSDR_ERR_INVALID and changes nothing; PSDR_ERR_STATE without a ring.  The first on = 1 allocates the device state (block
 * maxima, levels and counts of max_batch + 1 halves, the blocks' masks), all or none: PSDR_ERR_NOMEM leaves the setting as
 * it was.  psdr_process_batch (the caller's const buffer), the Level-1 path and psdr_group_* are not touched.
 * psdr_ring_read_blanker: for a half blanked by the LAST psdr_process_ring call, the number of samples zeroed (what a
 * "blanker active" indicator shows) and R_H; synchronises; PSDR_ERR_NO_DATA for any other half; either pointer may be NULL.
 * psdr_ring_read: drains, then copies slot half_index % nhalves to host_half (psdr_half_frame_bytes) - the slot's bytes as
 * the first pass reads them; for a server that records. */
int psdr_ring_set_blanker(psdr_ctx *ctx, int on, double threshold_db, int guard);
int psdr_ring_read_blanker(psdr_ctx *ctx, uint64_t half_index, uint32_t *blanked, float *ref_level);
int psdr_ring_read(psdr_ctx *ctx, uint64_t half_index, void *host_half);

/* ---- Level 2: batched frames ------------------------------------------------------ */
/* Frame loop body, src/fft.cpp:47-105, for nframes consecutive frames at once.
 * d_halves: device pointer to nframes+1 consecutive raw half-frames (cfg.input_format);
 * frame f = [half f ; half f+1] (50 % overlap, src/fft.cpp:49-53).  Device-side sample
 * conversion = src/samplereader.cpp:29-40.  Asynchronous on the context's stream. */
int psdr_process_batch(psdr_ctx *ctx, const void *d_halves, int nframes);

/* audio clients: AudioClient (src/signal.h:53-123) */
int psdr_client_add(psdr_ctx *ctx, int *id_out);
int psdr_client_remove(psdr_ctx *ctx, int id);
/* AudioClient::set_audio_range (src/signal.cpp:81-94): unchecked, like the reference */
int psdr_client_set_audio_range(psdr_ctx *ctx, int id, int l, double audio_mid, int r);
/* AudioClient::on_window_message (src/signal.cpp:300-314): validated; PSDR_ERR_INVALID
 * (and no change) when the reference would silently return */
int psdr_client_on_window_message(psdr_ctx *ctx, int id, int l, double audio_mid, int r);
/* AudioClient::set_audio_demodulation / on_demodulation_message (src/signal.cpp:95-97,316-328).
 * The first PSDR_IQ of a context allocates the IQ rows: two sets of 8 * (audio_fft_size/2) bytes per client slot and
 * batch frame, i.e. 16 * (audio_fft_size/2) * max_clients * max_batch bytes in all (a context that never sees an IQ client
 * allocates none); PSDR_ERR_NOMEM, and the mode unchanged, if that fails.  The first PSDR_SAM allocates the carrier tails
 * (16 * (audio_fft_size/2) bytes per client slot) and two sets of carrier records (8 bytes per client slot and batch
 * frame each), all or none, with the same answer on failure; PSDR_ERR_STATE if the context's audio_rate is not positive;
 * PSDR_ERR_UNSUPPORTED, and the mode unchanged, if audio_fft_size >= 65536 (PSDR_SAM below: the carrier's direct sum). */
int psdr_client_set_audio_demodulation(psdr_ctx *ctx, int id, int mode);
/* signal_loop's slow-client rule (src/websocket.cpp:170-176): the reference does not call send_audio at all for a
 * client with more than 50 kB queued on its socket, so NOTHING of that client moves for the frame - overlap-add tails and
 * FM's last sample (src/signal.cpp:200-203, 273-275), DC blocker and AGC (:277-284).  A paused client sits out every
 * psdr_demod_batch* until it is resumed (paused = 0): its state is frozen bit for bit, and its results read as
 * PSDR_ERR_NO_DATA for those batches.  A Level-2 caller evaluates the backlog BEFORE the frame is demodulated
 * (phantomsdr_amd/host/hip_level2.h). */
int psdr_client_set_paused(psdr_ctx *ctx, int id, int paused);
/* signal_loop + send_audio (src/websocket.cpp:156-185, src/signal.cpp:102-275) for every
 * active client over the frames of the last psdr_process_batch.  first_frame_num is the
 * server's frame counter of the first frame (flip parity, src/signal.cpp:160-168,223). */
int psdr_demod_batch(psdr_ctx *ctx, uint64_t first_frame_num);
/* same, but reading nframes spectra from a caller-supplied device buffer in the device layout of
 * psdr_spectrum_device_ptr() of an identically configured context (frame_stride_bins complex bins
 * between frames): used when the spectrum was produced on another GPU and received over xGMI
 * (SURVEY 8e). */
int psdr_demod_batch_from(psdr_ctx *ctx, const float *d_spec, size_t frame_stride_bins,
                          int nframes, uint64_t first_frame_num);
/* Band sharding (SURVEY 8e variant ii): a GPU that serves only the clients of one frequency band needs
 * only that band of the spectrum.  psdr_pack_band copies bins [first_bin, first_bin + nbins) - indexed
 * like the clients' l and r (IQ: client order, real: k), wrapping at the spectrum's end - of the first
 * nframes frames of the last batch out of the device layout into a linear device buffer (stream
 * ordered, no synchronisation): that is what is sent.  psdr_demod_batch_from_band is psdr_demod_batch_from
 * on such a buffer; every active client's [l, r) must lie inside the band (PSDR_ERR_INVALID names the
 * first that does not, and nothing is demodulated). */
int psdr_pack_band(psdr_ctx *ctx, int nframes, uint32_t first_bin, uint32_t nbins, float *d_out,
                   size_t out_stride_bins);
int psdr_demod_batch_from_band(psdr_ctx *ctx, const float *d_band, size_t frame_stride_bins, uint32_t first_bin,
                               uint32_t nbins, int nframes, uint64_t first_frame_num);
/* Band sharding WITHOUT the pack pass (2^20- and 2^21-point IQ contexts; PSDR_ERR_UNSUPPORTED otherwise - use
 * psdr_pack_band).
 * After psdr_set_band_layout(ctx, nbands, halo_bins) the second FFT pass writes the spectrum as nbands (a power of two,
 * <= 16) band REGIONS: region b holds bins [b*R/nbands, (b+1)*R/nbands + halo) - the halo, rounded up to whole
 * columns of M1 = N / 1024 bins, repeats the start of band b+1 - of ALL frames of the batch in one contiguous piece (frames
 * frame_stride_bins apart), in device order.  psdr_band_region gives the piece of the LAST processed batch: that is
 * what is sent to peer b, as it is.  Two result sets alternate from batch to batch (also on a caller's stream), so a
 * region stays valid until the batch after the next one is processed.  Everything else (demodulation, pyramid,
 * psdr_read_spectrum, psdr_pack_band) works unchanged on the root; psdr_spectrum_device_ptr does not (a frame is no
 * longer one piece).  Call before the first batch; reallocates the spectrum buffers.
 * psdr_demod_batch_from_band_region: psdr_demod_batch_from_band on a received region (an IQ context of the same size). */
int psdr_set_band_layout(psdr_ctx *ctx, int nbands, uint32_t halo_bins);
int psdr_band_region(psdr_ctx *ctx, int band, const float **d_region, size_t *frame_stride_bins, uint32_t *first_bin,
                     uint32_t *nbins);
int psdr_demod_batch_from_band_region(psdr_ctx *ctx, const float *d_region, size_t frame_stride_bins, uint32_t first_bin,
                                      uint32_t nbins, int nframes, uint64_t first_frame_num);
/* results of the last demod batch for one client: audio [nframes][n/2] floats (the
 * demodulated, overlap-added samples handed to the DC blocker at src/signal.cpp:278),
 * pwr [nframes] (average_power, src/signal.cpp:117-119), nan_flags [nframes] (1 = the
 * reference would have dropped the frame, src/signal.cpp:266-271).  Any may be NULL. */
/* nframes = rows the caller's buffers hold; it must be >= the frames of the last demod batch
 * (PSDR_ERR_INVALID otherwise, nothing is written); *nframes_out (may be NULL) = rows written. */
int psdr_read_audio(psdr_ctx *ctx, int id, int nframes, float *audio, float *pwr, int32_t *nan_flags,
                    int *nframes_out);
/* PSDR_IQ - the overlap-added complex baseband at the audio rate as the client's output (external decoders,
 * stereo / RDS; synchronous AM is a mode of its own, PSDR_SAM).  With n = audio_fft_size, h = n/2, frame f of an IQ client is h complex samples
 *   IQ_f[j] = s_f y_f[j] + s_{f-1} y_{f-1}[h + j],  j < h
 * y_f: the UN-NORMALISED n-point backward DFT of the AM / FM bin placement (src/signal.cpp:175-198, 214), s_f: the flip sign
 * of :223-234 - exactly what AM and FM detect (audio_complex_baseband after :235-237), interleaved re, im.  pwr is the
 * usual sum over [l, r); the NaN flag of a frame is 1 if any component of IQ_f is NaN; the state always moves and is AM's
 * and FM's (the tail, the last sample; the USB / LSB tail is kept), so a client may change between USB, LSB, AM, FM and IQ
 * at any batch boundary and every mode continues as if it had run all along (never reset, src/signal.cpp:81-94, 316-328).
 * A batch demodulated as IQ has NO audio and NO PCM: psdr_read_audio / psdr_read_pcm / psdr_fetched_audio /
 * psdr_fetched_pcm16 answer PSDR_ERR_NO_DATA for such a slot, and the IQ calls answer PSDR_ERR_NO_DATA for a slot whose
 * batch was not IQ.  To the post chain an IQ client is a paused one: its DC blocker and AGC stand still, and the AGC reset
 * of the mode command takes effect at its next audio batch.  Other clients are not affected by a bit.
 * psdr_read_iq: iq [nframes][n/2][2] floats (nframes * n in all), otherwise the contract of psdr_read_audio.
 * psdr_iq_device_ptr: the rows [frames][n/2][2] of slot `id` in the LAST batch's set of IQ rows (two sets alternate from
 * batch to batch: the pointer is good for that batch only; PSDR_ERR_NO_DATA before the context's first IQ client). */
int psdr_read_iq(psdr_ctx *ctx, int id, int nframes, float *iq, float *pwr, int32_t *nan_flags, int *nframes_out);
int psdr_iq_device_ptr(psdr_ctx *ctx, int id, const float **d_iq, const float **d_pwr);
/* PSDR_SAM - synchronous AM: detection against the recovered carrier instead of the envelope (at modulation index 1.5 the
 * envelope detector leaves a second harmonic at 0.23 of the fundamental, this one 1.3e-4).  A SAM client is an ordinary
 * AUDIO client - audio rows, pwr, NaN flags, the post chain (DC blocker, AGC, PCM / PCM16), read and fetched like an AM
 * client - only the detector differs.  With n = audio_fft_size, h = n/2, the AM / FM / IQ placement, flip sign s_f and
 * state:
 *   Baseband.  B_f[j] = s_f y_f[j] + s_{f-1} y_{f-1}[h + j] is the baseband AM detects, bit-identical to the PSDR_IQ rows of
 *     a client on the same window (same transform code, same operation order).
 *   Carrier transform.  c_f = the un-normalised n-point backward DFT of the same placed bins with indices
 *     [cutoff, n - cutoff) zeroed, cutoff = 500 * n / audio_rate in integer division (src/signal.cpp:217-220).  If
 *     2 * cutoff >= n nothing is zeroed (the reference's std::fill would be undefined there); if cutoff = 0 everything is.
 *   Carrier baseband.  C_f[j] = s_f c_f[j] + s_{f-1} c_{f-1}[h + j].
 *   Audio.  audio_f[j] = (B.re * C.re + B.im * C.im) / |C| at index j, |C| = sqrtf(C.re^2 + C.im^2); where |C| == 0,
 *     audio_f[j] = B.re (the phase reference is 1).  Every operation is a correctly rounded f32 one (no fast division, no
 *     fused product) in this order, and no batch split changes a bit.
 *   NaN flag.  1 if any audio sample of the frame is NaN; the state moves before the guard, as for AM / FM.
 *   State.  The AM / FM state (the tail, the last sample) moves exactly as in AM, the USB / LSB tail is copied through; the
 *     one new piece is the carrier tail s_f c_f[h..n), [2][slots][h] complex.  A slot that was not demodulated as SAM in its
 *     previous batch (a fresh slot; USB / LSB / AM / FM / IQ in between) starts from a ZERO carrier tail, not a stale one -
 *     only the phase of C is used, so this warm-up of one frame is benign.  A paused slot keeps everything frozen.  Switching
 *     among all six modes at batch boundaries leaves the other modes' streams continuous.
 *   Carrier record.  Per frame two floats, what a front end needs for a lock indicator and auto-tune:
 *     level = mean over j < h of |C_f[j]|;  offset_hz = audio_rate / (2 pi) * atan2f(Im S, Re S),
 *     S = sum over j < h - 1 of C[j+1] * conj(C[j]): positive when the carrier sits above the centre of bin
 *     floor(audio_mid), 0 when S = 0.
 * n = 360 / 720 run the transform's compile-time plan twice per frame, any other n (and PSDR_DEMOD_CHAIN=0) sums the kept
 * bins directly: the two paths may differ in the carrier's last bits, never in B.  The direct sum looks its twiddles up at
 * (bin * sample) mod n with a 32-bit product: PSDR_SAM is served for audio_fft_size < 65536 only, and
 * psdr_client_set_audio_demodulation answers PSDR_ERR_UNSUPPORTED for it above that (every other mode is served at any size).
 * psdr_read_carrier: level / offset_hz [nframes] (either may be NULL), otherwise the contract of psdr_read_audio;
 * PSDR_ERR_NO_DATA for a slot whose batch was not SAM.  psdr_fetched_carrier answers from the fetched set: a fetch that
 * carries audio, PCM or IQ also copies the carrier records, ONE extra copy of the span from the lowest to the highest SAM
 * slot of the batch. */
int psdr_read_carrier(psdr_ctx *ctx, int id, int nframes, float *level, float *offset_hz, int *nframes_out);
int psdr_fetched_carrier(psdr_ctx *ctx, int id, int frame, float *level, float *offset_hz);
/* Fine tuning below one FFT bin.  The kernels place a client's bins around m = floor(audio_mid), as the reference does: the
 * tuning grid is one bin of the main FFT (33 Hz at 35 MSPS and 2^20 points).  With the flag on, a client in mode USB, LSB or
 * IQ is a TUNED client: the fraction delta = audio_mid - m is taken out at the audio rate by a rotator behind the
 * overlap-add.  psdr_client_set_fine_tune may be called from any thread and takes force at the next batch; PSDR_ERR_INVALID
 * for an unknown id.  The default is 0 - the reference's behaviour and the launches of a library without this call, bit
 * for bit - or what psdr_set_option(ctx, PSDR_OPT_FINE_TUNE, 1) set before psdr_client_add (existing clients keep theirs).
 * A tuned client takes the tuned path whatever the fraction is, delta = 0 included: the path follows the flag, not the
 * value, so tuning across a bin boundary has no seam.  In AM, FM and SAM the flag is accepted and has NO effect - |B| and
 * Re(B conj C) / |C| are invariant under a rotation, and the constant it would add to FM sits below the DC blocker: those
 * clients' launches and bits are the untuned ones.  With n = audio_fft_size, h = n/2, s_f the flip sign:
 *   Step.  step = (uint32) floor(delta * 2^32 / n + 0.5), in double, from the batch's snapshot of audio_mid: one unit is
 *     2^-32 turn per audio sample (2.8e-6 Hz at 12 kHz); step < 2^30.
 *   Phase.  One uint32 per client, 0 at psdr_client_add.  Sample j of frame f of a batch has phi = phi0 + (f * h + j) * step
 *     in wrapping 32-bit arithmetic; a batch of F frames ends with phi0 += F * h * step.  The phase is continuous across
 *     frames, batches and changes of delta (a retune by a fraction does not click); a paused client keeps it, and so does
 *     a batch in which the client was not on the tuned path (flag off, or AM / FM / SAM).
 *   Rotator.  w(phi) = exp(-2 pi i phi / 2^32) in f32: a pure function of a frame's phi and step, correctly rounded f32
 *     operations in a fixed order (no fused contraction left to the compiler), the same device function in every kernel -
 *     no batch split and no choice of path changes a bit.
 *   Tuned IQ.  row_f[j] = B_f[j] * w(phi_{f,j}), B the PSDR_IQ row of the same window (bit-identical before the rotation).
 *     State is IQ's (the tail, the UN-rotated last sample; the USB / LSB tail copied through); rows, NaN flag (of the
 *     rotated row), psdr_read_iq, psdr_iq_device_ptr and PSDR_FETCH_IQ as for IQ; to the post chain a paused client.
 *   Tuned USB / LSB.  B' is the same baseband built from the window clipped to the sideband - [max(l, m), r) for USB,
 *     [l, min(r, m + 1)) for LSB - in the AM / FM placement (USB's bin m + k at index k, LSB's bin m - k at index n - k,
 *     k < h; no Nyquist bin): bit-identical to the PSDR_IQ row of a client on the clipped window.
 *     audio_f[j] = 2 Re(B'_f[j] w(phi_{f,j})): a bin at m + k comes out at k - delta bins of audio in USB, one at m - k at
 *     k + delta in LSB.  pwr stays the sum over the whole [l, r).  The NaN flag is 1 if any audio sample is NaN; the state
 *     moves before the guard (no frame is replayed).  State: a tail of its own, [2][slots][h] complex, allocated with the
 *     context's first tuned USB / LSB client (16 * (audio_fft_size/2) bytes per client slot; PSDR_ERR_NOMEM and the flag - or,
 *     from psdr_client_set_audio_demodulation, the mode - unchanged if that fails; a context that never sees one allocates
 *     nothing).  A client whose previous batch was not tuned in the same mode starts from a ZERO tail: its first frame fades
 *     in under the window's rising half.  The untuned USB / LSB tail, the AM / FM tail and last sample are copied through:
 *     every other mode continues behind a tuned stretch as if it had run all along.  To the post chain a tuned USB / LSB
 *     client is an ordinary audio client (DC blocker, AGC, PCM / PCM16), read and fetched like any other. */
int psdr_client_set_fine_tune(psdr_ctx *ctx, int id, int on);
/* Selectable-sideband synchronous AM.  A PSDR_SAM client detects both sidebands together against the recovered carrier; with
 * PSDR_SAM_UPPER or PSDR_SAM_LOWER it detects only that sideband against the SAME carrier, so an interferer that sits in the
 * other sideband (a heterodyne from the neighbouring channel, splatter) is gone from the audio.  The sideband is a setting
 * of the client beside its mode, not a mode: psdr_client_set_sam_sideband may be called from any thread and takes force at
 * the next batch; PSDR_ERR_INVALID for an unknown id or an unknown value.  The default is PSDR_SAM_BOTH - PSDR_SAM as defined
 * above, the launches and the bits of a library without this call - or what psdr_set_option(ctx, PSDR_OPT_SAM_SIDEBAND, v)
 * set before psdr_client_add (existing clients keep theirs).  In every mode other than PSDR_SAM the value is stored and has
 * NO effect; the fine-tune flag still has no effect on a SAM client, whatever its sideband.  There is no psdr_group_* call
 * (SAM is not served through a group).  With n = audio_fft_size, h = n/2, m = floor(audio_mid), s_f the flip sign:
 *   Carrier.  c_f, C_f, the carrier tail and the carrier record (level, offset_hz) are exactly PSDR_SAM's, built from the
 *     WHOLE window [l, r) with the same cutoff: bit-identical to a PSDR_SAM_BOTH client on the same window in the same
 *     batches.  A change of sideband at a batch boundary does not reset the carrier tail (it is zeroed only under PSDR_SAM's
 *     rule: the previous batch was not SAM).
 *   Baseband.  B'_f is the AM / FM placement of the window clipped to the sideband - [max(l, m), r) for PSDR_SAM_UPPER,
 *     [l, min(r, m + 1)) for PSDR_SAM_LOWER, the clipping rule of tuned USB / LSB - overlap-added from a tail of the client
 *     type's own: bit-identical to the PSDR_IQ row of a client on the clipped window with the same audio_mid (from the
 *     second frame after both start: both begin from a zero tail, IQ carries AM's).
 *   Audio.  audio_f[j] = 2 * ((B'.re * C.re + B'.im * C.im) / |C|) at index j, |C| = sqrtf(C.re^2 + C.im^2); where
 *     |C| == 0, audio_f[j] = 2 * B'.re.  Every operation is a correctly rounded f32 one in PSDR_SAM's order, the final
 *     doubling is exact; a modulation tone comes out at the amplitude PSDR_SAM_BOTH gives it.  No batch split changes a bit.
 *   pwr.  The sum over the whole [l, r).
 *   NaN flag.  1 if any audio sample of the frame is NaN; the state moves before the guard.
 *   State.  The tail of B', [2][slots][h] complex, is allocated with the context's first sideband SAM client - the first
 *     call that makes a client both PSDR_SAM and not PSDR_SAM_BOTH, whichever of the two calls comes second
 *     (16 * (audio_fft_size/2) bytes per client slot; PSDR_ERR_NOMEM and the sideband - or, from
 *     psdr_client_set_audio_demodulation, the mode - unchanged if that fails; a context that never sees one allocates
 *     nothing).  A slot whose previous batch was not SAM with the SAME sideband starts from a ZERO tail of B'.  The AM / FM
 *     tail and last sample and the USB / LSB tail are copied through: PSDR_SAM_BOTH and every other mode continue behind a
 *     sideband stretch from the state they had before it.  A paused slot keeps everything frozen.  To the post chain a
 *     sideband SAM client is an ordinary audio client; psdr_read_carrier, psdr_fetched_carrier and every audio / PCM read
 *     and fetch behave as for PSDR_SAM.
 * n = 360 / 720 run the transform's compile-time plan twice per frame (the carrier's slice, the sideband's slice), any
 * other n (and PSDR_DEMOD_CHAIN=0) transforms the clipped window and sums the carrier's kept bins directly: the two paths
 * differ as PSDR_SAM's own two do - in the carrier's last bits, never in B'. */
typedef enum psdr_sam_sideband { PSDR_SAM_BOTH = 0, PSDR_SAM_UPPER = 1, PSDR_SAM_LOWER = 2 } psdr_sam_sideband;
int psdr_client_set_sam_sideband(psdr_ctx *ctx, int id, int sideband);
/* Notch filters: manual and automatic heterodyne removal.  A steady carrier inside the wanted passband whistles through
 * every mode and captures the AGC.  A client's passband is held here as FFT bins, so a notch is exact: a NOTCH is a half-open
 * interval [first, end) of spectrum bins, in the coordinates of the client's l, r and audio_mid (client order for IQ input, k
 * for real input) - absolute, not relative to the window: it stays on the interferer when the listener retunes.  A client has
 * up to PSDR_NOTCH_MANUAL manual notches and up to PSDR_NOTCH_AUTO automatic ones.
 *   The defining rule.  A client with notches is bit-identical to the same client without notches on a spectrum in which
 *     every bin of every notch is +0.0 + 0.0i: audio, pwr, NaN flags, IQ rows, carrier records, every piece of carried state
 *     and the PCM behind the post chain; in every mode (tuned and sideband clients included), on both transform paths and
 *     for every batch split.  So pwr is the power of what is heard, and a NaN or Inf in a notched bin does not flag the frame:
 *     the kernels do not load a notched bin.  A client with no notch and auto-notch off gives the bits and the launches of
 *     a library without these calls; manual notches need no allocation of their own (they travel in the client
 *     parameter ring, which is 48 bytes per client slot and ring slot larger for them in every context).
 *   psdr_client_set_notch(ctx, id, index, centre_bin, width_bins): manual notch `index` (0 or 1) becomes
 *     first = floor(centre_bin - width_bins/2 + 0.5), end = floor(centre_bin + width_bins/2 + 0.5), computed in double, at
 *     least one bin (end = first + 1 if end <= first); width_bins <= 0 clears the entry.  PSDR_ERR_INVALID, and nothing
 *     changed, for an unknown id, an index outside 0..1, a non-finite argument or a width above audio_fft_size.  Any thread;
 *     takes force at the next batch, through the batch's snapshot, like psdr_client_set_audio_range.
 *   psdr_client_set_auto_notch(ctx, id, on): the detector.  Behind every batch one wave per auto-notch client adds the power
 *     |X|^2 of the client's window bins - un-notched: it keeps seeing a carrier it has removed - to a sum per bin, frame by
 *     frame; every period = max(1, audio_rate / audio_fft_size) frames (half a second) it evaluates and starts the sums
 *     again.  With mean = the sums' mean over the window: an automatic entry that is set stays while some bin of it is above
 *     8 * mean; a free entry takes the strongest bin t that is a local maximum (sum[t] >= sum[t-1], sum[t] > sum[t+1],
 *     outside the window 0) above 16 * mean, is not within 3 bins of floor(audio_mid) in PSDR_AM, PSDR_FM or PSDR_SAM (the
 *     wanted carrier) and whose entry [l + t - 1, l + t + 2) overlaps no set one; ties go to the lower bin.  Non-finite sums
 *     compare false: they set nothing and keep nothing.  A decision made behind batch b is in force from batch b + 1.  The
 *     sums, the frame counter and both entries start from zero when auto-notch is switched on (also while paused) and whenever [l, r),
 *     floor(audio_mid) or the mode differ from the client's previous batch; switching it off clears the entries; a paused
 *     client's stand still.  The state (4 * audio_fft_size + 20 bytes per client slot) is allocated with the context's
 *     first auto-notch client, all or none: PSDR_ERR_NOMEM and the flag unchanged if that fails.  The default is off, or what
 *     psdr_set_option(ctx, PSDR_OPT_AUTO_NOTCH, 1) set before psdr_client_add (existing clients keep theirs).
 *   psdr_read_notches(ctx, id, first, end): the last batch's notches of the client, entries 0..1 the manual ones of its
 *     snapshot, 2..3 the automatic ones as the batch's detector left them (in force from the next batch); an empty entry
 *     reads 0, 0.  Synchronises.  PSDR_ERR_NO_DATA under psdr_read_audio's rule (the client was not part of the last batch).
 * There is no psdr_group_* call: a group's clients have no notches. */
#define PSDR_NOTCH_MANUAL 2
#define PSDR_NOTCH_AUTO   2
int psdr_client_set_notch(psdr_ctx *ctx, int id, int index, double centre_bin, double width_bins);
int psdr_client_set_auto_notch(psdr_ctx *ctx, int id, int on);
int psdr_read_notches(psdr_ctx *ctx, int id, int first[4], int end[4]);
/* Squelch: a level gate per client, with hysteresis, attack and hang.  A client parked on a quiet channel costs the served
 * path what a client on a busy one costs, and the AGC pumps its noise up to full scale; a squelch-closed frame is to the post
 * chain what a NaN-flagged one is - no chain work, no PCM, nothing to encode or send.  The decision uses the frame's pwr, the
 * number the reference puts into every audio packet: the threshold is in the units of the S-meter.
 * With P_f the frame's pwr exactly as psdr_read_audio / psdr_read_iq deliver it (notches applied, any mode):
 *   Thresholds.  T_open = (float)pow(10.0, open_db / 10.0), computed in double and rounded once to f32; T_close the same
 *     from close_db.
 *   State per client, carried from frame to frame and batch to batch: open (0 / 1) and a run counter cnt (both int32).  For
 *     each frame of a batch, in order:
 *       closed:  above = (P_f >= T_open),   cnt = above ? cnt + 1 : 0;  if (cnt >= attack_frames) open = 1, cnt = 0
 *       open:    below = !(P_f >= T_close), cnt = below ? cnt + 1 : 0;  if (cnt > hang_frames)    open = 0, cnt = 0
 *     The frame's flag is `open` AFTER the update: the frame that completes the attack is heard, the frame that exhausts the
 *     hang is not.  NaN compares false both ways - it never opens, and it counts as below; +Inf is above.
 *   Start.  The state starts from (closed, 0) when squelch is switched ON for the client - while paused too, and for a fresh
 *     slot.  A change of thresholds or counts while on keeps the state and takes effect at the next batch, through the
 *     batch's snapshot.  A retune or a mode change does NOT reset it: the threshold is absolute, unlike the notch detector's
 *     (which is relative to the window's mean).  A paused client's state stands still.
 *   The demodulator is untouched.  Audio rows, IQ rows, pwr, NaN flags, carrier records and every piece of demodulation
 *     state are bit for bit those of the same client without squelch, in every client kind (USB, LSB, AM, FM, SAM, IQ,
 *     tuned, sideband SAM).
 *   The post chain treats a closed frame exactly as a NaN-flagged one: it is not part of the client's stream, the DC blocker
 *     and the AGC stand still across it, its PCM row (int32 or PCM16) is zero, and a batch that is closed throughout is an
 *     empty stream, as an all-NaN batch is.  Other clients are not affected by a bit.
 *   Nothing changes without squelch: a context with no squelch client launches and allocates exactly what a library
 *     without these calls does, and a batch with none hands the chain the NaN flags' own pointer.
 * psdr_client_set_squelch: any thread; in force from the client's next batch.  PSDR_ERR_INVALID, with nothing changed, for an
 *   unknown id, non-finite dB values or values outside [-300, 300], close_db > open_db, attack_frames outside 1..2^20 or
 *   hang_frames outside 0..2^20.  on = 0 ignores the other arguments.  The device state (flag rows, state, the batch's table:
 *   12 * max_batch + 200 bytes per client slot) is allocated with the context's first squelch client, all or none:
 *   PSDR_ERR_NOMEM and the setting unchanged if that fails.  There is deliberately NO PSDR_OPT_SQUELCH (it would be 8): an
 *   option hands psdr_client_add ONE value, and this setting has five.
 * psdr_read_squelch: open[nframes] (1 = heard), otherwise the contract of psdr_read_audio, for a client of any mode.  A
 *   client whose last batch ran with squelch off reads 1 for every frame - answered from the host snapshot, no device access.
 *   PSDR_ERR_NO_DATA under psdr_read_audio's rule.
 * psdr_fetched_squelch answers from the fetched set: a fetch (with any of the audio bits) of a batch that had squelch clients
 *   carries their flags as ONE extra copy, the span from the lowest to the highest squelch slot - the rule of the carrier
 *   records; keep squelch clients in neighbouring slots.  Squelch-off clients read 1.  Errors as psdr_fetched_audio, for a
 *   client of any mode.
 * There is no psdr_group_* call: a group's clients have no squelch. */
int psdr_client_set_squelch(psdr_ctx *ctx, int id, int on, double open_db, double close_db, int attack_frames, int hang_frames);
int psdr_read_squelch(psdr_ctx *ctx, int id, int nframes, int32_t *open, int *nframes_out);
int psdr_fetched_squelch(psdr_ctx *ctx, int id, int frame, int32_t *open);
/* Noise floor: the noise power of a client's window, frame by frame - the reference an S-meter needs for an SNR and a squelch
 * needs to be set in dB ABOVE THE NOISE (band noise moves by tens of dB over a day and from band to band; an absolute threshold is
 * wrong an hour later).  Only the device can estimate it: the full-resolution spectrum never leaves it.  Opt-in per client;
 * nothing changes for a client that does not ask for it.  For a noise-floor client with window [l, r), len = r - l, and
 * period = max(1, audio_rate / audio_fft_size) frames (the auto-notch detector's period):
 *   Bin power.  For window bin t of frame f: p = fmaf(re, re, im * im) of the raw spectrum bin l + t - un-notched, as the
 *     auto-notch detector takes it, indexed as l and r are, on every spectrum layout.
 *   Sums.  acc[t] += p, per bin, in frame order: the bits do not depend on how the stream is split into batches.
 *   Evaluation, every `period` frames the client takes part in: k = (len - 1) / 4 (integer division); q = the k-th smallest
 *     (0-based) of the len sums, ordered as unsigned 32-bit integers on the f32 bit pattern - numeric order for the non-negative
 *     sums, +Inf above every finite value, NaN above +Inf; the order is total, ties need no rule.  e = q / (float)period, one
 *     correctly rounded f32 division: the lower-quartile bin power per frame.  e goes into a ring of the last 8 evaluations; the
 *     sums restart from zero.
 *   Estimate.  m = +Inf; for each filled ring entry x: m = (x < m) ? x : m; n0 = (m < +Inf) ? m : 0.  A NaN or Inf entry is
 *     never the minimum; before the first evaluation, and when all 8 entries are non-finite, n0 = 0.
 *   Record.  W_f = n0 * (float)len, one f32 product, with n0 as it stands after frame f has been added and any evaluation it
 *     completes has run: the window's noise power in the units of pwr, so pwr_f / W_f is the SNR.  Any split of the same
 *     frames into batches gives the same W bits.
 *   What n0 is not: the mean noise power.  The quartile and the minimum over the ring (4 s) bias it BELOW the mean; for
 *     Gaussian noise the factor depends on `period`.  Thresholds and SNRs are relative to this number, not to the mean (the
 *     blanker's threshold is relative to its own reference level in the same way).
 *   State per client slot: the sums (audio_fft_size floats), the ring, its fill and position, the frame counter and the
 *     previous [l, r).  Everything starts from zero when the feature is switched ON for the client (also while paused) and
 *     whenever [l, r) differs from the client's previous batch.  A mode change, a change of audio_mid alone or a change of
 *     notches does NOT reset it.  A paused client's state stands still.  len <= 0: nothing is added, W_f = 0.
 *   Every client kind: USB, LSB, AM, FM, SAM, IQ, tuned, sideband SAM.  Audio rows, IQ rows, pwr, NaN flags, carrier records
 *     and every piece of demodulation state are bit for bit those of the same client without the feature.
 * psdr_client_set_noise_floor: any thread; in force from the client's next batch.  PSDR_ERR_INVALID for an unknown id, then
 *   PSDR_ERR_STATE if the context's audio_rate is not positive, then PSDR_ERR_STATE for on = 0 while the client's squelch
 *   reference is PSDR_SQ_NOISE; nothing changed in each case.  The device state (4 * audio_fft_size + 8 * max_batch + 176 bytes
 *   per client slot) is allocated with the context's first on = 1, all or none: PSDR_ERR_NOMEM and the setting unchanged if
 *   that fails.  A context that never has such a client allocates nothing, a batch without one launches nothing.
 * psdr_client_set_squelch_reference: what the squelch's thresholds (psdr_client_set_squelch) are relative to.
 *   PSDR_SQ_ABSOLUTE, the default: the squelch as described above, bit for bit.  PSDR_SQ_NOISE: the two comparisons of frame f
 *   are P_f >= T_open * W_f and P_f >= T_close * W_f, each threshold one f32 product - open_db and close_db keep their range
 *   and are dB above W; everything else of the gate (attack, hang, the post chain's view of a closed frame) stays.  W_f = 0 -
 *   before the first estimate, digital silence - lets any power that is not NaN compare at or above the threshold: the gate is
 *   open until there is an estimate.  PSDR_ERR_INVALID for an unknown id or value; PSDR_ERR_STATE for PSDR_SQ_NOISE on a client
 *   whose noise floor is off.  The gate's state is not reset by a change of reference.  Any thread; in force from the next batch.
 * psdr_read_noise: w[nframes], the W of every frame of the client's last batch, otherwise the contract of psdr_read_squelch.  A
 *   client whose last batch ran with the feature off reads 0 for every frame.  PSDR_ERR_NO_DATA under psdr_read_audio's rule.
 * psdr_fetched_noise answers from the fetched set: a fetch (with any of the audio bits) of a batch that had noise-floor clients
 *   carries their rows as ONE extra copy, the span from the lowest to the highest such slot - the rule of the squelch flags and
 *   the carrier records.  Clients without the feature read 0.  Errors as psdr_fetched_squelch.
 * There is no psdr_group_* call: a group's clients have no noise floor. */
enum { PSDR_SQ_ABSOLUTE = 0, PSDR_SQ_NOISE = 1 };
int psdr_client_set_noise_floor(psdr_ctx *ctx, int id, int on);
int psdr_client_set_squelch_reference(psdr_ctx *ctx, int id, int ref);
int psdr_read_noise(psdr_ctx *ctx, int id, int nframes, float *w, int *nframes_out);
int psdr_fetched_noise(psdr_ctx *ctx, int id, int frame, float *w);
/* Audio filter: a cascade of 1 or 2 biquad sections per client on the audio BEHIND the detector - the one place the window
 * [l, r) cannot reach: FM de-emphasis, a cut against a sub-audible tone, hum on an AM carrier, a CW peak filter.
 *   Form.  Each section is in transposed direct form II with two f32 states, from sample to sample:
 *       y = fma(b0, x, s1);  s1 = fma(b1, x, fma(-a1, y, s2));  s2 = fma(b2, x, -a2 * y)
 *     with the coefficients rounded once from double to f32, every operation a fused multiply-add or a lone multiply, subnormals
 *     kept.  The second section takes the first one's y.  The device evaluates a client's stream in blocks of 64 chunks of 16
 *     samples (a zero-state pass per chunk, a scan of the chunks' end states over the powers of the section's state matrix, a
 *     pass from the true entry state): a re-association of the recurrence above whose rounding differs from the sample-by-
 *     sample form by a few units in the last place; phantomsdr_amd/csrc/audiofilterplan.h is its one definition, for the
 *     device and for a host program alike, bit for bit.
 *   Who.  Every client of a batch whose kind writes audio rows: USB / LSB / AM / FM, SAM, sideband SAM, tuned USB / LSB.  A
 *     PSDR_IQ client (tuned or not) keeps its setting, is not filtered and its state stands still; a paused client's too.
 *   What.  A client's batch is the contiguous stream of nframes * audio_fft_size / 2 floats of its rows, filtered in place:
 *     psdr_read_audio, the fetches, psdr_audio_device_ptr and the post chain see filtered rows; pwr, NaN flags, carrier
 *     records and every piece of demodulation state are untouched.  A frame whose NaN flag is set enters the filter as zeros -
 *     the state advances, time passes - and its row is left exactly as the demodulator wrote it.  Frames the squelch closes
 *     are filtered like any others.
 *   State.  It starts from zero when psdr_client_set_audio_filter is called with nsections >= 1 - switching on, or new
 *     coefficients - and at no other time: a retune or a mode change does not reset it.
 * psdr_client_set_audio_filter: any thread; in force from the client's next batch; nsections = 0 switches it off and ignores
 *   `sections`.  PSDR_ERR_INVALID, with nothing changed, for an unknown id, nsections outside 0..2, a null pointer with
 *   nsections > 0, a non-finite coefficient, a section that is not stable (stable: |a2| < 1 and |a1| < 1 + a2) or one whose
 *   pole radius exceeds 0.9995 - in this order, each looked for in every section before the next.  Stability and the radius are
 *   those of the coefficients AS GIVEN, in double; the rounding to f32 moves 1 + a1 + a2 by 1.5e-7 at the most, less than the
 *   2.5e-7 two real poles at the limit leave, so an accepted section stays stable, with a pole up to 3e-4 past the limit.  The device state (16 bytes
 *   per client slot and the batches' table, 2176 bytes per slot) is allocated with the context's first filter client, all or
 *   none: PSDR_ERR_NOMEM and the setting unchanged if that fails.
 * psdr_audio_filter_design: needs no context.  The bilinear transform, in double, with K = tan(pi f0 / audio_rate):
 *   PSDR_AF_DEEMPHASIS  b0 = b1 = K / (1 + K), b2 = 0, a1 = (K - 1) / (K + 1), a2 = 0 (q ignored)
 *   with N = 1 / (1 + K / q + K^2), a1 = 2 (K^2 - 1) N, a2 = (1 - K / q + K^2) N:
 *   PSDR_AF_LOWPASS     b0 = b2 = K^2 N, b1 = 2 b0          PSDR_AF_HIGHPASS  b0 = b2 = N, b1 = -2 N
 *   PSDR_AF_PEAK        b0 = (K / q) N, b1 = 0, b2 = -b0
 *   PSDR_ERR_INVALID for an unknown kind, a null `out`, a rate or f0 that is not finite, f0 outside (0, audio_rate / 2), q <= 0
 *   or not finite (but for PSDR_AF_DEEMPHASIS), and for any result psdr_client_set_audio_filter would refuse.
 * There is no psdr_group_* call: a group's clients have no audio filter. */
#define PSDR_AUDIO_FILTER_SECTIONS 2
typedef struct { double b0, b1, b2, a1, a2; } psdr_biquad;   /* y = b0 x + b1 x[-1] + b2 x[-2] - a1 y[-1] - a2 y[-2] */
int psdr_client_set_audio_filter(psdr_ctx *ctx, int id, int nsections, const psdr_biquad *sections); /* 0: off */
#define PSDR_AF_DEEMPHASIS 0   /* first order low-pass, corner f0 (tau = 1 / (2 pi f0)); q ignored */
#define PSDR_AF_HIGHPASS   1
#define PSDR_AF_LOWPASS    2
#define PSDR_AF_PEAK       3   /* band-pass with 0 dB at f0, bandwidth f0 / q */
int psdr_audio_filter_design(int kind, double audio_rate, double f0, double q, psdr_biquad *out);    /* no context */
/* Noise reduction: a short-time spectral gain per client on the audio rows, BEHIND the detector and IN FRONT of the audio filter
 * and the post chain (a de-emphasis or a CW peak filter sees the cleaned audio).
 *   Rule.  The client's stream - its rows in frame order, a frame whose NaN flag is set entering as zeros - is cut into blocks of
 *     256 samples at a hop of 128.  A block is multiplied by the periodic square-root Hann window and transformed (256 points, 129
 *     bins).  Per bin and block, all in f32: the power P = re^2 + im^2; the smoothed power Ps += 0.5 (P - Ps); the noise track N,
 *     which follows a falling Ps with N += 0.25 (Ps - N) and a rising one with a time constant of 3 s at the context's audio_rate;
 *     the raw gain g = 1 - beta N / Ps (g_min where Ps <= 0), kept inside [g_min, 1], g_min = 10^(-depth_db / 20); the gain
 *     smoothed in time, G += 0.5 (g - G) where g > G and G += 0.25 (g - G) otherwise (the faster rise keeps speech onsets); and
 *     the applied gain (G[k-1] + 2 G[k] + G[k+1]) / 4 with the edge bins mirrored.  The stream's first block sets N = Ps = P and
 *     G = g.  A bin whose P is not finite leaves its Ps, N and G alone and is given g_min.  The block goes back through the
 *     inverse transform and the same window and is overlap-added.  phantomsdr_amd/csrc/nrplan.h is the one definition of all of
 *     it - windows, butterflies, operation order - for the device and for a host program alike, bit for bit.
 *     What the noise track cannot tell from noise: a power that stays.  A tone that lasts for seconds - a carrier, a long dash - is
 *     followed up with the 3 s time constant and reduced like noise (the notches are the tool for a carrier); speech and keying,
 *     shorter than that, keep their level.
 *   Delay.  Output sample i of the stream is the overlap-added sample i - 256: a fixed delay of 256 samples, whatever the batch
 *     lengths; the first 256 samples after a start from zero are +0.0.
 *   Who.  Every client of a batch whose kind writes audio rows: USB / LSB / AM / FM, SAM, sideband SAM, tuned USB / LSB.  A PSDR_IQ
 *     client is refused; a client that becomes one keeps its setting, is not listed and its state stands still; a paused
 *     client's too.
 *   What.  The rows are rewritten in place: psdr_read_audio, psdr_fetch_begin / psdr_fetch_end with the psdr_fetched_* calls,
 *     psdr_audio_device_ptr, the audio filter and the post chain read the reduced rows.  pwr, NaN flags, carrier records, squelch
 *     flags and noise records are untouched, and so is every piece of demodulation state.  The row of a flagged frame is left as
 *     the demodulator wrote it; output that falls on it is dropped.
 *   State.  3648 bytes per client slot.  It starts from zero when the call switches noise reduction on (again, too: new numbers
 *     start over), on a mode change and on a retune - whenever the mode, [l, r) or floor(audio_mid) are not those of the client's
 *     last batch with noise reduction.  It is carried across batches, pauses and dropped or flagged frames.
 * psdr_client_set_noise_reduction: any thread; in force from the client's next batch; on = 0 switches it off and ignores the
 *   numbers.  depth_db inside [0, 40], beta (the over-subtraction factor) inside [0.5, 4].  PSDR_ERR_INVALID, with nothing changed
 *   and a text of its own each, for an id outside the slots, a slot without a client, (on != 0) a PSDR_IQ client, a value that is not
 *   finite, depth_db outside its range, beta outside its range - in this order; PSDR_ERR_STATE for a context without a positive
 *   audio_rate.  The device state and tables are allocated with the context's first such client, all or none: PSDR_ERR_NOMEM and
 *   the setting unchanged if that fails.
 * psdr_noise_reduction_preset: needs no context.  PSDR_ERR_INVALID for an unknown kind or a null pointer.
 * There is no psdr_group_* call: a group's clients have no noise reduction. */
#define PSDR_NR_LIGHT  1   /* depth  8 dB, beta 1 */
#define PSDR_NR_NORMAL 2   /* depth 14 dB, beta 1.5 */
#define PSDR_NR_STRONG 3   /* depth 22 dB, beta 2 */
int psdr_client_set_noise_reduction(psdr_ctx *ctx, int id, int on, double depth_db, double beta);
int psdr_noise_reduction_preset(int kind, double *depth_db, double *beta);   /* needs no context */
/* Audio blanker: an impulse blanker per client on the audio rows, BEHIND the detector and IN FRONT of the noise reduction, the
 * audio filter and the post chain.  (psdr_ring_set_blanker is the wideband one on the ingest ring, one threshold for the whole
 * band; this one sees an impulse that is large inside one listener's window only, and is set per listener.)
 *   Rule.  The client's stream - its rows in frame order, a frame whose NaN flag is set entering as zeros, zeros before its start -
 *     is cut into blocks of 256 samples.  A block reads the INPUT samples of itself and of 24 samples on either side, never a
 *     repaired one, so every block is a function of the input alone.  All in f32: (1) the autocorrelation R[0..10] over the block,
 *     both factors of a product inside it; (2) Levinson-Durbin for the prediction-error filter a[0..10], a[0] = 1 - a block whose
 *     R[0] is not finite or not above 1e-20 has no detections; where the recursion's error stops being positive and finite the
 *     filter of the order before stands, the higher coefficients 0; (3) the residual e[n] = sum a[j] x[n - j] and the zero-phase
 *     matched filter m[n] = sum a[j] e[n + j]; (4) T = threshold * sqrt(var m), the mean-removed variance of m over the block,
 *     and no other factor; (5) n ascending, |m[n]| > T (strictly) makes n an impulse centre and the scan goes on at
 *     n + PL + 1, PL = (width - 1) / 2, at most 16 centres per block; (6) the gap [c - PL, c + PL] of centre c is replaced:
 *     the forward prediction f[i] = -sum a[j] f[i - j] from the 10 input samples in front of the gap, the backward one b[i] from
 *     the 10 behind it, gap sample i = (1 - w) f[i] + w b[i] with w = i / (width - 1), the f32 quotient, and 1 - w the f32
 *     difference; the block's own a also where the gap reaches into a neighbouring block; (7) a sample in more than one gap takes
 *     the value of the gap with the later centre, every other sample passes through.  phantomsdr_amd/csrc/anbplan.h is the one
 *     definition of all of it - the order of every sum included - for the device and for a host program alike, bit for bit.
 *   Delay.  Output sample i of the stream is processed sample i - 536 (two blocks and the 24 samples), whatever the batch lengths;
 *     the first 536 samples after a start from zero are +0.0.
 *   Who, What.  As the noise reduction: every client of a batch whose kind writes audio rows, a PSDR_IQ client is refused, a
 *     client that becomes one or is paused keeps its setting and its state stands still; the rows are rewritten in place and
 *     every later reader sees them; pwr, NaN flags, carrier, squelch and noise records are untouched; the row of a flagged frame
 *     is left as the demodulator wrote it.
 *   State.  6624 bytes per client slot: the last 824 input samples twice over (one half is read while the other is written), the
 *     position, two totals.  It starts from zero when the call
 *     switches the blanker on (again, too), on a mode change and on a retune, as the noise reduction's does.
 * psdr_client_set_audio_blanker: any thread; in force from the client's next batch; on = 0 switches it off and ignores the
 *   numbers.  threshold inside [2, 12], width odd in 3..15.  PSDR_ERR_INVALID, with nothing changed and a text of its own each, for
 *   an id outside the slots, a slot without a client, (on != 0) a PSDR_IQ client, a threshold that is not finite, threshold
 *   outside its range, a width that is not odd in 3..15 - in this order.  The device state is allocated with the context's first
 *   such client, all or none: PSDR_ERR_NOMEM and the setting unchanged if that fails.
 * psdr_audio_blanker_preset: needs no context.  PSDR_ERR_INVALID for an unknown kind or a null pointer.
 * psdr_read_audio_blanker: what an "NB active" indicator reads; synchronises.  impulses: the centres found, samples: the samples
 *   their gaps hold (a sample in two gaps counts twice; samples before the stream's start do not count), both over the blocks
 *   whose input is complete - block b once 256 (b + 1) + 24 samples are in - and cumulative since the state last started from
 *   zero.  PSDR_ERR_NO_DATA where psdr_read_audio has none - the client was not part of the last demodulation batch, or as
 *   PSDR_IQ - and for a client whose last batch ran without the blanker.  No per-frame record goes through psdr_fetch_*.
 * There is no psdr_group_* call: a group's clients have no audio blanker. */
#define PSDR_ANB_LIGHT  1   /* threshold 6,   width 5 */
#define PSDR_ANB_NORMAL 2   /* threshold 4.5, width 7 */
#define PSDR_ANB_STRONG 3   /* threshold 3.5, width 11 */
int psdr_client_set_audio_blanker(psdr_ctx *ctx, int id, int on, double threshold, int width);
int psdr_audio_blanker_preset(int kind, double *threshold, int *width);      /* needs no context */
int psdr_read_audio_blanker(psdr_ctx *ctx, int id, uint64_t *impulses, uint64_t *samples); /* cumulative since the state last started; synchronises */
/* Tone decoder: which sub-audible (CTCSS) tone a client's audio carries, per client on the audio rows, and a tone squelch: the
 * channel stays shut unless the transmission carries the right tone.  It READS the rows as the demodulator wrote them - in front
 * of the audio blanker, the noise reduction and the audio filter, which would damage or remove the tone - and never writes them.
 *   Tones.  The 50 standard tones, numbered 0..49 in ascending order, 67.0 Hz .. 254.1 Hz (psdr_tone_table).
 *   Rule.  The client's stream is its rows in frame order, a NaN-flagged frame entering as zeros, sample t counting from the state's
 *     start.  Tone k has the phase increment inc_k = round(f_k / audio_rate * 2^32), in double; the phase of sample t is the low 32
 *     bits of inc_k t, exact at any stream position.  Blocks hold 256 samples; block b gives per tone
 *     C[b][k] = sum_n x[256 b + n] conj(w_k(256 b + n)), n ascending in one f32 accumulator, where the twiddle w_k starts each block
 *     from two 4096-entry tables over bits 31..20 and 19..8 of the phase (computed in double, rounded once) and is turned once per
 *     sample by exp(2 pi i inc_k / 2^32).  The window is NB = ceil(0.4 audio_rate / 256) blocks (13 at 8 kHz, 19 at 12 kHz, 75 at
 *     48 kHz) with weights h_j = 0.5 - 0.5 cos(2 pi (j + 0.5) / NB); every block b >= NB - 1 gives S_k = sum_j h_j C[b - NB + 1 + j][k],
 *     j ascending, P_k = |S_k|^2, and a decision: best = the lowest k with the largest P_k; ref = the 12th smallest (0-based) of
 *     the 50 powers, ordered as unsigned integers on the f32 bit pattern; level = P_best * 4 / (256 sum h)^2, the squared amplitude
 *     of the tone in the units of the rows; hit = P_best >= ratio * ref && level >= min_level && (want < 0 || best == want) with
 *     ratio = (float)pow(10, snr_db / 10).  A power that is not finite gives no hit and level 0.  phantomsdr_amd/csrc/toneplan.h is
 *     the one definition of all of it - the order of every sum included - for the device and for a host program alike, bit for bit.
 *   Gate.  The squelch's state machine in units of blocks: closed, attack_blocks consecutive hits open it; open, more than
 *     hang_blocks consecutive misses close it; it starts at (closed, 0).
 *   Records.  Frame f's record is what stands behind the last block that is complete at the frame's last sample (block b once
 *     256 (b + 1) samples are in): tone = best if the last decision was a hit, else -1; level = the last decision's; open = the
 *     gate; before the first decision -1, 0, closed.  Any split of the same frames into batches gives the same bits.
 *   gate = 1.  With the post chain on, a frame whose record says closed stays out of the chain's stream like a NaN-flagged one
 *     (together with what the level squelch drops: nan | !squelch_open | !tone_open); rows, pwr, NaN flags, psdr_read_squelch's
 *     flags and every other state are those of a client without the decoder.  gate = 0: records only.
 *   Who.  Every client of a batch whose kind writes audio rows; a PSDR_IQ client is refused, a client that becomes one keeps its
 *     setting and is not listed.  The state is carried across batches and across dropped or flagged frames and stands still while
 *     the client is paused.
 *   State.  Per client slot 1048 bytes (the unfinished block's samples, the position, the gate, the last decision) and the block
 *     correlations of the last NB + 3 blocks, 512 bytes each (64 lanes' worth): 12.3 KB in all at 12 kHz, 41 KB at 48 kHz; 16 bytes per
 *     slot and frame of a batch for the records.  It starts from zero when the call switches the decoder on (again, too), on a mode
 *     change and on a retune, as the noise reduction's does.
 *   The default snr_db = 22 is a design constant between what tones in white noise reach and what noise alone reaches (DESIGN.md
 *     3.20); nobody has tried it on off-air FM audio.
 * psdr_client_set_tone_decoder: any thread; in force from the client's next batch; cfg = NULL switches it off.  PSDR_ERR_INVALID,
 *   with nothing changed and a text of its own each, for an id outside the slots, a slot without a client, (cfg != NULL) a PSDR_IQ
 *   client, want outside -1..49, gate outside 0..1, snr_db not finite or outside [6, 60], min_level not finite or below 0,
 *   attack_blocks outside 1..1024, hang_blocks outside 0..1024; then PSDR_ERR_STATE for a context whose audio_rate is outside
 *   [2000, 48000] (below, the top tone is not under Nyquist with room to spare; above, the window needs more than 75 blocks and the state per slot, 41 KB at 48 kHz, grows further) - in
 *   this order.  The device state is allocated with the context's first such client, all or none: PSDR_ERR_NOMEM and the setting
 *   unchanged if that fails.  A context without such a client allocates nothing, a batch without one launches nothing.
 * psdr_tone_defaults, psdr_tone_table: need no context.  PSDR_ERR_INVALID for a null pointer or an audio_rate outside [2000, 48000].
 * psdr_read_tone: psdr_read_squelch's contract - the records of the last demodulation batch, nframes the room of the arrays (any
 *   of which may be null), synchronises - but a client whose last batch ran without the decoder reads PSDR_ERR_NO_DATA, as does one
 *   that was not part of the batch or was demodulated as PSDR_IQ.
 * Nothing of it goes through psdr_fetch_* yet, and there is no psdr_group_* call: a group's clients have no tone decoder. */
#define PSDR_TONE_COUNT 50
#define PSDR_TONE_ANY (-1)
typedef struct {
    int want;          /* 0..49, or PSDR_TONE_ANY (-1) */
    int gate;          /* 1: a closed frame stays out of the post chain; 0: records only */
    double snr_db;     /* [6, 60], default 22 */
    double min_level;  /* >= 0, finite; default 0 */
    int attack_blocks; /* 1..1024, default 2 */
    int hang_blocks;   /* 0..1024, default NB */
} psdr_tone_config;
int psdr_tone_defaults(double audio_rate, psdr_tone_config *out);          /* needs no context */
int psdr_tone_table(const double **hz, int *n);                            /* needs no context */
int psdr_client_set_tone_decoder(psdr_ctx *ctx, int id, const psdr_tone_config *cfg);   /* NULL: off */
int psdr_read_tone(psdr_ctx *ctx, int id, int nframes, int32_t *tone, float *level, int32_t *open, int *nframes_out);
/* CW decoder: Morse text, speed and pitch of the signal a client's audio carries, per client on the audio rows.  It READS the rows
 * as the demodulator wrote them - the tone decoder's reading point: behind the squelch, in front of the audio blanker, the noise
 * reduction and the audio filter - and never writes them: every other output of the client is that of a client without it.
 *   Stream.  The client's rows in frame order, a NaN-flagged frame entering as zeros, sample t counting from the state's start.
 *   Hop.  H samples: 32 below audio_rate 8000, 64 below 16000, 128 below 32000, else 256 - 4 to 8 ms.
 *   Lanes.  Lane k = 0..63 listens at f_k = 250 + 25 k Hz.  Phase increment, the seed from the two 4096-entry tables at the exact
 *     32-bit phase of the hop's first sample, one rotation per sample and the single f32 accumulator are the tone decoder's, over
 *     H samples: C[b][k].  E[b][k] = |C[b][k] + C[b-1][k]|^2 (C[-1] = 0), a rectangular window of 2 H samples whose first nulls lie
 *     62 to 125 Hz off: lanes 25 Hz apart lose under 1 dB between them.  An E that is not finite enters as 0.
 *   Pitch.  A_k <- A_k + (E_k - A_k) / 64 per hop.  The candidates are the lanes with |f_k - pitch_hz| <= search_hz and always the
 *     lane nearest to pitch_hz (a tie goes up), where the followed lane p starts.  Behind the A update of a hop, q = the lowest
 *     candidate with the largest A (on the bit patterns); p becomes q only when A_q > 2 A_p.  e = E[b][p] with the new p.
 *   Levels.  hi <- max(e, hi - hi / 128); lo = the 16th smallest (0-based, ordered as unsigned integers on the f32 bit patterns) of
 *     the last 128 values of e.  The signal is present when 128 hops are in, hi is finite and above 0 (silence keys nothing) and hi >= ratio * lo with
 *     ratio = (float)pow(10, snr_db / 10).  Raw key = present && e >= hi / 4 - half the amplitude, so a mark reads as long as it was
 *     sent, to a hop.  For noise alone lo is 0.134 of the mean power and hi about 5 times the mean, some 16 dB apart; the
 *     default 22 dB means about 13 dB of signal over the mean noise in the window's bandwidth.  Nobody has tried it on off-air CW.
 *   Keying and timing, integers, in hops.  u is the dot length in 1/16 hop; it starts at round(16 * 1.2 / wpm * audio_rate / H) and
 *     stays inside what 40 and 10 WPM give.  A raw key change is taken once it has held g = max(1, u / 64) hops; the run it starts
 *     counts from its first hop, the run it ends stops in front of it.  A mark of len hops that ends is a dit if 16 len < 2 u, else
 *     a dah; the code starts at 1 and is shifted left, the low bit 1 for a dah; more than 7 elements stay "too long".  With
 *     track_speed, u <- u + floor((16 len - u) / 4) behind a dit and u + floor((floor(16 len / 3) - u) / 4) behind a dah.  When a
 *     space reaches 2 u the code's character is appended - the ITU-R M.1677 letters, figures and . , : ? ' - / ( ) " = + @, an
 *     unknown or too long code gives '*' -; when it reaches 5 u one ' ' is appended, once per gap and only behind a character.
 *   Records.  Frame f's record is the state behind the last hop that is complete at the frame's last sample: nchars = the text's
 *     length modulo 2^32, wpm = 1.2 audio_rate / (H u / 16), pitch_hz = f_p, level = hi / H^2 - the squared amplitude of a steady
 *     tone in the units of the rows -, key = the debounced key; before the first hop all zero but pitch_hz, the starting lane's.
 *     wpm and the scale are computed in double and rounded once.  Any split of the same frames into batches gives the same bits,
 *     records and text.  phantomsdr_amd/csrc/cwplan.h is the one definition of all of it, for the device and a host program alike.
 *   Who.  Every client of a batch whose kind writes audio rows; a PSDR_IQ client is refused, a client that becomes one keeps its
 *     setting and is not listed.  The state is carried across batches and across dropped or flagged frames and stands still while
 *     the client is paused.  It starts from zero when the call switches the decoder on (again, too), on a mode change and on a
 *     retune.  Per client slot 2352 bytes of state, 1024 bytes of text and 24 bytes per frame of a batch for the records.
 * psdr_client_set_cw_decoder: any thread; in force from the client's next batch; cfg = NULL switches it off.  PSDR_ERR_INVALID,
 *   with nothing changed and a text of its own each, for an id outside the slots, a slot without a client, (cfg != NULL) a PSDR_IQ
 *   client, pitch_hz outside [300, 1800], search_hz outside [0, 800], wpm outside [10, 40] (or any of them not finite),
 *   track_speed outside 0..1, snr_db not finite or outside [6, 40]; then PSDR_ERR_STATE for a context whose audio_rate is outside
 *   [4000, 48000] - in this order.  The device state is allocated with the context's first such client, all or none:
 *   PSDR_ERR_NOMEM and the setting unchanged if that fails.  A context without such a client allocates nothing, a batch without one
 *   launches nothing.
 * psdr_cw_defaults: needs no context.  PSDR_ERR_INVALID for a null pointer or an audio_rate outside [4000, 48000].
 * psdr_read_cw: psdr_read_tone's contract - the records of the last demodulation batch, nframes the room of the arrays (any of
 *   which may be null), synchronises; a client whose last batch ran without the decoder reads PSDR_ERR_NO_DATA, as does one that
 *   was not part of the batch or was demodulated as PSDR_IQ.
 * psdr_read_cw_text: characters from .. total - 1 of the client's text since the state last started - the first cap of them, cap
 *   being the room of out; no terminator is written -, their number in *n_out, total in *total_out (out with cap 0, n_out and
 *   total_out may be null); synchronises.  The device keeps the last 1024 characters per slot in a byte ring: a `from` older than
 *   that returns PSDR_ERR_NO_DATA; from == total returns PSDR_OK with 0 characters; from beyond total PSDR_ERR_INVALID.  A client
 *   without the decoder reads PSDR_ERR_NO_DATA; a start that is pending (the call came, no batch since) reads total 0.
 * Nothing of it goes through psdr_fetch_* yet, and there is no psdr_group_* call: a group's clients have no CW decoder. */
#define PSDR_CW_LANES 64
typedef struct {
    double pitch_hz;   /* [300, 1800], default 700: where the listener put the signal in the audio */
    double search_hz;  /* [0, 800], default 100: lanes within it may be followed; 0: the nearest lane only */
    double wpm;        /* [10, 40], default 20: the speed the dot length starts from */
    int track_speed;   /* 1 (default): the dot length follows the sender; 0: it stays at wpm */
    double snr_db;     /* [6, 40], default 22: keying is recognised only while peak >= ratio * floor */
} psdr_cw_config;
int psdr_cw_defaults(double audio_rate, psdr_cw_config *out);                 /* needs no context */
int psdr_client_set_cw_decoder(psdr_ctx *ctx, int id, const psdr_cw_config *cfg);   /* NULL: off */
int psdr_read_cw(psdr_ctx *ctx, int id, int nframes, uint32_t *nchars, float *wpm, float *pitch_hz, float *level, int32_t *key,
                 int *nframes_out);
int psdr_read_cw_text(psdr_ctx *ctx, int id, uint64_t from, char *out, size_t cap, size_t *n_out, uint64_t *total_out);
/* RTTY decoder: Baudot text and tuning offset of the radioteletype signal a client's audio carries, per client on the audio rows.
 * It READS the rows as the demodulator wrote them - the tone and CW decoders' reading point: behind the squelch, in front of the audio
 * blanker, the noise reduction and the audio filter - and never writes them: every other output of the client is that of a client
 * without it.
 *   Stream.  The client's rows in frame order, a NaN-flagged frame entering as zeros, sample t counting from the state's start.
 *   Hop.  H samples: 8 below audio_rate 8000, 16 below 16000, 32 below 32000, else 64 - 1 to 2 ms, 6.7 hops per bit at least.
 *   Lanes.  32 lanes in 16 pairs; pair j = 0..15 sits d_j = 20 (j - 8) Hz off the configured tones: lane 2 j listens at
 *     mark_hz + d_j, lane 2 j + 1 at mark_hz + shift_hz + d_j.  Phase increment round(f / audio_rate * 2^32) in double, the seed from
 *     the two 4096-entry tables at the exact 32-bit phase of the hop's first sample, one rotation per sample and the single f32
 *     accumulator, n ascending, are the tone decoder's, over H samples: C[b][k].  A signal half-way between two pairs loses 0.7 dB
 *     in a bit-long window at 45.45 baud.
 *   Bit window.  Wn = max(2, round(audio_rate / (baud H))) hops (7 to 22); S[b][k] = sum_{j < Wn} C[b - Wn + 1 + j][k], j ascending,
 *     hops before the start counting as 0, summed anew from the kept correlations every hop (no running sum: nothing drifts);
 *     E[b][k] = |S|^2, an E that is not finite entering as 0.
 *   Follower.  A_j <- A_j + ((E_2j + E_2j+1) - A_j) / 64 per hop.  The candidates are the pairs with |d_j| <= search_hz and always
 *     pair 8, where the followed pair p starts; q = the lowest candidate with the largest A (on the bit patterns); p becomes q only
 *     when A_q > 2 A_p.  m = E[2 p], s = E[2 p + 1] with the new p.
 *   Slicer with threshold correction.  pm = max(m, em - em / 256), ps = max(s, es - es / 256); em <- max(pm, ps / 16),
 *     es <- max(ps, pm / 16): a peak is held at 1/16 of the other at least, so that the tone that was not sent during a long idle
 *     is not sliced at its own leakage (without the floor the first start bit behind an idle of a second is taken half a bit
 *     early and the character is lost).  The bit is mark iff m es >= s em, in f32 products: a faded tone still slices at its own
 *     half, and silence reads as mark.
 *   Presence.  t = max(m, s), n = min(m, s); T <- T + (t - T) / 256, Nn <- Nn + (n - Nn) / 256.  The signal is present when 256
 *     hops are in, T is finite and above 0 and T >= ratio Nn, ratio = (float)pow(10, snr_db / 10).  line = present ? bit : mark:
 *     an absent signal is an idle line and prints nothing.  (Alternating bits keep the window across a transition all the time:
 *     T / Nn falls to 8 dB there at any signal-to-noise ratio; with a weight of 1/64 noise alone reached 8.3 dB within 60 s, with
 *     1/256 it stays under 6.4 dB - DESIGN.md 3.22.)
 *   Framing, integers in 1/16 hop.  u = round(16 audio_rate / (baud H)), in double.  When idle, a hop whose line is space directly
 *     behind a hop whose line is mark starts a character at t0 = 16 (that hop).  The sample points are c_i = t0 + floor(u / 2) + i u,
 *     i = 0..6, each read at the hop b with 16 b <= c_i < 16 (b + 1): i = 0 the start bit - mark there is a false start: back to
 *     idle, nothing counted -, i = 1..5 the data bits, least significant first, mark = 1, i = 6 the stop bit: mark and the code is
 *     taken, space and one framing error is counted and the code dropped.  Idle again from the hop behind the stop sample.  The
 *     window trails by half a bit, so the sample is the integral over the whole sent bit.
 *   Baudot.  ITA2 with the US-TTY figures.  Code 31 switches to letters, code 27 to figures, both print nothing, as does code 0;
 *     code 4 prints ' ' and with usos returns to letters; code 8 prints CR, code 2 LF, figures-S 0x07.  The state starts in letters.
 *   Records.  Frame f's record is the state behind the last hop that is complete at the frame's last sample: nchars = the text's
 *     length modulo 2^32, errors = the framing errors modulo 2^32, offset_hz = d_p, level = 4 max(em, es) / (Wn H)^2 - the squared
 *     amplitude of a steady tone in the units of the rows, the scale computed in double and rounded once -, quality = T / Nn as
 *     one f32 division, 0 when Nn is 0 or the quotient is not finite, present = the presence flag; before the first hop all zero.
 *     Any split of the same frames into batches gives the same bits, records and text.  phantomsdr_amd/csrc/rttyplan.h is the one
 *     definition of all of it, for the device and a host program alike.
 *   Who.  Every client of a batch whose kind writes audio rows; a PSDR_IQ client is refused, a client that becomes one keeps its
 *     setting and is not listed.  The state is carried across batches and across dropped or flagged frames (a flagged frame inside
 *     a transmission can cost the characters up to the next idle) and stands still while the client is paused.  It starts from
 *     zero when the call switches the decoder on (again, too), on a mode change and on a retune.  Per client slot 6536 bytes of
 *     state - the last 24 hops' correlations of the 32 lanes (6144), the unfinished hop (256), the followers (64), levels and
 *     framing (72) -, 1024 bytes of text and 24 bytes per frame of a batch for the records; 416 bytes per listed client in the
 *     batch's table.
 *   The default snr_db = 7.5 is measured on the host model: half-way between the 6.4 dB noise alone reaches in
 *     60 s and the 8.6 dB the quality keeps while the test text is read at 15 dB in the bit window's bandwidth, the lowest ratio
 *     in 3 dB steps at which it is read exactly.  Nobody has tried it on off-air RTTY.
 * psdr_client_set_rtty_decoder: any thread; in force from the client's next batch; cfg = NULL switches it off.  PSDR_ERR_INVALID,
 *   with nothing changed and a text of its own each, for an id outside the slots, a slot without a client, (cfg != NULL) a PSDR_IQ
 *   client, mark_hz outside [300, 3000], shift_hz of a magnitude outside [85, 1000], baud outside [45, 75] (or any of them not
 *   finite), usos outside 0..1, search_hz not finite or outside [0, 160], snr_db not finite or outside [3, 30]; then PSDR_ERR_STATE
 *   for a context whose audio_rate is outside [4000, 48000]; then PSDR_ERR_STATE when the higher tone + 160 Hz lies above
 *   0.45 audio_rate or the lower tone - 160 Hz below 100 Hz - in this order.  The device state is allocated with the context's
 *   first such client, all or none: PSDR_ERR_NOMEM and the setting unchanged if that fails.  A context without such a client
 *   allocates nothing, a batch without one launches nothing.
 * psdr_rtty_defaults: needs no context; mark_hz is 915 where 2125 + 170 + 160 Hz does not stay under 0.45 audio_rate.
 *   PSDR_ERR_INVALID for a null pointer or an audio_rate outside [4000, 48000].
 * psdr_read_rtty: psdr_read_cw's contract - the records of the last demodulation batch, nframes the room of the arrays (any of
 *   which may be null), synchronises; a client whose last batch ran without the decoder reads PSDR_ERR_NO_DATA, as does one that
 *   was not part of the batch or was demodulated as PSDR_IQ.
 * psdr_read_rtty_text: psdr_read_cw_text's contract to the letter: characters from .. total - 1 of the client's text since the state
 *   last started - the first cap of them, no terminator -, their number in *n_out, total in *total_out (out with cap 0, n_out and
 *   total_out may be null); synchronises.  The device keeps the last 1024 characters per slot: a `from` older than that returns
 *   PSDR_ERR_NO_DATA; from == total returns PSDR_OK with 0 characters; from beyond total PSDR_ERR_INVALID.  A client without the
 *   decoder reads PSDR_ERR_NO_DATA; a start that is pending (the call came, no batch since) reads total 0.
 * Nothing of it goes through psdr_fetch_* yet, and there is no psdr_group_* call: a group's clients have no RTTY decoder.  Out of
 * scope: the 100-baud SITOR-B / NAVTEX framing (its demodulator is this one; its 7-bit code and time diversity are not here) and
 * automatic detection of speed or shift. */
#define PSDR_RTTY_LANES 32
#define PSDR_RTTY_SNR_DEFAULT 7.5
typedef struct {
    double mark_hz;    /* [300, 3000], default 2125 (915 at an audio_rate that has no room for it): the mark tone in the audio */
    double shift_hz;   /* 85 <= |shift_hz| <= 1000, default 170: space = mark + shift; negative: the other sideband ("reverse") */
    double baud;       /* [45, 75], default 45.45 */
    int usos;          /* 1 (default): a space returns to letters (unshift on space); 0: it does not */
    double search_hz;  /* [0, 160], default 60: pairs within it may be followed; 0: the configured tones only */
    double snr_db;     /* [3, 30], default PSDR_RTTY_SNR_DEFAULT: the line is read only while T >= ratio * Nn */
} psdr_rtty_config;
int psdr_rtty_defaults(double audio_rate, psdr_rtty_config *out);               /* needs no context */
int psdr_client_set_rtty_decoder(psdr_ctx *ctx, int id, const psdr_rtty_config *cfg);   /* NULL: off */
int psdr_read_rtty(psdr_ctx *ctx, int id, int nframes, uint32_t *nchars, uint32_t *errors, float *offset_hz, float *level, float *quality,
                   int32_t *present, int *nframes_out);
int psdr_read_rtty_text(psdr_ctx *ctx, int id, uint64_t from, char *out, size_t cap, size_t *n_out, uint64_t *total_out);
/* PSK31 decoder: varicode text and tuning offset of the BPSK31 or BPSK63 signal a client's audio carries, per client on the audio
 * rows.  It READS the rows as the demodulator wrote them - the tone, CW and RTTY decoders' reading point: behind the squelch, in
 * front of the audio blanker, the noise reduction and the audio filter - and never writes them: every other output of the client is
 * that of a client without it.
 *   Stream, hop.  The RTTY decoder's: the client's rows in frame order, a NaN-flagged frame entering as zeros, sample t counting
 *     from the state's start; H = 8 samples below audio_rate 8000, 16 below 16000, 32 below 32000, else 64.
 *   Lanes.  16 lanes; lane j = 0..15 listens at carrier_hz + (j - 8) baud / 8: 3.90625 Hz apart at 31.25 baud, so a signal half-way
 *     between two lanes turns 22.5 degrees per symbol.  Phase increment round(f / audio_rate * 2^32) in double, the seed from the
 *     two 4096-entry tables at the exact 32-bit phase of the hop's first sample, one rotation per sample and the single f32
 *     accumulator, n ascending, are the tone decoder's, over H samples: C[b][j].
 *   Symbol window.  Wn = round(audio_rate / (baud H)) hops (8 to 32); S[b][j] = sum_{i < Wn} C[b - Wn + 1 + i][j], i ascending, hops
 *     before the start counting as 0, summed anew from the kept correlations every hop; E[b][j] = |S|^2, an E that is not finite
 *     entering as 0.
 *   Symbol clock, integers in 1/16 hop.  u = round(16 audio_rate / (baud H)), in double.  Every hop c <- (c + 16) mod u, from 0.
 *     Sixteen timing bins hold followers G_i; the hop's bin is floor(16 c / u) and G_bin <- G_bin + (T[b] - G_bin) / 32, T[b] the
 *     sum of the candidate lanes' E[b][j], j ascending (the followed lane's alone loses the clock on a lane that sits on one of the
 *     idle's two tones: DESIGN.md 3.23).  g = the lowest bin with the largest G (on the bit patterns), tau = floor(g u / 16).  The
 *     hop is a sample point when ((c - tau) mod u) < floor(u / 2) - the clock is within half a symbol behind tau - and
 *     floor(3 u / 4) at least has passed since the last sample point (counted in steps of 16 from 0 at the start).  The dips of the
 *     phase reversals make E peak where the window covers one whole symbol; a steady carrier leaves the bins level and g where
 *     it was.
 *   Differential detection, at a sample point, every lane: d_j = S_j conj(prev_j), then prev_j <- S_j; Re q_j = (Re d_j)^2 -
 *     (Im d_j)^2 - the square takes the keying out - and |d_j|^2, either entering as 0 when it is not finite;
 *     Qre_j <- Qre_j + (Re q_j - Qre_j) / 32.
 *   Carrier follower.  M_j = max(Qre_j, +0): a lane 3.9 Hz off turns q by 90 degrees and reads 0, one 2 Hz off reads 0.7 - the
 *     energy alone would differ by 0.2 dB.  The candidates are the lanes with |(j - 8) baud / 8| <= search_hz and always lane 8,
 *     where the followed lane p starts; q = the lowest candidate with the largest M (on the bit patterns); p becomes q only when
 *     M_q > 2 M_p, and a move clears the shift register.  search_hz stays below baud / 2: a lane half the baud rate off sees the same q - the false lock every PSK31
 *     program knows - and nothing here could tell the two apart.
 *   Presence.  A symbol's own coherence is Re q_p / |d_p|^2 as one f32 division, 0 when |d_p|^2 is 0 or the quotient is not
 *     finite: the cosine of twice its turn.  coherence <- coherence + (it - coherence) / 32 per sample point, with the new p: near
 *     1 for a clean signal, scattered about 0 for noise.  The signal is present when 32 sample points are in and
 *     coherence >= quality.  (The quotient of two energy-weighted followers reached 0.70 on noise alone: DESIGN.md 3.23.)
 *   Bit and varicode.  bit = Re d_p >= 0 ? 1 : 0 - a reversal is 0.  While the signal is absent nothing is shifted and the register
 *     is cleared: an absent signal prints nothing.  Else sr <- sr << 1 | bit; when its low two bits are 00, code = sr >> 2 and
 *     sr <- 0: code 0 is nothing, a code of G3PLX's 128-entry table appends its character (NUL is dropped), any other code counts
 *     one error.  A register that passes 12 bits without 00 is cleared and counts one error - unless it holds ones only: that is
 *     the steady carrier behind a transmission, which is no fault of the line.
 *   Records.  Frame f's record is the state behind the last hop that is complete at the frame's last sample: nchars = the text's
 *     length modulo 2^32, errors modulo 2^32, offset_hz = (p - 8) baud / 8, level = 4 A / (Wn H)^2 with A <- A + (E[b][p] - A) / 32
 *     per sample point - the squared amplitude of a steady carrier in the units of the rows, the scale computed in double and
 *     rounded once; idle reversals read (2 / pi)^2 of theirs -, quality = the coherence as of the last sample point, present = the presence flag; before the first hop all zero.
 *     Any split of the same frames into batches gives the same bits, records and text.  phantomsdr_amd/csrc/pskplan.h is the one
 *     definition of all of it, for the device and a host program alike.
 *   Who.  Every client of a batch whose kind writes audio rows; a PSDR_IQ client is refused, a client that becomes one keeps its
 *     setting and is not listed.  The state is carried across batches and across dropped or flagged frames and stands still while
 *     the client is paused.  It starts from zero when the call switches the decoder on (again, too), on a mode change and on a
 *     retune.  Per client slot 4664 bytes of state - the last 32 hops' correlations of the 16 lanes (4096), the unfinished hop
 *     (256), prev, Qre and the bins (256), clock and register (56) -, 1024 bytes of text and 24 bytes per frame of a batch for
 *     the records; 224 bytes per listed client in the batch's table.
 *   The default quality is measured on the host model: half-way between the largest coherence noise alone
 *     reaches in 60 s and the smallest it keeps while the test text is read at the lowest ratio, in 3 dB steps, at which it is
 *     read exactly: 0.405, 0.616 at 12 dB in a bandwidth equal to the baud rate, 0.51.  Behind the end of a signal the coherence
 *     needs some twenty symbols to fall under that: a transmission that ends without its carrier tail can print noise
 *     meanwhile.  Nobody has tried it on off-air PSK31.
 * psdr_client_set_psk_decoder: any thread; in force from the client's next batch; cfg = NULL switches it off.  PSDR_ERR_INVALID,
 *   with nothing changed and a text of its own each, for an id outside the slots, a slot without a client, (cfg != NULL) a PSDR_IQ
 *   client, carrier_hz not finite or outside [300, 3000], a baud that is neither 31.25 nor 62.5, search_hz not finite or outside
 *   [0, baud / 2), quality not finite or outside (0, 1); then PSDR_ERR_STATE for a context whose audio_rate is outside
 *   [4000, 48000]; then PSDR_ERR_STATE when lane 15 lies above 0.45 audio_rate or lane 0 below 100 Hz - in this order.  The device
 *   state is allocated with the context's first such client, all or none: PSDR_ERR_NOMEM and the setting unchanged if that fails.
 *   A context without such a client allocates nothing, a batch without one launches nothing.
 * psdr_psk_defaults: needs no context; 1000 Hz, 31.25 baud, three lanes to either side (11.71875 Hz), the measured quality.
 *   PSDR_ERR_INVALID for a null pointer or an audio_rate outside [4000, 48000].
 * psdr_read_psk: psdr_read_rtty's contract - the records of the last demodulation batch, nframes the room of the arrays (any of
 *   which may be null), synchronises; a client whose last batch ran without the decoder reads PSDR_ERR_NO_DATA, as does one that
 *   was not part of the batch or was demodulated as PSDR_IQ.
 * psdr_read_psk_text: psdr_read_rtty_text's contract to the letter; the device keeps the last 1024 characters per slot.
 * Nothing of it goes through psdr_fetch_* yet, and there is no psdr_group_* call: a group's clients have no PSK decoder.  Out of
 * scope: QPSK31 (it needs a Viterbi decoder), PSK125 and automatic detection of the speed. */
#define PSDR_PSK_LANES 16
#define PSDR_PSK_QUALITY_DEFAULT 0.51
typedef struct {
    double carrier_hz;  /* [300, 3000], default 1000: where the listener put the signal in the audio */
    double baud;        /* 31.25 (default) or 62.5, nothing else */
    double search_hz;   /* [0, baud / 2), default 3 baud / 8: lanes within it may be followed; 0: the configured carrier only */
    double quality;     /* (0, 1), default PSDR_PSK_QUALITY_DEFAULT: the line is read only while coherence >= quality */
} psdr_psk_config;
int psdr_psk_defaults(double audio_rate, psdr_psk_config *out);               /* needs no context */
int psdr_client_set_psk_decoder(psdr_ctx *ctx, int id, const psdr_psk_config *cfg);   /* NULL: off */
int psdr_read_psk(psdr_ctx *ctx, int id, int nframes, uint32_t *nchars, uint32_t *errors, float *offset_hz, float *level, float *quality,
                  int32_t *present, int *nframes_out);
int psdr_read_psk_text(psdr_ctx *ctx, int id, uint64_t from, char *out, size_t cap, size_t *n_out, uint64_t *total_out);
/* Radiofax (WEFAX) decoder: the image lines of the HF facsimile a client's audio carries - black 1500 Hz, white 2300 Hz in USB
 * audio, 120 lines per minute as the weather services send it -, per client on the audio rows.  It READS the rows as the
 * demodulator wrote them - the tone, CW, RTTY and PSK decoders' reading point: behind the squelch, in front of the audio blanker,
 * the noise reduction and the audio filter - and never writes them: every other output of the client is that of a client without it.
 *   Stream, hop.  The other decoders': the client's rows in frame order, a NaN-flagged frame entering as zeros, sample t counting
 *     from the state's start; H = 8 samples below audio_rate 8000, 16 below 16000, 32 below 32000, else 64.
 *   Discriminator, per sample.  z[t] = x[t] conj(w[t]); w turns at centre_hz = (black_hz + white_hz) / 2: phase increment
 *     round(centre_hz / audio_rate * 2^32) in double, the seed from the two 4096-entry tables at the exact 32-bit phase of the hop's
 *     first sample and one rotation per sample are the tone decoder's.  y[t] = sum_{i < K} z[t - i], i ascending from +0,
 *     K = max(2, round(audio_rate / (2 centre_hz))), samples before the start counting as 0: the boxcar's first null sits on the
 *     mixing image.  d[t] = y[t] conj(y[t - D]), D = max(1, floor(audio_rate / 3200)).  a[t] = fax_angle(d): ONE f32 division, of
 *     the smaller of |Im d| and Re d by the larger (the quotient, in [-1, 1], clamped to it), an odd polynomial of degree 17 in fmaf
 *     form with literal coefficients (Abramowitz and Stegun 4.4.49) and, where Im was the larger, +-pi/2 minus it; a d with
 *     Re <= 0 or one that is not finite saturates at +-pi/2 by the sign of Im, a zero d reads 0.  (A clamped tangent Im / Re cannot
 *     reach the +-pi/2 that a shift of 1600 Hz needs at a rate that is a multiple of 3200: DESIGN.md 3.24.)
 *     v[t] = clamp(0.5 + a[t] s, 0, 1), s = audio_rate / (2 pi D (white_hz - black_hz)) in double, rounded once: 0 is black, 1 is
 *     white, and a white_hz below black_hz inverts the picture.
 *   Line and column, integers.  Lq = round(65536 * 60 audio_rate / lpm * (1 + slant_ppm 1e-6)) in double, held as 64 bits: the
 *     line in 1/65536 sample.  Sample t lies in line floor((65536 t + Lq - origin) / Lq) - 1 and in column
 *     floor(((65536 t + Lq - origin) mod Lq) width / Lq); origin, in [0, Lq), starts as phase_col Lq / width and is moved only by
 *     the phasing, with the next line boundary.  The samples in front of the first origin and behind a move are a partial line,
 *     which is never looked at.  A pixel is the sum of its samples' v (t ascending, one f32 accumulator) divided by their count
 *     (one f32 division) as min(255, floor(255 p + 0.5)); the call makes sure that a pixel has 1 to 64 samples.  A line is
 *     complete with the first sample of the next one.
 *   Tones, on v, PSDR_FAX_AUTO only.  Per hop C_k = sum (v - 0.5) conj(w_k) for 300, 450 and 675 Hz (the tone decoder's seed,
 *     rotation and single accumulator), Q = sum (v - 0.5)^2, M = sum (v - 0.5).  Blocks of NB = round(audio_rate / (8 H)) hops
 *     (1/8 s) do not overlap; at a block's end rho_k = 2 |sum C_k|^2 / (NB H sum Q), 0 when not finite; tone k hits when it is
 *     the (lowest) largest of the three and rho_k >= tone_ratio.  One counter per tone: + 1 in a block it hits, - 1 in any other,
 *     held in [0, 2 start_blocks].
 *   Machine.  IDLE -> PHASING when the 300 Hz counter (IOC 576) or the 675 Hz counter (IOC 288) reaches start_blocks: the image's
 *     serial goes up by one, the IOC is noted, the counters are cleared.  Any state -> IDLE when the 450 Hz counter reaches
 *     start_blocks (looked at first; the counters are cleared).  In PHASING every complete line is searched for the narrow pulse
 *     of either polarity: a line whose pixels sum to 255 width / 2 or more has a dark pulse and is measured as 255 - pix, else as
 *     pix; dev(c) = the sum over wp = max(1, width / 20) circular columns from c, c* the lowest column with the largest dev; the
 *     line is valid when dev(c*) >= 192 wp and the rest of it sums to 64 (width - wp) at most.  A valid line within width / 64
 *     columns, circularly, of the previous valid line's c* extends a run, any other starts it over; when the run reaches
 *     phase_lines the origin moves on by ((c* + wp / 2) mod width) Lq / width - the pulse's middle becomes column 0 - and the
 *     state is IMAGE; after 80 lines without that it is IMAGE with the origin as it stands.  In IMAGE every complete line is
 *     kept; behind max_lines of them (0: no limit) the state is IDLE.  PSDR_FAX_FREE: no tones, no phasing, IMAGE from sample 0.
 *   Kept lines.  A ring of R lines of width bytes per slot, each with 32 bits of meta: the image's serial << 8 | the state in
 *     which it was taken.  R = max(64, 2 + the lines the context's largest batch can complete, floor(samples 65536 / Lq) + 1), fixed by the call.
 *   Records.  Frame f's record is the state behind the last hop that is complete at the frame's last sample: nlines = the kept
 *     lines modulo 2^32, state (0 IDLE, 1 PHASING, 2 IMAGE), image = the serial, ioc (0 before the first start tone),
 *     offset_hz = (white_hz - black_hz) F with F <- F + (sum M / (NB H) - F) / 8 in the blocks with a hit - a start or stop tone
 *     is symmetric about the centre, so this is the listener's mistuning; it is reported only -, tone_quality = the last block's
 *     largest rho.  Any split of the same frames into batches gives the same bits in records, lines and meta.
 *     phantomsdr_amd/csrc/faxplan.h is the one definition of all of it, for the device and a host program alike.
 *   Who.  Every client of a batch whose kind writes audio rows; a PSDR_IQ client is refused, a client that becomes one keeps its
 *     setting and is not listed.  The state is carried across batches and across dropped or flagged frames and stands still while
 *     the client is paused.  It starts from zero when the call switches the decoder on (again, too), on a mode change and on a
 *     retune.  Per client slot 3224 bytes of state, the ring (2048 bytes per line the context's largest batch can complete at 240
 *     lines per minute, 64 lines at least), 24 bytes per frame of a batch for the records; 128 bytes per listed client in the
 *     batch's table.
 *   The default tone_ratio is the middle between two figures of the host model: the largest rho unit noise alone
 *     reaches in 120 s, 0.0184, and the smallest a start tone keeps at the lowest signal-to-noise ratio, in 3 dB steps, at which
 *     the test sequence still locks, 0.425 at 6 dB in 3 kHz: 0.22.  Nobody has tried it on off-air radiofax.
 * psdr_client_set_fax_decoder: any thread; in force from the client's next batch; cfg = NULL switches it off.  PSDR_ERR_INVALID,
 *   with nothing changed and a text of its own each, for an id outside the slots, a slot without a client, (cfg != NULL) a PSDR_IQ
 *   client, then the fields in their order: a mode that is neither, black_hz or white_hz not finite or outside [300, 3400] or
 *   |white_hz - black_hz| outside [200, 1600], an lpm that is none of 60, 90, 120, 240, width outside [256, 2048], slant_ppm not
 *   finite or outside [-2000, 2000], phase_col outside [0, width), tone_ratio not finite or outside (0, 1), start_blocks outside
 *   [2, 64], phase_lines outside [2, 32], max_lines below 0; then PSDR_ERR_STATE for a context whose audio_rate is outside
 *   [4000, 48000]; then PSDR_ERR_STATE when the higher tone plus 300 Hz lies above 0.45 audio_rate; then PSDR_ERR_STATE when a
 *   pixel would hold fewer than 1 or more than 64 samples - in this order.  The device state is allocated with the context's first
 *   such client, all or none: PSDR_ERR_NOMEM and the setting unchanged if that fails.  A context without such a client allocates
 *   nothing, a batch without one launches nothing.
 * psdr_fax_defaults: needs no context; the values in the struct's comments.  PSDR_ERR_INVALID for a null pointer or an audio_rate
 *   outside [4000, 48000].  (Below 5778 Hz the default tones do not fit: the call says so.)
 * psdr_read_fax: psdr_read_psk's contract - the records of the last demodulation batch, nframes the room of the arrays (any of
 *   which may be null), synchronises; a client whose last batch ran without the decoder reads PSDR_ERR_NO_DATA, as does one that
 *   was not part of the batch or was demodulated as PSDR_IQ.
 * psdr_read_fax_lines: psdr_read_psk_text's contract with a line in place of a character: the kept lines from .. total - 1 since
 *   the state last started, cap_lines at most, width bytes each into pix and one meta word each into meta (either may be null when
 *   cap_lines is 0); a from beyond total is PSDR_ERR_INVALID, one older than the ring's R lines PSDR_ERR_NO_DATA; total_out counts
 *   every kept line, width_out is the client's width.
 * Nothing of it goes through psdr_fetch_* yet, and there is no psdr_group_* call: a group's clients have no fax decoder.  Out of
 * scope: applying offset_hz (AFC), automatic slant correction, colour fax and SSTV. */
#define PSDR_FAX_AUTO 0
#define PSDR_FAX_FREE 1
#define PSDR_FAX_TONE_RATIO_DEFAULT 0.22
typedef struct {
    int    mode;         /* PSDR_FAX_AUTO (default) | PSDR_FAX_FREE */
    double black_hz, white_hz;   /* each in [300, 3400], |white-black| in [200, 1600]; 1500 / 2300 */
    double lpm;          /* 60, 90, 120 (default) or 240 */
    int    width;        /* pixels per line, [256, 2048], default 1024 */
    double slant_ppm;    /* [-2000, 2000], default 0 */
    int    phase_col;    /* [0, width), default 0 */
    double tone_ratio;   /* (0, 1), default PSDR_FAX_TONE_RATIO_DEFAULT (measured, above) */
    int    start_blocks; /* [2, 64], default 8 (1 s) */
    int    phase_lines;  /* [2, 32], default 4 */
    int    max_lines;    /* >= 0, default 0 */
} psdr_fax_config;
int psdr_fax_defaults(double audio_rate, psdr_fax_config *out);               /* needs no context */
int psdr_client_set_fax_decoder(psdr_ctx *ctx, int id, const psdr_fax_config *cfg);   /* NULL: off */
int psdr_read_fax(psdr_ctx *ctx, int id, int nframes, uint32_t *nlines, int32_t *state, uint32_t *image, int32_t *ioc,
                  float *offset_hz, float *tone_quality, int *nframes_out);
int psdr_read_fax_lines(psdr_ctx *ctx, int id, uint64_t from, uint8_t *pix, uint32_t *meta, size_t cap_lines,
                        size_t *n_out, uint64_t *total_out, int *width_out);
/* AGC profile: speed, target, gain cap and manual gain per client.  The context's AGC is the reference's - target 0.2, attack
 * 50 ms, release 300 ms (psdr_set_post_chain) - for every client; a profile replaces these numbers for one client: a fast AGC for
 * CW, a slow one for broadcast, a bound on the gain a quiet channel is pumped up by, or no AGC at all and a fixed gain, which is
 * what a digital-mode decoder behind the PCM needs.
 *   The rule.  The reference's recurrence (src/utils/audioprocessing.cpp:40-66), every quantity and every operation as it is:
 *     peak_t the maximum of |x| over the look-ahead window, the gain step g <- g + (w_t < g ? att : rel) * (w_t - g), the output
 *     the sample delayed by L - 1 times g, zeros while the look-ahead fills.  Three things are the client's own, in f32:
 *       att = (float)(1 - exp((double)(-1.0f / ((float)attack_ms * 0.001f * sr)))), sr = (float)audio_rate, exp in double;
 *       rel   the same expression from release_ms - for 50 and 300 ms these are the context's own coefficients;
 *       w_t = manual ? (float)manual_gain : fminf((float)desired / (peak_t + 1e-10f), cap),
 *             cap = max_gain > 0 ? (float)max_gain : +Inf (fminf against +Inf is the identity);
 *     each operation rounded once, nothing contracted; phantomsdr_amd/csrc/agcplan.h is the one definition of w_t, for the device
 *     and for a host program alike.  In manual mode the gain therefore GLIDES from wherever the AGC left it to manual_gain with
 *     the profile's own time constants and then stays: no click, and no time shift - the look-ahead's delay of L - 1 samples
 *     stays.  The step moves g only while |c (w_t - g)| is at least half a unit in the last place of g, so the gain comes to
 *     rest within 1 / (2 c) such units of manual_gain (c = att or rel): exactly on it for c > 0.5, within 600 units for a 100 ms
 *     release at 12 kHz.  A gain that climbs to the cap rests below it by the same rule.
 *   What does not move.  The look-ahead (200 ms), the DC blocker and the int16 conversion stay the context's.  A profile change
 *     resets nothing: the gain, the look-ahead's fill count and the DC sums carry on, and AGC::reset remains what
 *     psdr_client_set_audio_demodulation alone triggers.  Dropped, squelch-closed and paused frames are handled as before.  A
 *     client with the profile {0.2, 50, 300, 0, 0, -} gives the bits of a client without one; other clients of the batch are not
 *     affected by a bit; and a context in which no client ever had a profile allocates, uploads and launches exactly what a
 *     library without these calls does.  An IQ client keeps its setting, which has no effect while the client is IQ.
 * psdr_client_set_agc_profile: any thread; in force from the client's next batch, through the batch's snapshot (batches in
 *   flight keep theirs: the chain runs up to three steps behind).  p = NULL: back to the context's AGC.  PSDR_ERR_INVALID, with
 *   nothing changed, for an unknown id, a non-finite field (manual_gain is read only when manual = 1), desired outside (0, 1], a
 *   time outside (0, 10000] ms, max_gain < 0, manual outside 0..1, manual_gain < 0 - in this order - and at last for a computed
 *   att < rel: the gain step picks between its two candidates by min / max, which is the reference's pick only while attack is
 *   at least as fast as release, as the context's own is.  PSDR_ERR_STATE if the context's audio_rate is not positive.  The
 *   batches' table (256 bytes per client slot) is allocated with the context's first profile, all or none: PSDR_ERR_NOMEM and the
 *   setting unchanged if that fails.
 * psdr_agc_preset: needs no context.  PSDR_ERR_INVALID for an unknown kind or a null `out`.
 * psdr_read_agc_gain: the gain the client's last chain batch left behind, the one its next batch starts from; synchronises.  A
 *   paused client's stands still.  PSDR_ERR_STATE before psdr_set_post_chain, PSDR_ERR_NO_DATA for a client no chain batch has
 *   listed yet.
 * There is no psdr_group_* call: a group's clients run the context's AGC. */
typedef struct psdr_agc_profile {
    double desired;      /* target level, (0, 1] */
    double attack_ms;    /* (0, 10000] */
    double release_ms;   /* (0, 10000] */
    double max_gain;     /* > 0: upper bound of the wanted gain; 0: none (the reference) */
    int32_t manual;      /* 1: the wanted gain is manual_gain whatever the signal */
    double manual_gain;  /* >= 0, finite (read only when manual = 1) */
} psdr_agc_profile;
int psdr_client_set_agc_profile(psdr_ctx *ctx, int id, const psdr_agc_profile *p);   /* NULL: back to the context's AGC */
#define PSDR_AGC_REFERENCE 0   /* 0.2, 50, 300, no cap: the reference's constructor arguments */
#define PSDR_AGC_FAST      1   /* 0.2,  5, 100 */
#define PSDR_AGC_SLOW      2   /* 0.2, 50, 2000 */
int psdr_agc_preset(int kind, psdr_agc_profile *out);   /* needs no context */
int psdr_read_agc_gain(psdr_ctx *ctx, int id, float *gain);  /* the carried gain behind the client's last chain batch; synchronises */
/* A client added after the last psdr_demod_batch has no results in it (the reference's frame loop would not
 * have posted a task for it either, src/websocket.cpp:156-185): psdr_read_audio / psdr_read_pcm / psdr_fetched_audio
 * return PSDR_ERR_NO_DATA for such a slot instead of the previous occupant's samples.
 *
 * Batched read-back - what a per-frame fan-out should use: psdr_fetch_batch copies the last demod batch's audio,
 * pwr, NaN flags (and PCM with the post chain on; the IQ rows of PSDR_IQ clients) of ALL client slots into pinned host memory owned by the
 * context with ONE synchronisation and at most four strided copies; psdr_fetched_audio then hands out pointers
 * into that block (valid until the next psdr_fetch_batch) without touching the device.  frame: index inside the
 * batch.  audio / pcm: audio_fft_size/2 values.  Any output pointer may be NULL. */
int psdr_fetch_batch(psdr_ctx *ctx);
int psdr_fetched_audio(psdr_ctx *ctx, int id, int frame, const float **audio, float *pwr, int32_t *nan_flag,
                       const int32_t **pcm);
/* The same read-back WITHOUT a stall of the frame loop - the served end of the path: every send_audio / send_waterfall of
 * the reference ends in host memory (src/signal.cpp:283-291 -> src/audio.cpp:26-44; src/waterfall.cpp:44-51).
 * psdr_fetch_begin enqueues the device-to-host copies of the last psdr_demod_batch* (pwr and NaN flags always; float audio
 * with PSDR_FETCH_AUDIO; the post chain's PCM with PSDR_FETCH_PCM) and of the last psdr_waterfall_batch
 * (PSDR_FETCH_WATERFALL) on a copy stream of the context, behind the kernels that produce them, into one of
 * PSDR_FETCH_SETS pinned host sets (a ring; a set's buffers are allocated when it is first used), and returns at once.  The caller then enqueues the next batch (psdr_process_* / psdr_demod_batch /
 * psdr_waterfall_batch): the copies run beside its FFT passes; the kernels that overwrite the device-side results wait for
 * the copies in stream order (no host wait).  psdr_fetch_end waits for the OLDEST fetch in flight; from then on
 * psdr_fetched_audio / _window / _waterfall answer from that set, until the next psdr_fetch_end - its pointers stay valid
 * until PSDR_FETCH_SETS - 1 further psdr_fetch_begin calls have been made.  How far the host stays behind is the caller's
 * choice: one batch for the float audio; the post chain's PCM is ready up to two steps after its passes (three with
 * hundreds of clients), so a caller that fetches it keeps two or three fetches in flight.  A psdr_fetch_begin with every
 * set in flight waits for the oldest copy and gives its results up.  Frame-loop thread only.  psdr_fetch_batch = every outstanding
 * psdr_fetch_end + a full drain + begin(all) + end.  bench.py's `with_fetch` times this pattern. */
#define PSDR_FETCH_SETS 4
#define PSDR_FETCH_AUDIO 1u
#define PSDR_FETCH_PCM 2u
#define PSDR_FETCH_WATERFALL 4u
/* the IQ rows of the batch's PSDR_IQ clients (with pwr and NaN flags, as always): ONE copy of the span from the lowest to
 * the highest slot that was IQ in the batch, not of all max_clients slots - keep IQ clients in neighbouring slots. */
#define PSDR_FETCH_IQ 8u
int psdr_fetch_begin(psdr_ctx *ctx, unsigned what);
int psdr_fetch_end(psdr_ctx *ctx);
/* one frame of an IQ client in the fetched set: iq = n/2 (re, im) pairs in pinned host memory (NULL if the set was fetched
 * without PSDR_FETCH_IQ), valid like psdr_fetched_audio's pointers: until PSDR_FETCH_SETS - 1 further psdr_fetch_begin calls
 * have been made.  PSDR_ERR_NO_DATA: the client was not part of the fetched batch, or not as PSDR_IQ.  Any output pointer
 * may be NULL.  psdr_fetched_iq_span: what the fetch's IQ copy covered - the first slot, the number of slots (0: no IQ
 * client in the batch) and the bytes it moved (slots * frames * n/2 * 8); PSDR_ERR_STATE without PSDR_FETCH_IQ. */
int psdr_fetched_iq(psdr_ctx *ctx, int id, int frame, const float **iq, float *pwr, int32_t *nan_flag);
int psdr_fetched_iq_span(psdr_ctx *ctx, int *first_slot, int *nslots, size_t *bytes);
/* one frame's PCM row (audio_fft_size/2 int16) of client `id` in the fetched set when the batch was produced with
 * PSDR_OPT_POST_CHAIN_PCM16 = 1 (PSDR_ERR_STATE otherwise); pointer into pinned host memory, valid like psdr_fetched_audio's */
int psdr_fetched_pcm16(psdr_ctx *ctx, int id, int frame, const int16_t **pcm);
/* rows [nsent][r - l] of waterfall client `id` in the fetched set (pointer into pinned host memory, valid like
 * psdr_fetched_audio's), with the level and window they were GATHERED with.  PSDR_ERR_NO_DATA: the client was not
 * active in that batch.  Any output pointer may be NULL. */
int psdr_fetched_waterfall(psdr_ctx *ctx, int id, const int8_t **rows, int *nsent_out, int *level_out, int *l_out, int *r_out);
/* the window [l, r) and audio_mid client `id` was DEMODULATED with in the fetched batch (set_audio_range may have run on
 * another thread since, or have been refused): what the packet labels of src/signal.cpp:104-105, 287 must be computed
 * from.  Same error behaviour as psdr_fetched_audio. */
int psdr_fetched_window(psdr_ctx *ctx, int id, int *l, double *audio_mid, int *r);
/* device-resident results (no copy): audio of client slot `id` */
int psdr_audio_device_ptr(psdr_ctx *ctx, int id, const float **d_audio, const float **d_pwr);

/* Post-demodulation chain of AudioClient::send_audio (src/signal.cpp:277-284), batched for all
 * clients: DCBlocker (src/utils.h:139-169, delay audio_rate/750*2), AGC(0.2, 50 ms, 300 ms,
 * 200 ms look-ahead) (src/utils/audioprocessing.cpp:5-68; reset by
 * psdr_client_set_audio_demodulation like src/signal.cpp:316-328), dsp_float_to_int16 with
 * mult 65536/4 (src/utils/dsp.cpp:152-165).  Off by default; when on, every demod_batch also
 * produces the int16 PCM (held in int32, like the reference's int32_t buffer) that the reference
 * hands to its audio encoder.  Frames whose NaN flag is set are skipped by the chain (the
 * reference drops them before it, src/signal.cpp:266-271); their PCM rows are zero.
 * The conversion, for the AGC's output y (never NaN) and t = fma(y, 16384, 32768.5):
 *   t >= 65536 -> +32767,   t < 0 -> -32768,   otherwise (int)t - 32768.
 * That is the reference's value wherever the reference's `(int32)t - 32768` is defined (t < 2^31 and t - 32768 >= -2^31).
 * Beyond int32 - reached for real: digital silence drives the AGC's gain towards 0.2 / 1e-10 = 2e9, and part of it is still
 * there when a signal returns - the reference's expression is undefined and its x86 build yields +32767 for BOTH signs; this
 * is the one place where the library deliberately leaves that build: it saturates by sign (a hugely negative sample is
 * -32768).  int32 rows, the int16 rows of PSDR_OPT_POST_CHAIN_PCM16 and the CPU oracle share the one definition. */
int psdr_set_post_chain(psdr_ctx *ctx, int enable);
/* Knobs that are not part of psdr_config (whose layout is frozen per PSDR_ABI_VERSION).
 * PSDR_OPT_POST_CHAIN_STREAMS (before the first psdr_set_post_chain(ctx, 1); PSDR_ERR_STATE after it): which HIP streams the
 *   post chain's two sequential stages run on.  0 (default): streams created in a fixed order - deterministic, and in the
 *   FIRST context of a process these are the hardware queues that leave the FFT passes' launches alone.  1: chosen by a
 *   ~60 ms measurement of launch gaps (the chain's kernels beside empty launches on the main and the side stream) - for a
 *   process that creates several contexts, where creation order lands on a busy pipe of the command processor (+15 %
 *   instead of +3 % on the step); the outcome depends on wall-clock thresholds, and a failed
 *   measurement falls back to 0.
 * PSDR_OPT_POST_CHAIN_AGC (any time; drains the context): the form of the chain.  1 (default): the AGC as maxima of 16-sample
 *   chunks + ONE four-wave kernel for look-ahead peak, gain recurrence and int16 conversion - whenever the audio rate is a
 *   multiple of 80 Hz, the audio size a multiple of 8 and the CUs the chain reserves hold its work-groups - and the DC
 *   blocker's moving averages reading the demodulated rows themselves (no gathered copy while no frame is dropped and no
 *   client paused) and leaving the chunk maxima on their way: a third of the memory traffic of the other form, which is
 *   what the chain costs the FFT passes.  0: round 5's form everywhere (gather + five AGC kernels).
 *   Same bits either way, and the chain's carried state is the same: the forms may alternate between batches.
 * PSDR_OPT_POST_CHAIN_PCM16 (any time; drains the context): 1 = the chain writes its PCM as int16 rows instead of the int32
 *   buffer the reference hands its encoder (dsp_float_to_int16's output, src/utils/dsp.cpp:152-165, holds 16-bit values):
 *   half the bytes for psdr_fetch_begin(PSDR_FETCH_PCM) to move - with hundreds of clients the copy to the host is what
 *   bounds the served path.  psdr_fetched_pcm16 hands the rows out; psdr_fetched_audio's pcm is NULL for
 *   such a batch; psdr_read_pcm still delivers int32 (widened on the host).  0 (default): int32 rows.
 * PSDR_OPT_WATERFALL_DETECTOR (any time, any thread): the psdr_wf_detector a client gets at psdr_waterfall_add (clients that
 *   exist keep theirs: psdr_waterfall_set_detector).  PSDR_WF_SAMPLE (default): the reference's waterfall.
 * PSDR_OPT_FINE_TUNE (any time, any thread): 0 (default) or 1, the fine-tune flag a client gets at psdr_client_add (clients
 *   that exist keep theirs: psdr_client_set_fine_tune).  PSDR_ERR_INVALID for any other value.
 * PSDR_OPT_SAM_SIDEBAND (any time, any thread): the psdr_sam_sideband a client gets at psdr_client_add (clients that exist
 *   keep theirs: psdr_client_set_sam_sideband).  PSDR_SAM_BOTH (default).  PSDR_ERR_INVALID for any other value. */
enum { PSDR_OPT_POST_CHAIN_STREAMS = 1, PSDR_OPT_POST_CHAIN_AGC = 2, PSDR_OPT_POST_CHAIN_PCM16 = 3 };
#define PSDR_OPT_WATERFALL_DETECTOR 4
#define PSDR_OPT_FINE_TUNE 5
#define PSDR_OPT_SAM_SIDEBAND 6   /* the value a client gets at psdr_client_add; existing clients keep theirs */
#define PSDR_OPT_AUTO_NOTCH 7     /* 0 (default) or 1: the auto-notch flag a client gets at psdr_client_add; existing clients keep theirs */
#define PSDR_OPT_NOISE_REDUCTION 9 /* 0 (default) or a PSDR_NR_* preset: the noise reduction a client gets at psdr_client_add; existing
                                    * clients keep theirs.  PSDR_ERR_INVALID for any other value, PSDR_ERR_STATE without an audio_rate.  (8 stays free.) */
#define PSDR_OPT_AUDIO_BLANKER 10  /* 0 (default) or a PSDR_ANB_* preset: the audio blanker a client gets at psdr_client_add; existing
                                    * clients keep theirs.  PSDR_ERR_INVALID for any other value */
int psdr_set_option(psdr_ctx *ctx, int option, int value);
/* pcm: [frames of the last demod_batch][audio_fft_size/2]; nframes = rows pcm holds (as psdr_read_audio) */
int psdr_read_pcm(psdr_ctx *ctx, int id, int nframes, int32_t *pcm, int *nframes_out);

/* waterfall clients: WaterfallClient (src/waterfall.h) */
int psdr_waterfall_add(psdr_ctx *ctx, int *id_out);
int psdr_waterfall_remove(psdr_ctx *ctx, int id);
/* WaterfallClient::set_waterfall_range (src/waterfall.cpp:25-42); r is clamped to
 * R>>level (the reference forgets the upper bound, src/waterfall.cpp:55-58) */
int psdr_waterfall_set_range(psdr_ctx *ctx, int id, int level, int l, int r);
/* WaterfallClient::on_window_message (src/waterfall.cpp:53-94): picks the level */
int psdr_waterfall_on_window_message(psdr_ctx *ctx, int id, int l, int r, int *level_out,
                                     int *l_out, int *r_out);
/* What a sent row shows of the frames BETWEEN two sent frames - the detector of a spectrum display.  The reference sends
 * frame s (s % skip_num == 0) and drops the skip_num - 1 frames before it (src/fft.cpp:33,102-104), although the int8
 * pyramid exists for every frame: a burst shorter than skip_num frames is seen only if it falls on a sent one.
 *   PSDR_WF_SAMPLE  row[j] = q_s[j]: the reference's waterfall, bit for bit (the default; k_waterfall_gather alone runs)
 *   PSDR_WF_PEAK    row[j] = max over t in W(s) of q_t[j] (signed int8): max-hold
 *   PSDR_WF_MEAN    row[j] = floor((2 S + n) / (2 n)), S = sum over W(s) of q_t[j], n = |W(s)|: the mean of the dB values
 *                   (video averaging, round half up) - not of linear power, which is never stored per frame
 * q_t = frame t's values at the client's level, indices [l, r), as psdr_read_quantized delivers them.  W(s) is the WINDOW of
 * frame s: the frames t with s - skip_num < t <= s that belong to the current RUN (psdr_waterfall_batch below).  A detector
 * changes the bytes of a row and nothing else: number and length of the rows, labels, psdr_read_waterfall,
 * psdr_fetch_begin(PSDR_FETCH_WATERFALL) / psdr_fetched_waterfall are the same, and clients with different detectors share
 * a call.  psdr_waterfall_set_detector: any thread; PSDR_ERR_INVALID for an unknown id or value; PSDR_ERR_UNSUPPORTED for
 * PSDR_WF_MEAN on a context with skip_num > 2^24 (the sums are 32 bits wide: 255 * 2^24 fits); in force from the next
 * psdr_waterfall_batch on. */
typedef enum psdr_wf_detector { PSDR_WF_SAMPLE = 0, PSDR_WF_PEAK = 1, PSDR_WF_MEAN = 2 } psdr_wf_detector;
int psdr_waterfall_set_detector(psdr_ctx *ctx, int id, int detector);
/* waterfall_loop + send_waterfall (src/websocket.cpp:207-236, src/waterfall.cpp:44-51):
 * gathers q_level[l..r) of every waterfall client for every frame f of the last batch
 * with (first_frame_num+f) % skip_num == 0.
 * Detectors - runs and windows.  Each call speaks for the batch processed just before it.  A call whose first_frame_num
 * equals the previous call's first_frame_num + its number of frames CONTINUES the run; any other call (the first one, a
 * gap, a repeated first_frame_num) starts a new run, and so does the first call with a non-sample client among the active
 * ones after calls without any (the library keeps no history while nobody asks for it).  Frames before the run's start
 * never contribute: the first row of a run may stand for fewer than skip_num frames, frame 0 stands for itself.  Inside a
 * run a window reaches back across as many earlier batches as it needs (skip_num larger than the batch; one-frame
 * batches), through a context-wide carry over the raw pyramid records - element-wise maximum and sum of the run's frames
 * behind its last sent frame, updated by every call while some active client has a detector.  The client's window
 * [level, l, r) and detector AT THE CALL are applied to all frames of W(s): a client that retunes, zooms, changes its
 * detector or attaches in the middle of a window gets a complete row at the next sent frame.  A caller whose clients use
 * a detector therefore calls this for EVERY batch, also one without a sent frame (it gathers nothing, nsent = 0, and
 * feeds the carry).  psdr_group_step / _step_ring do: they call it on the root at every step, so the group path needs
 * nothing further. */
int psdr_waterfall_batch(psdr_ctx *ctx, uint64_t first_frame_num);
/* bytes [nsent][r-l] for one client, with the range the rows were GATHERED with: the window may
 * have been changed by another thread since psdr_waterfall_batch, so level/l/r of that batch are
 * returned (any of the out pointers may be NULL).  *nsent_out = number of sent frames in the batch;
 * out == NULL only queries. */
int psdr_read_waterfall(psdr_ctx *ctx, int id, int8_t *out, size_t out_cap, int *nsent_out, int *level_out,
                        int *l_out, int *r_out);

/* Band scan: a smoothed spectrum trace, the noise floor of the band by segments and a list of the signals on it - for markers
 * on the waterfall, "next signal up / down" tuning, an automatic colour scale and an occupancy display.  Context-wide and
 * opt-in: a context that never switches it on allocates nothing, a batch without a psdr_scan_batch launches nothing, and every
 * other output is bit for bit the same with the scan on or off.  Only the device can do this: the int8 pyramid of EVERY frame
 * is there, and the frames between two sent waterfall rows never leave it.
 *   The rule.  Every quantity is an integer; phantomsdr_amd/csrc/scanplan.h is the one definition of every step, for the device
 *   and for a host program alike.
 *   Values.  For scan level v, n = R >> v (R: the bins of level 0) and q_t[j], j in [0, n), is frame t's int8 value at level v -
 *     exactly what psdr_read_quantized delivers, indexed as a waterfall client's l and r are at that level.  u = q + 128 is in
 *     0..255.  One count of q is 0.5 dB: q = 20 log10(P) + 127 with P the bin's POWER scaled by the level's power offset
 *     (quantize.h), so q rises by 20 per decade of power, 10 log10 of a power ratio = (difference of q) / 2.
 *   Trace.  s[j], a uint32 in units of 1/256 count above -128.  The first frame of a run sets s = u << 8; every later frame, in
 *     frame order, d = (int)(u << 8) - (int)s; s += d >> a, the shift arithmetic (floor), a = avg_shift in 0..8 (0: the trace
 *     is the last frame).  s stays inside [0, 255 * 256], and the trace after frame f does not depend on how the frames were
 *     split into batches.
 *   Runs of frames.  psdr_waterfall_batch's rule: a psdr_scan_batch whose first_frame_num equals the previous call's
 *     first_frame_num plus its number of frames continues the run; any other call starts a new run, and so does the first call
 *     behind a psdr_scan_set.
 *   Evaluation, once per psdr_scan_batch, on the trace as it stands after the batch's last frame:
 *     Segments.  A segment is 256 bins, G = n / 256 of them.  Q_g is the 63rd smallest (0-based) of the segment's 256 trace
 *       values, the lower quartile; F_g = min(Q_{g-1}, Q_g, Q_{g+1}) over the neighbours that exist, so that a crowded segment
 *       does not lift its own floor.
 *     Hot bins.  hot[j] = s[j] >= F_{j >> 8} + (threshold << 8); threshold in 1..255, in counts (0.5 dB each).
 *     Runs of bins.  gap in 0..64.  Bin j starts a run if it is hot and no bin of [j - gap - 1, j - 1] is hot; hot bin j ends a
 *       run, with end = j + 1, if no bin of [j + 1, j + 1 + gap] is hot; bins outside [0, n) are not hot; segment borders do not
 *       cut runs.  Each run gives one psdr_signal: first, end, peak_bin (the lowest bin of [first, end) with the largest s - a
 *       cold bin inside the run counts), peak = s[peak_bin], floor = F_{peak_bin >> 8}.
 *     List.  The first PSDR_SCAN_MAX_SIGNALS runs in ascending order of first are kept, and the total number of runs, which
 *       is not truncated.
 * psdr_scan_set: any thread; in force from the next psdr_scan_batch, which starts a new run; NULL switches the scan off.  What
 *   the read calls deliver is gone until the next evaluation.  PSDR_ERR_INVALID, with nothing changed and a text of its own each,
 *   in this order: level outside [0, downsample_levels); R >> level < 256; avg_shift outside 0..8; threshold outside 1..255; gap
 *   outside 0..64.  The first call that switches the scan on allocates its device state - trace, bit mask, floors, list and
 *   scratch, sized for level 0 (about 2.6 bytes per bin of R) - all or none: PSDR_ERR_NOMEM leaves the setting unchanged.
 * psdr_scan_batch: frame-loop thread; speaks for the batch processed just before it, like psdr_waterfall_batch, and is ordered
 *   against the passes in the same way (the records it reads are overwritten by the next batch): call it before the next
 *   psdr_process_*.  PSDR_ERR_STATE while the scan is off, and (scan on) before any batch was processed.
 * The read calls synchronise; PSDR_ERR_NO_DATA before the first evaluation (and behind a psdr_scan_set until the next one).
 *   psdr_read_signals: the signals of the list with end - first >= min_width, in the list's order; at most cap of them are
 *     copied to out, *n_out says how many passed (it may exceed cap), *total_out is the device's untruncated number of runs,
 *     *frame_num_out the number of the last frame in the trace.  Any out pointer may be NULL.  PSDR_ERR_INVALID for cap < 0.
 *   psdr_read_scan_floor: F_g, G values; psdr_read_scan_trace: s[j] as uint16, n values.  *nseg_out / *n_out say how many there
 *     are; a NULL buffer only queries; PSDR_ERR_INVALID, nothing written, for a buffer that holds fewer.
 * There is no PSDR_FETCH_* bit and no psdr_group_* call for the scan: a group's caller runs it on the root,
 * psdr_group_ctx(g, 0), which transforms every frame. */
#define PSDR_SCAN_MAX_SIGNALS 8192
typedef struct psdr_scan_config { int level, avg_shift, threshold, gap; } psdr_scan_config;
typedef struct psdr_signal { uint32_t first, end, peak_bin; uint32_t peak, floor; } psdr_signal; /* peak, floor: 1/256 count above -128 */
int psdr_scan_set(psdr_ctx *ctx, const psdr_scan_config *cfg);      /* NULL: off */
int psdr_scan_batch(psdr_ctx *ctx, uint64_t first_frame_num);       /* speaks for the batch processed just before it */
int psdr_read_signals(psdr_ctx *ctx, int min_width, psdr_signal *out, int cap, int *n_out, int *total_out, uint64_t *frame_num_out);
int psdr_read_scan_floor(psdr_ctx *ctx, uint32_t *F, int cap, int *nseg_out);
int psdr_read_scan_trace(psdr_ctx *ctx, uint16_t *s, size_t cap, size_t *n_out);

/* last batch, raw device-side results (for consumers that stay on the GPU, and tests) */
/* spectrum of frame f, normalised by 1/N exactly like src/fft_impl.cpp:34-35.  IQ: N complex bins
 * indexed by the CLIENT coordinate c (bin k = (c+N/2+1) mod N); real: N/2+1 bins indexed by k.
 * The DEVICE LAYOUT is opaque: transforms whose row pass has 1024 points (2^20/2^21-point IQ,
 * 2^21/2^22-point real) keep a frame in tile-major 128-byte lines (phantomsdr_amd/csrc/quantize.h,
 * SpecLayout); psdr_demod_batch_from() on a context created with the same configuration understands
 * it (that is what the spectrum broadcast between GPUs ships), psdr_read_spectrum() delivers the
 * reference's k order.  nbins complex values per frame; frames are spec_stride apart:
 * N (IQ) or N/2+2 (real) bins. */
int psdr_spectrum_device_ptr(psdr_ctx *ctx, int frame, const float **d_spec, size_t *nbins);
/* (level-major layout as in the reference; materialised on demand from the device's tiled
 * records, so this call synchronises) */
int psdr_quantized_device_ptr(psdr_ctx *ctx, int frame, const int8_t **d_q, size_t *nbytes);
/* copies of the same to host; spectrum is delivered in the reference's k order */
int psdr_read_spectrum(psdr_ctx *ctx, int frame, float *out_k_order);
int psdr_read_quantized(psdr_ctx *ctx, int frame, int8_t *out);

/* ---- multi-GPU from C: ONE process, n devices of a node ---------------------------------------------
 * Device devices[0] is the root: it owns the raw ring, the forward FFT and the waterfall clients (use
 * psdr_group_ctx(g, 0) with the psdr_ring_* and psdr_waterfall_* calls above); the audio clients are spread over all n
 * contexts and every batch is exchanged ONCE over xGMI through RCCL, called directly (librccl.so is dlopen()ed when a
 * group of more than one device is created; a single-device group never loads it and issues no collective):
 *   PSDR_SHARD_CLIENTS  ncclBroadcast of the spectrum (BASELINE.json configs[3]); client i lives on device i mod n
 *   PSDR_SHARD_RAW      ncclBroadcast of the raw half-frames, every device runs the forward FFT itself
 *   PSDR_SHARD_BAND     device b receives band b of the spectrum + a halo of one maximal window (ncclSend / ncclRecv of
 *                       1/n of the bytes; n a power of two); a client lives on the device of the band its window starts in
 * | PSDR_SHARD_FORCE_COMM: create the communicator and issue the collectives even for ONE device (testing the RCCL
 * plumbing on a single-GPU box): CLIENTS / RAW broadcast to the one rank; BAND packs band 0 (the whole spectrum), sends it to
 * and receives it from itself (ncclSend / ncclRecv in one group) and demodulates from the received buffer.
 * | PSDR_SHARD_PEER_COPY: no RCCL at all - after the root's transform every peer pulls its share with hipMemcpyPeerAsync
 * on its own stream (n - 1 independent copies, one per root-to-peer xGMI link, ordered by events).  With it a device may
 * be listed more than once: n ranks on fewer GPUs, which is how a one-GPU box runs the multi-rank logic (placement, band
 * regions and halos, migration, fetch) for real.
 * The exchange of batch b runs BESIDE the root's transform of batch b + 1 (spectrum broadcast, and band regions written by
 * the root's second pass): the root alternates its two result sets and issues its side of the collective on an exchange
 * stream of its own; a set is overwritten only after its exchange has completed (stream-ordered, no host wait).
 * | PSDR_SHARD_SERIAL: exchange and transform strictly one after the other on the root's stream (round 5's schedule; A/B
 * and the bit-identity test of the overlapped schedule).  Raw sharding and packed band buffers are always serial.
 * Everything else of a rank is ordered on one stream per device; psdr_group_step returns without synchronising.  The calls
 * below may come from different threads (the server's websocket threads and its frame loop): the group serialises the
 * client calls (add / remove / set_* / fetched_*) against each other and against a step's enqueue.  psdr_group_step*,
 * psdr_group_fetch, psdr_group_synchronize and psdr_group_link_stats belong to the FRAME-LOOP thread alone (they wait for
 * devices and read the step's timing events: no lock is held while they do).
 * The process-per-GPU twin of this (torch.distributed over RCCL) is phantomsdr_amd/distributed.py.
 * Time sharding (batch g on device g mod n, no collective) needs no group: n independent contexts.
 * STATUS: no group of more than one physical device has run on hardware yet (every round's GPU box had one MI355X): the
 * RCCL calls have executed with one rank only, the multi-rank logic through PSDR_SHARD_PEER_COPY on one device.  Treat
 * ndevices > 1 - and PSDR_SHARD_BAND over RCCL in particular - as EXPERIMENTAL until a node run exists. */
typedef struct psdr_group psdr_group;
enum { PSDR_SHARD_CLIENTS = 0, PSDR_SHARD_RAW = 1, PSDR_SHARD_BAND = 2, PSDR_SHARD_FORCE_COMM = 0x100, PSDR_SHARD_PEER_COPY = 0x200,
       PSDR_SHARD_SERIAL = 0x400 };
int psdr_group_create(const psdr_config *cfg, const int *devices, int ndevices, int shard, psdr_group **out);
void psdr_group_destroy(psdr_group *g);
int psdr_group_size(const psdr_group *g);
psdr_ctx *psdr_group_ctx(psdr_group *g, int rank);
/* audio clients: the group picks the device; *gid_out names the client in every psdr_group_client_* / _fetched_* call and
 * NEVER changes (an index into the group's own table of (device, slot)).
 * psdr_group_client_set_audio_range: band sharding moves a client whose window now starts in another band to that
 * band's device behind its gid.  The demodulation state the reference keeps across a retune (src/signal.cpp:81-94) -
 * overlap-add tails, FM's last sample - the mode and the paused flag travel with it; the post chain's history on the GPU
 * (DC sums, AGC gain and look-ahead) does not: the client starts there like a fresh one (an AGC transient the reference
 * does not have); and psdr_group_fetched_audio answers PSDR_ERR_NO_DATA until the new device has demodulated a batch.
 * psdr_group_client_rank: the rank (index into `devices`) a client lives on now, -1 for an unknown gid. */
/* PSDR_IQ is not served through a group (its rows are neither migrated nor fetched by gid): psdr_group_client_add and
 * psdr_group_client_set_audio_demodulation answer PSDR_ERR_UNSUPPORTED for it.  The same holds for PSDR_SAM: the carrier
 * tail is not migrated and the carrier records are not fetched by gid.  There is no psdr_group_* call for the fine-tune
 * flag: a group's clients are untuned, and a band migration carries the flag's value 0.  There is none for notches either
 * (psdr_client_set_notch, psdr_client_set_auto_notch): a group's clients have none, and a band migration carries none.  Nor
 * is there one for the squelch (psdr_client_set_squelch): a group's clients are always open, and a band migration carries
 * neither the setting nor the gate's state.  Nor for the AGC profile (psdr_client_set_agc_profile): a group's clients run the
 * context's AGC. */
int psdr_group_client_add(psdr_group *g, int l, double audio_mid, int r, int mode, int *gid_out);
int psdr_group_client_remove(psdr_group *g, int gid);
int psdr_group_client_set_audio_range(psdr_group *g, int gid, int l, double audio_mid, int r);
int psdr_group_client_rank(psdr_group *g, int gid);
int psdr_group_client_set_audio_demodulation(psdr_group *g, int gid, int mode);
int psdr_group_client_set_paused(psdr_group *g, int gid, int paused);
/* one batch: the root transforms nframes frames (d_halves_root: nframes + 1 raw half-frames on the ROOT device; _ring:
 * the root context's ingest ring from first_half on), the exchange, every device demodulates its clients, the root
 * gathers the waterfall rows (psdr_demod_batch + psdr_waterfall_batch of a single context, for the whole group) */
int psdr_group_step(psdr_group *g, const void *d_halves_root, int nframes, uint64_t first_frame_num);
int psdr_group_step_ring(psdr_group *g, uint64_t first_half, int nframes, uint64_t first_frame_num);
int psdr_group_synchronize(psdr_group *g);
/* bytes that crossed ONE root-to-peer link in the last step, and the exchange's duration (RCCL: on the root's stream;
 * PSDR_SHARD_PEER_COPY: the slowest peer's own copy) */
int psdr_group_link_stats(psdr_group *g, double *bytes_per_link, double *exchange_ms);
/* psdr_fetch_batch on every device, then psdr_fetched_audio / psdr_fetched_window by gid */
int psdr_group_fetch(psdr_group *g);
int psdr_group_fetched_audio(psdr_group *g, int gid, int frame, const float **audio, float *pwr, int32_t *nan_flag,
                             const int32_t **pcm);
int psdr_group_fetched_window(psdr_group *g, int gid, int *l, double *audio_mid, int *r);

/* ---- wire formats of the reference's packets (host side) ----------------------- */
/* The CBOR map nlohmann::json::to_cbor produces in AudioEncoder::send (src/audio.cpp:17-36):
 * {"data": payload, "frame_num", "l", "m", "pwr", "r"} (keys in std::map order, shortest integer
 * heads, binary32 floats when exact).  payload = the encoded audio frame (FLAC/Opus bytes: the codecs
 * stay outside).  out must hold psdr_wire_packet_bound(bytes); *len = bytes written. */
size_t psdr_wire_packet_bound(size_t payload_bytes);
int psdr_wire_audio_packet(uint64_t frame_num, int l, double m, int r, double pwr, const void *payload,
                           size_t bytes, uint8_t *out, size_t cap, size_t *len);
/* WaterfallEncoder::set_data + the CBOR of ZstdEncoder::send (src/waterfallcompression.cpp:13-31):
 * {"data": int8 row, "frame_num", "l", "r"}; l, r are the client's range << level (src/waterfall.cpp:47) */
int psdr_wire_waterfall_packet(uint64_t frame_num, int l, int r, const void *payload, size_t bytes,
                               uint8_t *out, size_t cap, size_t *len);
/* ... and its zstd stream: one ZSTD_CStream per waterfall client, every packet flushed with
 * ZSTD_compressStream2(..., ZSTD_e_flush) (src/waterfallcompression.cpp:32-35).  libzstd is looked up
 * at run time; PSDR_ERR_UNSUPPORTED if the host has none. */
typedef struct psdr_zstd psdr_zstd;
int psdr_wire_zstd_create(psdr_zstd **out);
void psdr_wire_zstd_destroy(psdr_zstd *zs);
size_t psdr_wire_zstd_bound(size_t nbytes);
int psdr_wire_zstd_flush(psdr_zstd *zs, const void *in, size_t nbytes, uint8_t *out, size_t cap, size_t *len);

/* The text frame a client receives first (broadcast_server::send_basic_info, src/websocket.cpp:42-66):
 * a glaze (v2.4.4, subprojects/glaze.wrap) json_t object, i.e. a std::map - keys in lexicographic
 * order at both levels - whose numbers are all doubles, written in their shortest round-trip form
 * (integers without a fraction).  Strings are written as they are (the reference's are plain ASCII
 * mode and codec names; '"' and '\\' are escaped).  *len excludes the terminating NUL that is also
 * written. */
typedef struct psdr_hello {
    double sps, audio_max_sps, audio_max_fft, fft_size, fft_result_size, waterfall_size, basefreq;
    double total_bandwidth;           /* is_real ? sps / 2 : sps */
    double default_frequency, default_l, default_m, default_r;
    const char *default_modulation;   /* "USB" | "LSB" | "AM" | "FM" */
    const char *waterfall_compression, *audio_compression;
} psdr_hello;
int psdr_wire_hello_json(const psdr_hello *h, char *out, size_t cap, size_t *len);
/* A client's command frame (Client::on_message, src/client.cpp:19-117): a JSON object tagged by
 * "cmd" = "window" {l, r, m?, level?} | "demodulation" {demodulation} | "userid" {userid} | "mute"
 * {mute}.  Like glz::read_json with default options: an unknown key, a value of the wrong type or
 * malformed JSON rejects the message (PSDR_ERR_INVALID; the reference then ignores it, `if (ec)
 * return`), a missing key leaves its field at 0 / absent, null is "absent" for the optional m and
 * level.  text = the demodulation name or the user id cut to 32 characters (src/client.cpp:121). */
enum { PSDR_CMD_WINDOW = 0, PSDR_CMD_DEMODULATION = 1, PSDR_CMD_USERID = 2, PSDR_CMD_MUTE = 3 };
typedef struct psdr_command {
    int32_t cmd;
    int32_t l, r;
    int32_t has_m, has_level;
    double m;
    int32_t level;
    int32_t mute;
    char text[36];
} psdr_command;
int psdr_wire_parse_command(const char *msg, size_t len, psdr_command *out);

/* ---- instrumentation --------------------------------------------------------------- */
/* mode 0: off.  1: every kernel launch is bracketed by hipEvents on the stream it is launched on (the
 * marker packets between the kernels lengthen the two FFT passes by several per cent: use it for a replay,
 * not for a timed region).  2: no events; the two FFT passes stamp the device's constant 100 MHz clock at
 * their first work-group's entry and their last work-group's exit (two fire-and-forget atomics per
 * work-group) - cheap enough to stay on inside a timed region; up to 8192 launches per pass between resets. */
int psdr_set_profiling(psdr_ctx *ctx, int mode);
/* per-launch durations (microseconds) of kernel `name` ("fft_pass1", "fft_pass2", ...) since the last
 * reset, oldest first; *n_out = how many exist (may exceed cap) */
int psdr_get_kernel_samples(psdr_ctx *ctx, const char *name, double *us_out, int cap, int *n_out);
/* accumulated since the last reset: name[i] (static strings), total ms, launch count */
int psdr_get_kernel_stats(psdr_ctx *ctx, int max_entries, const char **names, double *total_ms,
                          int64_t *launches, int *n_out);
int psdr_reset_kernel_stats(psdr_ctx *ctx);
/* hipEvent-timed wall time of a region on the context's stream */
int psdr_timer_start(psdr_ctx *ctx);
int psdr_timer_stop_ms(psdr_ctx *ctx, double *ms_out);
/* the HIP stream (hipStream_t) the context launches on, for interop */
void *psdr_stream(psdr_ctx *ctx);
/* enqueue on the caller's stream instead (e.g. the stream RCCL collectives are ordered
 * against); NULL restores the context's own stream */
int psdr_set_stream(psdr_ctx *ctx, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* PSDR_H */

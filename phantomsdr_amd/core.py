"""Host-side mirror of the reference's plug-in/operator interface for the hot path, on top
of the C-ABI (include/psdr.h).  Names and argument meaning follow the reference:

  HipFFT            <-> class FFT / FFTW / cuFFT      (src/fft.h:33-63, src/fft_cuda.cu)
  AudioClient       <-> class AudioClient             (src/signal.h:53-123, src/signal.cpp)
  WaterfallClient   <-> class WaterfallClient         (src/waterfall.h, src/waterfall.cpp)
  SpectrumEngine    <-> the frame loop + fan-out      (src/fft.cpp:47-105,
                                                       src/websocket.cpp:156-185,207-236)

Everything numeric happens in libpsdr_hip.so (hand-written HIP, gfx950); this module only
marshals pointers.  numpy is used for host arrays; torch is not required here.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import PsdrError, check, psdr_config

FORMATS = {"u8": 0, "s8": 1, "u16": 2, "s16": 3, "f32": 4, "f64": 5}
FORMAT_DTYPES = {"u8": np.uint8, "s8": np.int8, "u16": np.uint16, "s16": np.int16,
                 "f32": np.float32, "f64": np.float64}
USB, LSB, AM, FM = 0, 1, 2, 3
IQ = 4  # PSDR_IQ (include/psdr.h): the overlap-added complex baseband itself as the client's output
SAM = 5  # PSDR_SAM: synchronous AM, detection against the recovered carrier (audio like AM, plus carrier records)
MODES = {"USB": USB, "LSB": LSB, "AM": AM, "FM": FM, "IQ": IQ, "SAM": SAM}
# psdr_sam_sideband (include/psdr.h): which sideband a SAM client detects against the recovered carrier
SAM_BOTH, SAM_UPPER, SAM_LOWER = 0, 1, 2
SAM_SIDEBANDS = {"both": SAM_BOTH, "upper": SAM_UPPER, "lower": SAM_LOWER}
SQ_ABSOLUTE, SQ_NOISE = 0, 1  # psdr_client_set_squelch_reference
SQUELCH_REFERENCES = {"absolute": SQ_ABSOLUTE, "noise": SQ_NOISE}
# psdr_wf_detector (include/psdr.h): what a sent waterfall row shows of the frames since the previous one
WF_SAMPLE, WF_PEAK, WF_MEAN = 0, 1, 2
WF_DETECTORS = {"sample": WF_SAMPLE, "peak": WF_PEAK, "mean": WF_MEAN}

# PSDR_AF_* (include/psdr.h): the presets of psdr_audio_filter_design
AF_DEEMPHASIS, AF_HIGHPASS, AF_LOWPASS, AF_PEAK = 0, 1, 2, 3
AF_KINDS = {"deemphasis": AF_DEEMPHASIS, "highpass": AF_HIGHPASS, "lowpass": AF_LOWPASS, "peak": AF_PEAK}
AUDIO_FILTER_SECTIONS = 2

# PSDR_NR_* (include/psdr.h): the presets of psdr_noise_reduction_preset
NR_LIGHT, NR_NORMAL, NR_STRONG = 1, 2, 3
NR_PRESETS = {"light": NR_LIGHT, "normal": NR_NORMAL, "strong": NR_STRONG}

# PSDR_ANB_* (include/psdr.h): the presets of psdr_audio_blanker_preset
ANB_LIGHT, ANB_NORMAL, ANB_STRONG = 1, 2, 3
ANB_PRESETS = {"light": ANB_LIGHT, "normal": ANB_NORMAL, "strong": ANB_STRONG}

# psdr_signal (include/psdr.h): one signal of the band scan's list; peak and floor in 1/256 count above -128
SIGNAL_DTYPE = np.dtype([("first", np.uint32), ("end", np.uint32), ("peak_bin", np.uint32), ("peak", np.uint32), ("floor", np.uint32)])
SCAN_MAX_SIGNALS = 8192  # PSDR_SCAN_MAX_SIGNALS

# PSDR_AGC_* (include/psdr.h): the presets of psdr_agc_preset
AGC_REFERENCE, AGC_FAST, AGC_SLOW = 0, 1, 2
AGC_PRESETS = {"reference": AGC_REFERENCE, "fast": AGC_FAST, "slow": AGC_SLOW}

FFTW_MEASURE, FFTW_DESTROY_INPUT, FFTW_ESTIMATE = 0, 1, 1 << 6  # accepted and ignored


def agc_preset(kind):
    """an AGC profile as a dict for AudioClient.set_agc_profile(**...) (psdr_agc_preset; needs no context): "reference" (0.2, 50 ms,
    300 ms: the context's own), "fast" (5 / 100 ms) or "slow" (50 / 2000 ms), or an AGC_* constant"""
    p = _lib.psdr_agc_profile()
    k = AGC_PRESETS[kind] if isinstance(kind, str) else int(kind)
    check(_lib.load().psdr_agc_preset(k, C.byref(p)))
    return dict(desired=p.desired, attack_ms=p.attack_ms, release_ms=p.release_ms, max_gain=p.max_gain, manual=bool(p.manual),
                manual_gain=p.manual_gain)


TONE_ANY = -1  # PSDR_TONE_ANY


def tone_table():
    """the 50 standard sub-audible tones in Hz, ascending: index = the tone's number (psdr_tone_table; needs no context)"""
    hz, n = C.POINTER(C.c_double)(), C.c_int(0)
    check(_lib.load().psdr_tone_table(C.byref(hz), C.byref(n)))
    return [hz[k] for k in range(n.value)]


def tone_defaults(audio_rate):
    """the tone decoder's defaults at `audio_rate` as a dict for AudioClient.set_tone_decoder(**...) (psdr_tone_defaults; needs no
    context): any tone, gate on, snr_db 22, min_level 0, attack 2 blocks, hang one window of blocks"""
    p = _lib.psdr_tone_config()
    check(_lib.load().psdr_tone_defaults(float(audio_rate), C.byref(p)))
    return dict(want=p.want, gate=p.gate, snr_db=p.snr_db, min_level=p.min_level, attack_blocks=p.attack_blocks, hang_blocks=p.hang_blocks)


CW_FIELDS = ("pitch_hz", "search_hz", "wpm", "track_speed", "snr_db")


def cw_defaults(audio_rate):
    """the CW decoder's defaults at `audio_rate` as a dict for AudioClient.set_cw_decoder(**...) (psdr_cw_defaults; needs no
    context): pitch 700 Hz, search 100 Hz, 20 WPM, speed tracking on, snr_db 22"""
    p = _lib.psdr_cw_config()
    check(_lib.load().psdr_cw_defaults(float(audio_rate), C.byref(p)))
    return {k: getattr(p, k) for k in CW_FIELDS}


RTTY_FIELDS = ("mark_hz", "shift_hz", "baud", "usos", "search_hz", "snr_db")


def rtty_defaults(audio_rate):
    """the RTTY decoder's defaults at `audio_rate` as a dict for AudioClient.set_rtty_decoder(**...) (psdr_rtty_defaults; needs no
    context): mark 2125 Hz (915 Hz where the audio_rate has no room for it), shift 170 Hz, 45.45 baud, unshift on space, search
    60 Hz, the measured snr_db"""
    p = _lib.psdr_rtty_config()
    check(_lib.load().psdr_rtty_defaults(float(audio_rate), C.byref(p)))
    return {k: getattr(p, k) for k in RTTY_FIELDS}


PSK_FIELDS = ("carrier_hz", "baud", "search_hz", "quality")


def psk_defaults(audio_rate):
    """the PSK31 decoder's defaults at `audio_rate` as a dict for AudioClient.set_psk_decoder(**...) (psdr_psk_defaults; needs no
    context): carrier 1000 Hz, 31.25 baud, search 11.71875 Hz (three lanes to either side), the measured quality"""
    p = _lib.psdr_psk_config()
    check(_lib.load().psdr_psk_defaults(float(audio_rate), C.byref(p)))
    return {k: getattr(p, k) for k in PSK_FIELDS}


FAX_AUTO, FAX_FREE = 0, 1
FAX_FIELDS = ("mode", "black_hz", "white_hz", "lpm", "width", "slant_ppm", "phase_col", "tone_ratio", "start_blocks", "phase_lines", "max_lines")
FAX_INT_FIELDS = ("mode", "width", "phase_col", "start_blocks", "phase_lines", "max_lines")


def fax_defaults(audio_rate):
    """the radiofax decoder's defaults at `audio_rate` as a dict for AudioClient.set_fax_decoder(**...) (psdr_fax_defaults; needs no
    context): PSDR_FAX_AUTO, black 1500 Hz, white 2300 Hz, 120 lines per minute, 1024 pixels, the measured tone_ratio"""
    p = _lib.psdr_fax_config()
    check(_lib.load().psdr_fax_defaults(float(audio_rate), C.byref(p)))
    return {k: getattr(p, k) for k in FAX_FIELDS}


def noise_reduction_preset(kind):
    """(depth_db, beta) of a noise reduction preset for AudioClient.set_noise_reduction (psdr_noise_reduction_preset; needs no
    context): "light" (8 dB, 1), "normal" (14 dB, 1.5) or "strong" (22 dB, 2), or an NR_* constant"""
    d, b = C.c_double(0), C.c_double(0)
    k = NR_PRESETS[kind] if isinstance(kind, str) else int(kind)
    check(_lib.load().psdr_noise_reduction_preset(k, C.byref(d), C.byref(b)))
    return d.value, b.value


def audio_blanker_preset(kind):
    """(threshold, width) of an audio blanker preset for AudioClient.set_audio_blanker (psdr_audio_blanker_preset; needs no
    context): "light" (6, 5), "normal" (4.5, 7) or "strong" (3.5, 11), or an ANB_* constant"""
    t, w = C.c_double(0), C.c_int(0)
    k = ANB_PRESETS[kind] if isinstance(kind, str) else int(kind)
    check(_lib.load().psdr_audio_blanker_preset(k, C.byref(t), C.byref(w)))
    return t.value, w.value


def design_audio_filter(kind, rate, f0, q=math.sqrt(0.5)):
    """one section (b0, b1, b2, a1, a2) for AudioClient.set_audio_filter (psdr_audio_filter_design; needs no context): kind
    "deemphasis" (first-order low-pass with its corner at f0, q ignored), "highpass", "lowpass" or "peak" (0 dB at f0, bandwidth
    f0 / q), or an AF_* constant"""
    b = _lib.psdr_biquad()
    k = AF_KINDS[kind] if isinstance(kind, str) else int(kind)
    check(_lib.load().psdr_audio_filter_design(k, float(rate), float(f0), float(q), C.byref(b)))
    return (b.b0, b.b1, b.b2, b.a1, b.a2)


def derived_params(sps, fft_size, is_real, audio_sps=12000, waterfall_size=1024):
    """src/spectrumserver.cpp:99-105 (R), :151 (audio_max_fft_size), :186-190
    (downsample_levels) and src/fft.cpp:33 (skip_num)."""
    R = fft_size // 2 if is_real else fft_size
    n = int(math.ceil(float(audio_sps) * fft_size / sps / 4.0) * 4)
    levels, cur = 0, R
    while cur >= waterfall_size:
        levels += 1
        cur //= 2
    skip = max(1, int(math.floor((np.float32(sps) / np.float32(fft_size)) / 10.0)) * 2)
    return dict(fft_result_size=R, audio_fft_size=n, downsample_levels=levels, skip_num=skip)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """Owns one psdr_ctx."""

    @staticmethod
    def _config(fft_size, is_real, downsample_levels, brightness_offset=0,
                additional_size=0, audio_fft_size=0, audio_rate=12000, input_format="f32",
                device=0, max_batch=1, max_clients=1, max_waterfall_clients=1, skip_num=1, waterfall_size=0):
        cfg = psdr_config()
        cfg.struct_size = C.sizeof(psdr_config)
        cfg.fft_size = fft_size
        cfg.is_real = int(bool(is_real))
        cfg.downsample_levels = downsample_levels
        cfg.brightness_offset = brightness_offset
        cfg.additional_size = additional_size
        cfg.audio_fft_size = audio_fft_size
        cfg.audio_rate = audio_rate
        cfg.input_format = FORMATS[input_format] if isinstance(input_format, str) else input_format
        cfg.device = device
        cfg.max_batch = max_batch
        cfg.max_clients = max_clients
        cfg.max_waterfall_clients = max_waterfall_clients
        cfg.skip_num = skip_num
        cfg.waterfall_size = waterfall_size
        return cfg

    def __init__(self, fft_size, is_real, downsample_levels, brightness_offset=0,
                 additional_size=0, audio_fft_size=0, audio_rate=12000, input_format="f32",
                 device=0, max_batch=1, max_clients=1, max_waterfall_clients=1, skip_num=1, waterfall_size=0):
        self.lib = _lib.load()
        cfg = Context._config(fft_size, is_real, downsample_levels, brightness_offset, additional_size, audio_fft_size,
                              audio_rate, input_format, device, max_batch, max_clients, max_waterfall_clients, skip_num,
                              waterfall_size)
        self.h = C.c_void_p()
        check(self.lib.psdr_create(C.byref(cfg), C.byref(self.h)))
        self._owned = True
        self._describe(cfg)

    @classmethod
    def _view(cls, lib, handle, cfg):
        """a Context object over a psdr_ctx somebody else owns (a psdr_group's member): close() leaves it alone"""
        self = cls.__new__(cls)
        self.lib = lib
        self.h = C.c_void_p(handle)
        self._owned = False
        self._describe(cfg)
        return self

    def _describe(self, cfg):
        self.cfg = cfg
        fft_size, is_real = cfg.fft_size, bool(cfg.is_real)
        self.N = fft_size
        self.is_real = is_real
        self.R = fft_size // 2 if is_real else fft_size
        self.levels = cfg.downsample_levels
        self.n = cfg.audio_fft_size
        self.max_batch = cfg.max_batch
        self.q_len = sum(self.R >> i for i in range(cfg.downsample_levels))
        self.nbins = fft_size // 2 + 1 if is_real else fft_size
        self.last_nframes = 0
        self.last_demod_frames = 0
        self.input_format = cfg.input_format

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            for p in getattr(self, "_pinned", []):
                self.lib.psdr_host_free(self.h, p)
            self._pinned = []
            if getattr(self, "_owned", True):
                self.lib.psdr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- device memory -------------------------------------------------------------
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        check(self.lib.psdr_dev_alloc(self.h, nbytes, C.byref(p)))
        return p

    def dev_free(self, p):
        check(self.lib.psdr_dev_free(self.h, p))

    def h2d(self, dptr, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        check(self.lib.psdr_memcpy_h2d(self.h, C.c_void_p(dptr.value + offset), _ptr(arr), arr.nbytes))

    def d2h(self, arr, dptr, offset=0):
        check(self.lib.psdr_memcpy_d2h(self.h, _ptr(arr), C.c_void_p(dptr.value + offset), arr.nbytes))

    def synchronize(self):
        check(self.lib.psdr_synchronize(self.h))

    def half_frame_bytes(self):
        return self.lib.psdr_half_frame_bytes(self.h)

    # --- batched path ---------------------------------------------------------------
    def process_batch(self, d_halves, nframes, offset_bytes=0):
        """d_halves: device pointer (ctypes.c_void_p or int) to nframes+1 raw half-frames."""
        base = d_halves.value if isinstance(d_halves, C.c_void_p) else int(d_halves)
        check(self.lib.psdr_process_batch(self.h, C.c_void_p(base + offset_bytes), nframes))
        self.last_nframes = nframes

    OPT_POST_CHAIN_STREAMS = 1
    OPT_POST_CHAIN_PCM16 = 3  # 1: the chain's PCM as int16 rows (half the bytes to the host; fetched_pcm16), 0 (default): int32 rows
    OPT_POST_CHAIN_AGC = 2  # 1 (default): chunk maxima + one kernel for the AGC where the rate allows it; 0: the five-kernel form
    OPT_WATERFALL_DETECTOR = 4  # WF_SAMPLE (default) / WF_PEAK / WF_MEAN: the detector of waterfall clients added from now on
    OPT_FINE_TUNE = 5  # 0 (default) / 1: the fine-tune flag of audio clients added from now on (AudioClient.set_fine_tune)
    OPT_SAM_SIDEBAND = 6  # SAM_BOTH (default) / SAM_UPPER / SAM_LOWER: the SAM sideband of audio clients added from now on
    OPT_AUTO_NOTCH = 7  # 0 (default) / 1: the auto-notch flag of audio clients added from now on (AudioClient.set_auto_notch)
    OPT_NOISE_REDUCTION = 9  # 0 (default) / NR_LIGHT / NR_NORMAL / NR_STRONG: the noise reduction of audio clients added from now on
    OPT_AUDIO_BLANKER = 10  # 0 (default) / ANB_LIGHT / ANB_NORMAL / ANB_STRONG: the audio blanker of audio clients added from now on

    def set_option(self, option, value):
        check(self.lib.psdr_set_option(self.h, int(option), int(value)))

    def set_post_chain(self, enable=True, measured_streams=None):
        """batched DC blocker + AGC + int16 conversion after every demod_batch.  measured_streams (first enable only): choose
        the chain's streams by measurement (psdr.h: PSDR_OPT_POST_CHAIN_STREAMS = 1) instead of creation order"""
        if measured_streams is not None and not getattr(self, "post_chain_on", False) and not getattr(self, "_pc_set_up", False):
            self.set_option(self.OPT_POST_CHAIN_STREAMS, 1 if measured_streams else 0)
        if enable:
            self._pc_set_up = True
        check(self.lib.psdr_set_post_chain(self.h, 1 if enable else 0))
        self.post_chain_on = bool(enable)

    def demod_batch(self, first_frame_num):
        check(self.lib.psdr_demod_batch(self.h, first_frame_num))
        self.last_demod_frames = self.last_nframes

    # --- the served end: results to pinned host memory (psdr_fetch_*) ------------------
    FETCH_AUDIO, FETCH_PCM, FETCH_WATERFALL = 1, 2, 4
    FETCH_IQ = 8  # the IQ rows of the batch's PSDR_IQ clients: one copy of the span of slots that hold them

    def fetch_batch(self):
        check(self.lib.psdr_fetch_batch(self.h))

    def fetch_begin(self, what=FETCH_AUDIO | FETCH_WATERFALL):
        """enqueue the device-to-host copies of the last demodulation / waterfall batch (returns at once)"""
        check(self.lib.psdr_fetch_begin(self.h, int(what)))

    def fetch_end(self):
        """wait for the oldest fetch in flight; fetched_audio / fetched_waterfall answer from it afterwards"""
        check(self.lib.psdr_fetch_end(self.h))

    def fetched_audio(self, cid, frame, pcm=False):
        """(audio[n/2] copy or None, pwr, nan flag[, pcm[n/2] copy or None]) of one frame of the fetched batch"""
        a, pc = C.POINTER(C.c_float)(), C.POINTER(C.c_int32)()
        pw, nan = C.c_float(0), C.c_int32(0)
        check(self.lib.psdr_fetched_audio(self.h, int(cid), int(frame), C.byref(a), C.byref(pw), C.byref(nan), C.byref(pc)))
        h = self.cfg.audio_fft_size // 2
        au = np.ctypeslib.as_array(a, shape=(h,)).copy() if a else None
        if not pcm:
            return au, pw.value, nan.value
        return au, pw.value, nan.value, (np.ctypeslib.as_array(pc, shape=(h,)).copy() if pc else None)

    def fetched_pcm16(self, cid, frame):
        """the int16 PCM row [n/2] (copy) of one frame of the fetched batch (OPT_POST_CHAIN_PCM16 = 1)"""
        pc = C.POINTER(C.c_int16)()
        check(self.lib.psdr_fetched_pcm16(self.h, int(cid), int(frame), C.byref(pc)))
        return np.ctypeslib.as_array(pc, shape=(self.cfg.audio_fft_size // 2,)).copy()

    def fetched_iq(self, cid, frame):
        """(iq complex64[n/2] copy or None, pwr, nan flag) of one frame of an IQ client in the fetched batch"""
        p = C.POINTER(C.c_float)()
        pw, nan = C.c_float(0), C.c_int32(0)
        check(self.lib.psdr_fetched_iq(self.h, int(cid), int(frame), C.byref(p), C.byref(pw), C.byref(nan)))
        iq = np.ctypeslib.as_array(p, shape=(self.cfg.audio_fft_size,)).copy().view(np.complex64) if p else None
        return iq, pw.value, nan.value

    def fetched_carrier(self, cid, frame):
        """(level, offset_hz) of one frame of a SAM client in the fetched batch (psdr.h: psdr_fetched_carrier)"""
        lv, off = C.c_float(0), C.c_float(0)
        check(self.lib.psdr_fetched_carrier(self.h, int(cid), int(frame), C.byref(lv), C.byref(off)))
        return lv.value, off.value

    def fetched_squelch(self, cid, frame):
        """1 / 0: one frame of the fetched batch is heard / squelched (psdr.h: psdr_fetched_squelch); 1 for a client without squelch"""
        o = C.c_int32(0)
        check(self.lib.psdr_fetched_squelch(self.h, int(cid), int(frame), C.byref(o)))
        return o.value

    def fetched_noise(self, cid, frame):
        """the window's noise power W of one frame of the fetched batch (psdr.h: psdr_fetched_noise); 0.0 for a client without
        the noise floor"""
        w = C.c_float(0)
        check(self.lib.psdr_fetched_noise(self.h, int(cid), int(frame), C.byref(w)))
        return w.value

    def fetched_iq_span(self):
        """(first slot, slots, bytes) the fetched batch's IQ copy covered (psdr.h: psdr_fetched_iq_span)"""
        lo, ns, nb = C.c_int(0), C.c_int(0), C.c_size_t(0)
        check(self.lib.psdr_fetched_iq_span(self.h, C.byref(lo), C.byref(ns), C.byref(nb)))
        return lo.value, ns.value, nb.value

    def fetched_waterfall(self, wid):
        """(rows [nsent][r - l] copy, level, l, r) of a waterfall client in the fetched batch"""
        rows = C.POINTER(C.c_int8)()
        ns, lv, l, r = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(self.lib.psdr_fetched_waterfall(self.h, int(wid), C.byref(rows), C.byref(ns), C.byref(lv), C.byref(l), C.byref(r)))
        ln = r.value - l.value
        if ns.value == 0 or ln == 0:
            return np.zeros((0, ln), np.int8), lv.value, l.value, r.value
        return np.ctypeslib.as_array(rows, shape=(ns.value, ln)).copy(), lv.value, l.value, r.value

    # --- streaming ingest (psdr_ring_*): pinned host half-frames -> HBM ring on a copy stream -----
    def ring_create(self, nhalves):
        check(self.lib.psdr_ring_create(self.h, int(nhalves)))

    def ring_write_async(self, half_index, host_half):
        """host_half: numpy array of one raw half-frame (ideally from pinned_array()); it must stay
        alive and unchanged until ring_wait(half_index) or a synchronising call returns."""
        assert host_half.nbytes == self.half_frame_bytes()
        check(self.lib.psdr_ring_write_async(self.h, int(half_index), _ptr(host_half)))

    def ring_wait(self, half_index):
        check(self.lib.psdr_ring_wait(self.h, int(half_index)))

    def process_ring(self, first_half, nframes):
        check(self.lib.psdr_process_ring(self.h, int(first_half), int(nframes)))
        self.last_nframes = nframes

    def ring_set_blanker(self, on, threshold_db=0.0, guard=0):
        """the impulse blanker on the ring, ahead of the FFT (psdr.h: psdr_ring_set_blanker); threshold_db is relative to the
        reference level R (the smallest block maximum of the half before), not to the mean power"""
        check(self.lib.psdr_ring_set_blanker(self.h, int(bool(on)), float(threshold_db), int(guard)))

    def ring_read_blanker(self, half_index):
        """(samples zeroed, R) of a half the last process_ring blanked, or None for any other half"""
        n, r = C.c_uint32(0), C.c_float(0.0)
        rc = self.lib.psdr_ring_read_blanker(self.h, int(half_index), C.byref(n), C.byref(r))
        if rc == -7:  # PSDR_ERR_NO_DATA
            return None
        check(rc)
        return n.value, np.float32(r.value)

    def ring_read(self, half_index, dtype=np.uint8):
        """the bytes of slot half_index % nhalves as the first pass reads them (drains first)"""
        out = np.empty(self.half_frame_bytes(), np.uint8)
        check(self.lib.psdr_ring_read(self.h, int(half_index), _ptr(out)))
        return out.view(dtype)

    def pinned_array(self, nbytes, dtype=np.uint8):
        """numpy view of pinned host memory from psdr_host_alloc (freed with the context)"""
        p = C.c_void_p()
        nfl = (nbytes + 3) // 4
        check(self.lib.psdr_host_alloc(self.h, nfl, C.byref(p)))
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p)
        return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p.value)).view(dtype)

    def waterfall_batch(self, first_frame_num):
        check(self.lib.psdr_waterfall_batch(self.h, first_frame_num))

    # --- band scan (psdr_scan_*): smoothed trace, segment noise floor, list of signals ----------
    def scan_set(self, level=None, avg_shift=3, threshold=12, gap=2):
        """the context's band scan (psdr.h: psdr_scan_set).  level None: off.  avg_shift 0..8: the trace's time constant is
        2^avg_shift frames; threshold 1..255 in counts of the int8 scale (0.5 dB each) above the segment floor; gap 0..64: cold
        bins that do not split a signal.  In force from the next scan_batch, which starts a new run."""
        if level is None:
            check(self.lib.psdr_scan_set(self.h, None))
            return
        cfg = _lib.psdr_scan_config(int(level), int(avg_shift), int(threshold), int(gap))
        check(self.lib.psdr_scan_set(self.h, C.byref(cfg)))

    def scan_batch(self, first_frame_num):
        """folds the batch processed just before into the trace and evaluates floors and signals (psdr_scan_batch)"""
        check(self.lib.psdr_scan_batch(self.h, first_frame_num))

    def read_signals(self, min_width=1):
        """(signals, total, frame_num): the kept signals at least min_width bins wide as a structured array (first, end,
        peak_bin, peak, floor; SIGNAL_DTYPE), the untruncated number of runs and the number of the last frame in the trace
        (psdr_read_signals); synchronises"""
        n, total, fn = C.c_int(0), C.c_int(0), C.c_uint64(0)
        check(self.lib.psdr_read_signals(self.h, int(min_width), None, 0, C.byref(n), C.byref(total), C.byref(fn)))
        out = np.zeros(n.value, SIGNAL_DTYPE)
        if n.value:
            check(self.lib.psdr_read_signals(self.h, int(min_width), _ptr(out), n.value, C.byref(n), C.byref(total), C.byref(fn)))
        return out, total.value, fn.value

    def read_scan_floor(self):
        """uint32[G]: the segments' floors F_g in 1/256 count above -128 (psdr_read_scan_floor)"""
        g = C.c_int(0)
        check(self.lib.psdr_read_scan_floor(self.h, None, 0, C.byref(g)))
        out = np.empty(g.value, np.uint32)
        check(self.lib.psdr_read_scan_floor(self.h, _ptr(out), g.value, C.byref(g)))
        return out

    def read_scan_trace(self):
        """uint16[n]: the trace s[j] in 1/256 count above -128 (psdr_read_scan_trace)"""
        n = C.c_size_t(0)
        check(self.lib.psdr_read_scan_trace(self.h, None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint16)
        check(self.lib.psdr_read_scan_trace(self.h, _ptr(out), n.value, C.byref(n)))
        return out

    def read_spectrum(self, frame):
        """complex64[nbins] in the reference's k order."""
        out = np.empty(self.nbins, np.complex64)
        check(self.lib.psdr_read_spectrum(self.h, frame, _ptr(out)))
        return out

    def read_quantized(self, frame):
        out = np.empty(self.q_len, np.int8)
        check(self.lib.psdr_read_quantized(self.h, frame, _ptr(out)))
        return out

    def quantized_level(self, q, i):
        off = sum(self.R >> t for t in range(i))
        return q[off:off + (self.R >> i)]

    # --- instrumentation ---------------------------------------------------------------
    def set_profiling(self, mode):
        """0 / False: off; 1 / True: hipEvent brackets around every launch; 2: device-clock stamps inside the
        two FFT passes (cheap enough for a timed region)"""
        check(self.lib.psdr_set_profiling(self.h, int(mode)))

    def kernel_samples(self, name):
        """per-launch durations (microseconds) of kernel `name` since the last reset"""
        n = C.c_int(0)
        check(self.lib.psdr_get_kernel_samples(self.h, name.encode(), None, 0, C.byref(n)))
        out = np.empty(max(n.value, 1), np.float64)
        check(self.lib.psdr_get_kernel_samples(self.h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_double)), n.value,
                                               C.byref(n)))
        return out[: n.value]

    def reset_kernel_stats(self):
        check(self.lib.psdr_reset_kernel_stats(self.h))

    def kernel_stats(self):
        names = (C.c_char_p * 32)()
        ms = (C.c_double * 32)()
        cnt = (C.c_int64 * 32)()
        n = C.c_int(0)
        check(self.lib.psdr_get_kernel_stats(self.h, 32, names, ms, cnt, C.byref(n)))
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(n.value)}

    def timer_start(self):
        check(self.lib.psdr_timer_start(self.h))

    def timer_stop_ms(self):
        ms = C.c_double(0)
        check(self.lib.psdr_timer_stop_ms(self.h, C.byref(ms)))
        return ms.value


class HipFFT:
    """The reference's FFT plug-in interface (src/fft.h:33-63) on the HIP back-end.

    Same call sequence as broadcast_server (src/spectrumserver.cpp:192-214, src/fft.cpp:17-30,
    61-98): ctor(size, nthreads, downsample_levels, brightness_offset),
    set_output_additional_size(A), plan_c2c()/plan_r2c(), malloc() x3,
    load_*_input(a1, a2), execute(), get_output_buffer(), get_quantized_buffer().
    """
    FORWARD, BACKWARD = 0, 1

    def __init__(self, size, nthreads=1, downsample_levels=1, brightness_offset=0, **ctx_kwargs):
        self.size = int(size)
        self.nthreads = nthreads  # CPU thread count of the FFTW sibling; unused on the GPU
        self.downsample_levels = downsample_levels
        self.brightness_offset = brightness_offset
        self.additional_size = 0
        self.ctx = None
        self._ctx_kwargs = ctx_kwargs
        self._bufs = {}

    def set_output_additional_size(self, size):
        self.additional_size = int(size)

    def _plan(self, is_real):
        assert self.ctx is None, "already planned"  # assert(!p), src/fft_impl.cpp:90,105
        self.ctx = Context(self.size, is_real, self.downsample_levels, self.brightness_offset,
                           self.additional_size, **self._ctx_kwargs)
        return 0

    def plan_c2c(self, direction=0, options=0):
        if direction != self.FORWARD:
            raise PsdrError(-6, "only FORWARD transforms are planned (src/fft.cpp:28)")
        return self._plan(False)

    def plan_r2c(self, options=0):
        return self._plan(True)

    def malloc(self, nfloats):
        """pinned host buffer as a float32 numpy view (FFT::malloc)."""
        assert self.ctx is not None, "plan first"
        p = C.c_void_p()
        check(self.ctx.lib.psdr_host_alloc(self.ctx.h, nfloats, C.byref(p)))
        arr = np.ctypeslib.as_array((C.c_float * nfloats).from_address(p.value))
        self._bufs[arr.ctypes.data] = p
        return arr

    def free(self, arr):
        p = self._bufs.pop(arr.ctypes.data)
        check(self.ctx.lib.psdr_host_free(self.ctx.h, p))

    def load_real_input(self, a1, a2):
        a1 = np.ascontiguousarray(a1, np.float32)
        a2 = np.ascontiguousarray(a2, np.float32)
        assert a1.size == self.size // 2 and a2.size == self.size // 2
        return check(self.ctx.lib.psdr_load_real_input(self.ctx.h, _ptr(a1), _ptr(a2)))

    def load_complex_input(self, a1, a2):
        a1 = np.ascontiguousarray(a1).view(np.float32)
        a2 = np.ascontiguousarray(a2).view(np.float32)
        assert a1.size == self.size and a2.size == self.size
        return check(self.ctx.lib.psdr_load_complex_input(self.ctx.h, _ptr(a1), _ptr(a2)))

    def execute(self):
        rc = check(self.ctx.lib.psdr_execute(self.ctx.h))
        self.ctx.last_nframes = 1
        return rc

    def get_output_buffer(self):
        """complex64 view: N+A bins (IQ) / N/2+1 bins (real), natural k order."""
        p = C.c_void_p()
        check(self.ctx.lib.psdr_get_output_buffer(self.ctx.h, C.byref(p)))
        nb = self.size // 2 + 1 if self.ctx.is_real else self.size + self.additional_size
        return np.ctypeslib.as_array((C.c_float * (2 * nb)).from_address(p.value)).view(np.complex64)

    def get_quantized_buffer(self):
        p = C.c_void_p()
        check(self.ctx.lib.psdr_get_quantized_buffer(self.ctx.h, C.byref(p)))
        return np.ctypeslib.as_array((C.c_int8 * self.ctx.q_len).from_address(p.value))

    def close(self):
        if self.ctx is not None:
            for p in list(self._bufs.values()):
                self.ctx.lib.psdr_host_free(self.ctx.h, p)
            self._bufs.clear()
            self.ctx.close()
            self.ctx = None


class AudioClient:
    """AudioClient (src/signal.h:53-123): one tuned demodulator channel on a Context."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        cid = C.c_int(-1)
        check(ctx.lib.psdr_client_add(ctx.h, C.byref(cid)))
        self.id = cid.value
        self.l = self.r = 0
        self.audio_mid = 0.0
        self.demodulation = USB

    def set_audio_range(self, l, audio_mid, r):
        check(self.ctx.lib.psdr_client_set_audio_range(self.ctx.h, self.id, int(l), float(audio_mid), int(r)))
        self.l, self.audio_mid, self.r = int(l), float(audio_mid), int(r)

    def set_audio_demodulation(self, demodulation):
        mode = MODES[demodulation] if isinstance(demodulation, str) else int(demodulation)
        check(self.ctx.lib.psdr_client_set_audio_demodulation(self.ctx.h, self.id, mode))
        self.demodulation = mode

    def set_paused(self, paused):
        """signal_loop's slow-client rule (src/websocket.cpp:170-176): a paused client gets no send_audio call -
        it sits out the demodulation batches with all of its state frozen."""
        check(self.ctx.lib.psdr_client_set_paused(self.ctx.h, self.id, 1 if paused else 0))

    def set_fine_tune(self, on):
        """tuning below one FFT bin (psdr_client_set_fine_tune): with the flag on, a USB / LSB / IQ client's fraction
        audio_mid - floor(audio_mid) is taken out by a rotator at the audio rate; AM / FM / SAM are not affected."""
        check(self.ctx.lib.psdr_client_set_fine_tune(self.ctx.h, self.id, 1 if on else 0))

    def set_sam_sideband(self, sideband):
        """selectable-sideband synchronous AM (psdr_client_set_sam_sideband): "both" (default), "upper" or "lower" - in SAM
        mode only that sideband is detected against the carrier recovered from the whole window; no effect in other modes."""
        sb = SAM_SIDEBANDS[sideband] if isinstance(sideband, str) else int(sideband)
        check(self.ctx.lib.psdr_client_set_sam_sideband(self.ctx.h, self.id, sb))

    def set_notch(self, index, centre_bin, width_bins):
        """manual notch `index` (0 or 1) on the spectrum bins around centre_bin (psdr_client_set_notch): the client's kernels
        take those bins as zero; width_bins <= 0 clears the entry.  Takes force at the next batch."""
        check(self.ctx.lib.psdr_client_set_notch(self.ctx.h, self.id, int(index), float(centre_bin), float(width_bins)))

    def set_auto_notch(self, on):
        """automatic notches (psdr_client_set_auto_notch): every half second the detector behind the batches notches up to two
        steady carriers that stand 16 times above the window's mean power."""
        check(self.ctx.lib.psdr_client_set_auto_notch(self.ctx.h, self.id, 1 if on else 0))

    def notches(self):
        """[(first, end)] x 4 of the last batch (psdr_read_notches): entries 0..1 manual, 2..3 automatic; (0, 0) = empty"""
        first, end = (C.c_int * 4)(), (C.c_int * 4)()
        check(self.ctx.lib.psdr_read_notches(self.ctx.h, self.id, first, end))
        return [(first[k], end[k]) for k in range(4)]

    def set_squelch(self, on, open_db=0.0, close_db=None, attack_frames=1, hang_frames=0):
        """level gate with hysteresis (psdr_client_set_squelch): the client opens after attack_frames consecutive frames whose
        pwr is at least 10^(open_db/10) and closes after more than hang_frames consecutive frames below 10^(close_db/10)
        (close_db None: open_db, no hysteresis).  A closed frame stays out of the post chain's stream like a NaN-flagged one;
        the demodulated rows are not touched.  Switching it on starts from closed; in force from the next batch."""
        close_db = open_db if close_db is None else close_db
        check(self.ctx.lib.psdr_client_set_squelch(self.ctx.h, self.id, 1 if on else 0, float(open_db), float(close_db),
                                                   int(attack_frames), int(hang_frames)))

    def read_squelch(self, nframes=None):
        """open[F] (int32, 1 = heard) of the last demod batch (psdr.h: psdr_read_squelch); all 1 for a client without squelch"""
        F = nframes or self.ctx.last_demod_frames or self.ctx.last_nframes
        o = np.empty(F, np.int32)
        got = C.c_int(0)
        check(self.ctx.lib.psdr_read_squelch(self.ctx.h, self.id, F, _ptr(o), C.byref(got)))
        return o[:got.value]

    def set_noise_floor(self, on):
        """noise floor of the client's window (psdr_client_set_noise_floor): behind every batch the device estimates the
        window's noise power W per frame - the lower quartile of the bins' power sums, the minimum over the last 8 evaluations -
        for an SNR (pwr / W) and for a squelch set in dB above the noise.  Starts from zero when switched on and on a retune."""
        check(self.ctx.lib.psdr_client_set_noise_floor(self.ctx.h, self.id, 1 if on else 0))

    def set_squelch_reference(self, ref):
        """what the squelch's thresholds are relative to (psdr_client_set_squelch_reference): "absolute" (default) or "noise" -
        dB above the noise floor's W, for a client whose noise floor is on.  The gate's state is kept."""
        ref = SQUELCH_REFERENCES[ref] if isinstance(ref, str) else int(ref)
        check(self.ctx.lib.psdr_client_set_squelch_reference(self.ctx.h, self.id, ref))

    def read_noise(self, nframes=None):
        """W[F] (float32), the window's noise power per frame of the last demod batch (psdr.h: psdr_read_noise); all 0 for a
        client without the noise floor"""
        F = nframes or self.ctx.last_demod_frames or self.ctx.last_nframes
        w = np.empty(F, np.float32)
        got = C.c_int(0)
        check(self.ctx.lib.psdr_read_noise(self.ctx.h, self.id, F, _ptr(w), C.byref(got)))
        return w[:got.value]

    def set_audio_filter(self, sections):
        """biquad sections behind the detector (psdr_client_set_audio_filter): a list of one or two (b0, b1, b2, a1, a2), for
        instance from design_audio_filter(); the empty list switches the filter off.  The client's audio rows are filtered in
        place from its next batch on; the state starts from zero with every call that sets sections."""
        sections = [tuple(float(v) for v in s) for s in sections]
        if any(len(s) != 5 for s in sections):
            raise ValueError("a section is (b0, b1, b2, a1, a2)")
        arr = (_lib.psdr_biquad * max(len(sections), 1))(*[_lib.psdr_biquad(*s) for s in sections])
        check(self.ctx.lib.psdr_client_set_audio_filter(self.ctx.h, self.id, len(sections), C.cast(arr, C.c_void_p) if sections else None))

    def set_noise_reduction(self, kind, depth_db=None, beta=None):
        """spectral noise reduction on the client's audio rows, in front of the audio filter and the post chain
        (psdr_client_set_noise_reduction).  `kind`: None - off -, a preset name ("light", "normal", "strong") or an NR_*
        constant; depth_db (0..40, the deepest attenuation) and beta (0.5..4, the over-subtraction) replace the preset's
        numbers.  The rows are delayed by 256 samples; the state starts from zero with every call that switches it on."""
        if kind is None:
            check(self.ctx.lib.psdr_client_set_noise_reduction(self.ctx.h, self.id, 0, 0.0, 0.0))
            return
        d, b = noise_reduction_preset(kind)
        check(self.ctx.lib.psdr_client_set_noise_reduction(self.ctx.h, self.id, 1, float(d if depth_db is None else depth_db),
                                                           float(b if beta is None else beta)))

    def set_audio_blanker(self, kind, threshold=None, width=None):
        """impulse blanker on the client's audio rows, in front of the noise reduction, the audio filter and the post chain
        (psdr_client_set_audio_blanker).  `kind`: None - off -, a preset name ("light", "normal", "strong") or an ANB_* constant;
        threshold (2..12, in standard deviations of the whitened block) and width (odd, 3..15, the samples cut out per impulse)
        replace the preset's numbers.  The rows are delayed by 536 samples; the state starts from zero with every call that
        switches it on."""
        if kind is None:
            check(self.ctx.lib.psdr_client_set_audio_blanker(self.ctx.h, self.id, 0, 0.0, 0))
            return
        t, w = audio_blanker_preset(kind)
        check(self.ctx.lib.psdr_client_set_audio_blanker(self.ctx.h, self.id, 1, float(t if threshold is None else threshold),
                                                         int(w if width is None else width)))

    def audio_blanker_counts(self):
        """(impulses, samples): what the client's audio blanker found and rewrote since its state last started from zero
        (psdr_read_audio_blanker); synchronises"""
        n, s = C.c_uint64(0), C.c_uint64(0)
        check(self.ctx.lib.psdr_read_audio_blanker(self.ctx.h, self.id, C.byref(n), C.byref(s)))
        return n.value, s.value

    def set_tone_decoder(self, on=True, **fields):
        """sub-audible tone detection and tone squelch on the client's audio rows as the demodulator wrote them
        (psdr_client_set_tone_decoder).  on false or None: off.  Keyword arguments replace single fields of tone_defaults() at
        the context's audio_rate: want (0..49 or TONE_ANY), gate (1: a closed frame stays out of the post chain), snr_db,
        min_level, attack_blocks, hang_blocks.  The state starts from zero with every call that switches it on."""
        if not on:
            check(self.ctx.lib.psdr_client_set_tone_decoder(self.ctx.h, self.id, None))
            return
        p = _lib.psdr_tone_config(want=TONE_ANY, gate=1, snr_db=22.0, min_level=0.0, attack_blocks=2, hang_blocks=0)
        # (a rate outside the decoder's range is the call's refusal to make, not the defaults')
        if self.ctx.lib.psdr_tone_defaults(float(self.ctx.cfg.audio_rate), C.byref(p)) != 0:
            p.hang_blocks = 0
        for k, v in fields.items():
            if k not in ("want", "gate", "snr_db", "min_level", "attack_blocks", "hang_blocks"):
                raise TypeError("set_tone_decoder: unknown field %r" % k)
            setattr(p, k, float(v) if k in ("snr_db", "min_level") else int(v))
        check(self.ctx.lib.psdr_client_set_tone_decoder(self.ctx.h, self.id, C.byref(p)))

    def read_tone(self, nframes=None):
        """(tone[F] int32, level[F] float32, open[F] int32) of the last demod batch (psdr.h: psdr_read_tone): per frame the tone's
        number or -1, the squared amplitude the last decision measured, and the tone gate"""
        F = nframes or self.ctx.last_demod_frames or self.ctx.last_nframes
        t, lv, o = np.empty(F, np.int32), np.empty(F, np.float32), np.empty(F, np.int32)
        got = C.c_int(0)
        check(self.ctx.lib.psdr_read_tone(self.ctx.h, self.id, F, _ptr(t), _ptr(lv), _ptr(o), C.byref(got)))
        return t[:got.value], lv[:got.value], o[:got.value]

    def set_cw_decoder(self, on=True, **fields):
        """Morse text, speed and pitch from the client's audio rows as the demodulator wrote them (psdr_client_set_cw_decoder).
        on false or None: off.  Keyword arguments replace single fields of cw_defaults(): pitch_hz, search_hz, wpm, track_speed,
        snr_db.  The state and the text start from zero with every call that switches it on."""
        if not on:
            check(self.ctx.lib.psdr_client_set_cw_decoder(self.ctx.h, self.id, None))
            return
        p = _lib.psdr_cw_config(pitch_hz=700.0, search_hz=100.0, wpm=20.0, track_speed=1, snr_db=22.0)
        for k, v in fields.items():
            if k not in CW_FIELDS:
                raise TypeError("set_cw_decoder: unknown field %r" % k)
            setattr(p, k, int(v) if k == "track_speed" else float(v))
        check(self.ctx.lib.psdr_client_set_cw_decoder(self.ctx.h, self.id, C.byref(p)))

    def read_cw(self, nframes=None):
        """(nchars[F] uint32, wpm[F] float32, pitch_hz[F] float32, level[F] float32, key[F] int32) of the last demod batch (psdr.h:
        psdr_read_cw): per frame the text's length so far, the speed the dot length stands at, the followed lane's pitch, the
        squared amplitude of the peak, and the debounced key"""
        F = nframes or self.ctx.last_demod_frames or self.ctx.last_nframes
        n, w, p, lv, k = np.empty(F, np.uint32), np.empty(F, np.float32), np.empty(F, np.float32), np.empty(F, np.float32), np.empty(F, np.int32)
        got = C.c_int(0)
        check(self.ctx.lib.psdr_read_cw(self.ctx.h, self.id, F, _ptr(n), _ptr(w), _ptr(p), _ptr(lv), _ptr(k), C.byref(got)))
        g = got.value
        return n[:g], w[:g], p[:g], lv[:g], k[:g]

    def read_cw_text(self, since=0):
        """(text, total): the characters since .. total - 1 of the client's text since the decoder's state last started
        (psdr_read_cw_text); the device keeps the last 1024"""
        buf = C.create_string_buffer(1024)
        n, total = C.c_size_t(0), C.c_uint64(0)
        check(self.ctx.lib.psdr_read_cw_text(self.ctx.h, self.id, int(since), buf, 1024, C.byref(n), C.byref(total)))
        return buf.raw[:n.value].decode("ascii"), total.value

    def set_rtty_decoder(self, on=True, **fields):
        """Baudot text and tuning offset from the client's audio rows as the demodulator wrote them (psdr_client_set_rtty_decoder).
        on false or None: off.  Keyword arguments replace single fields of rtty_defaults() at the context's audio_rate: mark_hz,
        shift_hz (negative: reverse), baud, usos, search_hz, snr_db.  The state and the text start from zero with every call that
        switches it on."""
        if not on:
            check(self.ctx.lib.psdr_client_set_rtty_decoder(self.ctx.h, self.id, None))
            return
        p = _lib.psdr_rtty_config(mark_hz=2125.0, shift_hz=170.0, baud=45.45, usos=1, search_hz=60.0, snr_db=0.0)
        # (a rate outside the decoder's range is the call's refusal to make, not the defaults')
        if self.ctx.lib.psdr_rtty_defaults(float(self.ctx.cfg.audio_rate), C.byref(p)) != 0:
            p.snr_db = 7.5
        for k, v in fields.items():
            if k not in RTTY_FIELDS:
                raise TypeError("set_rtty_decoder: unknown field %r" % k)
            setattr(p, k, int(v) if k == "usos" else float(v))
        check(self.ctx.lib.psdr_client_set_rtty_decoder(self.ctx.h, self.id, C.byref(p)))

    def read_rtty(self, nframes=None):
        """(nchars[F] uint32, errors[F] uint32, offset_hz[F] float32, level[F] float32, quality[F] float32, present[F] int32) of the
        last demod batch (psdr.h: psdr_read_rtty): per frame the text's length so far, the framing errors so far, the followed
        pair's offset from the configured tones, the squared amplitude of the stronger tone, T / Nn, and the presence flag"""
        F = nframes or self.ctx.last_demod_frames or self.ctx.last_nframes
        n, e, o = np.empty(F, np.uint32), np.empty(F, np.uint32), np.empty(F, np.float32)
        lv, q, pr = np.empty(F, np.float32), np.empty(F, np.float32), np.empty(F, np.int32)
        got = C.c_int(0)
        check(self.ctx.lib.psdr_read_rtty(self.ctx.h, self.id, F, _ptr(n), _ptr(e), _ptr(o), _ptr(lv), _ptr(q), _ptr(pr), C.byref(got)))
        g = got.value
        return n[:g], e[:g], o[:g], lv[:g], q[:g], pr[:g]

    def read_rtty_text(self, since=0):
        """(text, total): the characters since .. total - 1 of the client's text since the decoder's state last started
        (psdr_read_rtty_text); the device keeps the last 1024"""
        buf = C.create_string_buffer(1024)
        n, total = C.c_size_t(0), C.c_uint64(0)
        check(self.ctx.lib.psdr_read_rtty_text(self.ctx.h, self.id, int(since), buf, 1024, C.byref(n), C.byref(total)))
        return buf.raw[:n.value].decode("ascii"), total.value

    def set_psk_decoder(self, on=True, **fields):
        """varicode text and tuning offset of a BPSK31 / BPSK63 signal from the client's audio rows as the demodulator wrote them
        (psdr_client_set_psk_decoder).  on false or None: off.  Keyword arguments replace single fields of psk_defaults() at the
        context's audio_rate: carrier_hz, baud (31.25 or 62.5), search_hz, quality; a baud without a search_hz searches three lanes
        to either side at that speed.  The state and the text start from zero with every call that switches it on."""
        if not on:
            check(self.ctx.lib.psdr_client_set_psk_decoder(self.ctx.h, self.id, None))
            return
        p = _lib.psdr_psk_config(carrier_hz=1000.0, baud=31.25, search_hz=11.71875, quality=0.0)
        # (a rate outside the decoder's range is the call's refusal to make, not the defaults')
        if self.ctx.lib.psdr_psk_defaults(float(self.ctx.cfg.audio_rate), C.byref(p)) != 0:
            p.quality = 0.51
        for k, v in fields.items():
            if k not in PSK_FIELDS:
                raise TypeError("set_psk_decoder: unknown field %r" % k)
            setattr(p, k, float(v))
        if "baud" in fields and "search_hz" not in fields:
            p.search_hz = 3.0 * p.baud / 8.0
        check(self.ctx.lib.psdr_client_set_psk_decoder(self.ctx.h, self.id, C.byref(p)))

    def read_psk(self, nframes=None):
        """(nchars[F] uint32, errors[F] uint32, offset_hz[F] float32, level[F] float32, quality[F] float32, present[F] int32) of the
        last demod batch (psdr.h: psdr_read_psk): per frame the text's length so far, the varicode errors so far, the followed
        lane's offset from the configured carrier, the squared amplitude at the sample points, the coherence, and the presence flag"""
        F = nframes or self.ctx.last_demod_frames or self.ctx.last_nframes
        n, e, o = np.empty(F, np.uint32), np.empty(F, np.uint32), np.empty(F, np.float32)
        lv, q, pr = np.empty(F, np.float32), np.empty(F, np.float32), np.empty(F, np.int32)
        got = C.c_int(0)
        check(self.ctx.lib.psdr_read_psk(self.ctx.h, self.id, F, _ptr(n), _ptr(e), _ptr(o), _ptr(lv), _ptr(q), _ptr(pr), C.byref(got)))
        g = got.value
        return n[:g], e[:g], o[:g], lv[:g], q[:g], pr[:g]

    def read_psk_text(self, since=0):
        """(text, total): the characters since .. total - 1 of the client's text since the decoder's state last started
        (psdr_read_psk_text); the device keeps the last 1024"""
        buf = C.create_string_buffer(1024)
        n, total = C.c_size_t(0), C.c_uint64(0)
        check(self.ctx.lib.psdr_read_psk_text(self.ctx.h, self.id, int(since), buf, 1024, C.byref(n), C.byref(total)))
        return buf.raw[:n.value].decode("ascii"), total.value

    def set_fax_decoder(self, on=True, **fields):
        """the image lines of the HF radiofax in the client's audio rows as the demodulator wrote them
        (psdr_client_set_fax_decoder).  on false or None: off.  Keyword arguments replace single fields of fax_defaults(): mode
        (FAX_AUTO, FAX_FREE), black_hz, white_hz, lpm, width, slant_ppm, phase_col, tone_ratio, start_blocks, phase_lines,
        max_lines.  The state and the lines start from zero with every call that switches it on."""
        if not on:
            check(self.ctx.lib.psdr_client_set_fax_decoder(self.ctx.h, self.id, None))
            return
        p = _lib.psdr_fax_config()
        # (a rate outside the decoder's range is the call's refusal to make, not the defaults')
        if self.ctx.lib.psdr_fax_defaults(float(self.ctx.cfg.audio_rate), C.byref(p)) != 0:
            self.ctx.lib.psdr_fax_defaults(12000.0, C.byref(p))
        for k, v in fields.items():
            if k not in FAX_FIELDS:
                raise TypeError("set_fax_decoder: unknown field %r" % k)
            setattr(p, k, int(v) if k in FAX_INT_FIELDS else float(v))
        check(self.ctx.lib.psdr_client_set_fax_decoder(self.ctx.h, self.id, C.byref(p)))

    def read_fax(self, nframes=None):
        """(nlines[F] uint32, state[F] int32, image[F] uint32, ioc[F] int32, offset_hz[F] float32, tone_quality[F] float32) of the
        last demod batch (psdr.h: psdr_read_fax): per frame the kept lines so far, the machine's state (0 idle, 1 phasing, 2
        image), the image's serial, its index of cooperation, the mistuning read off the start and stop tones, the last tone
        block's largest rho"""
        F = nframes or self.ctx.last_demod_frames or self.ctx.last_nframes
        n, s, im = np.empty(F, np.uint32), np.empty(F, np.int32), np.empty(F, np.uint32)
        io, o, q = np.empty(F, np.int32), np.empty(F, np.float32), np.empty(F, np.float32)
        got = C.c_int(0)
        check(self.ctx.lib.psdr_read_fax(self.ctx.h, self.id, F, _ptr(n), _ptr(s), _ptr(im), _ptr(io), _ptr(o), _ptr(q), C.byref(got)))
        g = got.value
        return n[:g], s[:g], im[:g], io[:g], o[:g], q[:g]

    def read_fax_lines(self, from_=0):
        """(lines uint8 [n, width], meta uint32 [n], total): the kept lines from_ .. total - 1 since the decoder's state last started
        (psdr_read_fax_lines); the device keeps the last 64 at least.  meta: the image's serial << 8 | the state the line was
        taken in"""
        n, total, width = C.c_size_t(0), C.c_uint64(0), C.c_int(0)
        check(self.ctx.lib.psdr_read_fax_lines(self.ctx.h, self.id, int(from_), None, None, 0, C.byref(n), C.byref(total), C.byref(width)))
        cap = max(0, total.value - int(from_))
        pix, meta = np.empty((cap, max(width.value, 1)), np.uint8), np.empty(cap, np.uint32)
        if cap:
            check(self.ctx.lib.psdr_read_fax_lines(self.ctx.h, self.id, int(from_), _ptr(pix), _ptr(meta), cap, C.byref(n), C.byref(total), C.byref(width)))
        return pix[:n.value], meta[:n.value], total.value

    def set_agc_profile(self, profile, **fields):
        """the client's own AGC numbers in the post chain (psdr_client_set_agc_profile).  `profile`: None - back to the context's
        AGC -, a preset name ("reference", "fast", "slow") or a dict like agc_preset()'s; keyword arguments replace single fields
        of it: desired, attack_ms, release_ms, max_gain (a cap on the wanted gain, 0: none), manual (True: the gain glides to
        manual_gain and stays).  Nothing of the chain's state is reset; in force from the client's next batch."""
        if profile is None and not fields:
            check(self.ctx.lib.psdr_client_set_agc_profile(self.ctx.h, self.id, None))
            return
        f = agc_preset(profile if isinstance(profile, (str, int)) else AGC_REFERENCE)
        if isinstance(profile, dict):
            f.update(profile)
        unknown = set(fields) - set(f)
        if unknown:
            raise TypeError(f"unknown AGC profile fields {sorted(unknown)}")
        f.update(fields)
        p = _lib.psdr_agc_profile(float(f["desired"]), float(f["attack_ms"]), float(f["release_ms"]), float(f["max_gain"]),
                                  int(f["manual"]), float(f["manual_gain"]))
        check(self.ctx.lib.psdr_client_set_agc_profile(self.ctx.h, self.id, C.byref(p)))

    def read_agc_gain(self):
        """the gain the client's last post chain batch left behind (psdr_read_agc_gain); synchronises"""
        g = C.c_float(0)
        check(self.ctx.lib.psdr_read_agc_gain(self.ctx.h, self.id, C.byref(g)))
        return np.float32(g.value)

    def on_window_message(self, l, m, r):
        """returns False where the reference silently returns (src/signal.cpp:302-311)."""
        if m is None:
            return False
        rc = self.ctx.lib.psdr_client_on_window_message(self.ctx.h, self.id, int(l), float(m), int(r))
        if rc == -1:
            return False
        check(rc)
        self.l, self.audio_mid, self.r = int(l), float(m), int(r)
        return True

    def on_demodulation_message(self, demodulation: str):
        if demodulation in MODES:  # unknown strings leave the mode alone (src/signal.cpp:318-326)
            self.set_audio_demodulation(demodulation)

    def read_audio(self, nframes=None):
        """(audio[F][n/2], pwr[F], nan[F]) of the last demod batch (F = its frame count; `nframes`,
        if given, is the number of rows to allocate and must not be smaller)."""
        F = nframes or self.ctx.last_demod_frames or self.ctx.last_nframes
        h = self.ctx.n // 2
        audio = np.empty((F, h), np.float32)
        pwr = np.empty(F, np.float32)
        nan = np.empty(F, np.int32)
        got = C.c_int(0)
        check(self.ctx.lib.psdr_read_audio(self.ctx.h, self.id, F, _ptr(audio), _ptr(pwr), _ptr(nan), C.byref(got)))
        return audio[:got.value], pwr[:got.value], nan[:got.value]

    def read_iq(self, nframes=None):
        """(iq complex64[F][n/2], pwr[F], nan[F]) of the last demod batch of a client in IQ mode (psdr.h: psdr_read_iq)"""
        F = nframes or self.ctx.last_demod_frames or self.ctx.last_nframes
        iq = np.empty((F, self.ctx.n // 2), np.complex64)
        pwr = np.empty(F, np.float32)
        nan = np.empty(F, np.int32)
        got = C.c_int(0)
        check(self.ctx.lib.psdr_read_iq(self.ctx.h, self.id, F, _ptr(iq), _ptr(pwr), _ptr(nan), C.byref(got)))
        return iq[:got.value], pwr[:got.value], nan[:got.value]

    def read_carrier(self, nframes=None):
        """(level[F], offset_hz[F]) of the last demod batch of a client in SAM mode (psdr.h: psdr_read_carrier)"""
        F = nframes or self.ctx.last_demod_frames or self.ctx.last_nframes
        level = np.empty(F, np.float32)
        off = np.empty(F, np.float32)
        got = C.c_int(0)
        check(self.ctx.lib.psdr_read_carrier(self.ctx.h, self.id, F, _ptr(level), _ptr(off), C.byref(got)))
        return level[:got.value], off[:got.value]

    def read_pcm(self, nframes=None):
        """int16 PCM (in int32, like the reference's buffer) of the last demod batch after the
        DC blocker / AGC / int16 conversion (src/signal.cpp:277-284); needs
        Context.set_post_chain(True)."""
        F = nframes or self.ctx.last_demod_frames or self.ctx.last_nframes
        pcm = np.empty((F, self.ctx.n // 2), np.int32)
        got = C.c_int(0)
        check(self.ctx.lib.psdr_read_pcm(self.ctx.h, self.id, F, _ptr(pcm), C.byref(got)))
        return pcm[:got.value]

    def on_close(self):
        if self.id >= 0 and self.ctx.h:
            check(self.ctx.lib.psdr_client_remove(self.ctx.h, self.id))
            self.id = -1


class WaterfallClient:
    """WaterfallClient (src/waterfall.h): a [level, l, r) window on the int8 pyramid."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        wid = C.c_int(-1)
        check(ctx.lib.psdr_waterfall_add(ctx.h, C.byref(wid)))
        self.id = wid.value
        self.level = ctx.levels - 1
        mwf = ctx.cfg.waterfall_size or (ctx.R >> self.level)
        self.l, self.r = 0, min(mwf, ctx.R >> self.level)

    def set_waterfall_range(self, level, l, r):
        check(self.ctx.lib.psdr_waterfall_set_range(self.ctx.h, self.id, int(level), int(l), int(r)))
        self.level, self.l = int(level), max(0, int(l))
        self.r = min(int(r), self.ctx.R >> self.level)

    def set_detector(self, detector):
        """"sample" (the reference's waterfall, the default), "peak" (max-hold) or "mean" (mean of the dB values) over the
        frames a sent row stands for (psdr.h: psdr_wf_detector); in force from the next waterfall_batch on"""
        det = WF_DETECTORS[detector] if isinstance(detector, str) else int(detector)
        check(self.ctx.lib.psdr_waterfall_set_detector(self.ctx.h, self.id, det))
        self.detector = det

    def on_window_message(self, l, r):
        lv, nl, nr = C.c_int(), C.c_int(), C.c_int()
        rc = self.ctx.lib.psdr_waterfall_on_window_message(self.ctx.h, self.id, int(l), int(r),
                                                           C.byref(lv), C.byref(nl), C.byref(nr))
        if rc == -1:
            return False
        check(rc)
        self.level, self.l, self.r = lv.value, nl.value, nr.value
        return True

    def read_waterfall(self):
        """int8[nsent][r-l] for the frames of the last waterfall batch that were sent, plus
        the (l << level, r << level) labels of send_waterfall (src/waterfall.cpp:47).  Row length
        and labels are those of the BATCH (the window may have moved since)."""
        ns, lv, l, r = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        lib, h = self.ctx.lib, self.ctx.h
        check(lib.psdr_read_waterfall(h, self.id, None, 0, C.byref(ns), C.byref(lv), C.byref(l), C.byref(r)))
        ln = r.value - l.value
        cap = max(1, ns.value * ln)
        out = np.empty(cap, np.int8)
        check(lib.psdr_read_waterfall(h, self.id, _ptr(out), cap, C.byref(ns), C.byref(lv), C.byref(l), C.byref(r)))
        ln = r.value - l.value
        return out[: ns.value * ln].reshape(ns.value, ln), (l.value << lv.value, r.value << lv.value)

    def on_close(self):
        if self.id >= 0 and self.ctx.h:
            check(self.ctx.lib.psdr_waterfall_remove(self.ctx.h, self.id))
            self.id = -1


class Group:
    """psdr_group (include/psdr.h): one process, n GPUs, the batch exchanged over xGMI through RCCL called from C.
    shard: "clients" | "raw" | "band"; force_comm: issue the collectives even with one device (testing); peer_copy: no
    RCCL, the peers pull with hipMemcpyPeerAsync (a device may then be listed more than once)."""
    SHARDS = {"clients": 0, "raw": 1, "band": 2}

    def __init__(self, devices, shard, fft_size, is_real, downsample_levels, force_comm=False, peer_copy=False, serial=False, **ctx_kwargs):
        # a throw-away Context object only to build the psdr_config the same way Context does
        self.lib = _lib.load()
        cfg = Context._config(fft_size, is_real, downsample_levels, **ctx_kwargs)
        devs = (C.c_int * len(devices))(*devices)
        self.h = C.c_void_p()
        # serial: PSDR_SHARD_SERIAL - exchange and transform one after the other (default: the exchange of batch b beside the transform of b + 1)
        flag = self.SHARDS[shard] | (0x100 if force_comm else 0) | (0x200 if peer_copy else 0) | (0x400 if serial else 0)
        check(self.lib.psdr_group_create(C.byref(cfg), devs, len(devices), flag, C.byref(self.h)))
        self.n = len(devices)
        self.cfg = cfg
        self.h_audio = cfg.audio_fft_size // 2
        self.root = Context._view(self.lib, self.lib.psdr_group_ctx(self.h, 0), cfg)

    def client_add(self, l, mid, r, mode):
        gid = C.c_int(-1)
        mode = MODES[mode] if isinstance(mode, str) else int(mode)
        check(self.lib.psdr_group_client_add(self.h, int(l), float(mid), int(r), mode, C.byref(gid)))
        return gid.value

    def client_set_audio_range(self, gid, l, mid, r):
        """(band sharding may move the client to another device behind its gid, which stays what it is)"""
        check(self.lib.psdr_group_client_set_audio_range(self.h, int(gid), int(l), float(mid), int(r)))
        return gid

    def client_rank(self, gid):
        return int(self.lib.psdr_group_client_rank(self.h, int(gid)))

    def ctx_view(self, rank):
        """the context of `rank` (psdr_group_ctx), owned by the group"""
        return Context._view(self.lib, self.lib.psdr_group_ctx(self.h, int(rank)), self.cfg)

    def client_set_paused(self, gid, paused):
        check(self.lib.psdr_group_client_set_paused(self.h, gid, 1 if paused else 0))

    def step(self, d_halves, nframes, first_frame_num, offset_bytes=0):
        base = d_halves.value if isinstance(d_halves, C.c_void_p) else int(d_halves)
        check(self.lib.psdr_group_step(self.h, C.c_void_p(base + offset_bytes), nframes, first_frame_num))
        self.root.last_nframes = self.root.last_demod_frames = nframes

    def step_ring(self, first_half, nframes, first_frame_num):
        check(self.lib.psdr_group_step_ring(self.h, first_half, nframes, first_frame_num))
        self.root.last_nframes = self.root.last_demod_frames = nframes

    def synchronize(self):
        check(self.lib.psdr_group_synchronize(self.h))

    def fetch(self):
        check(self.lib.psdr_group_fetch(self.h))

    def fetched_audio(self, gid, frame):
        """(audio[n/2] copy, pwr, nan flag) of one frame of the fetched batch"""
        a = C.POINTER(C.c_float)()
        pw, nan = C.c_float(0), C.c_int32(0)
        check(self.lib.psdr_group_fetched_audio(self.h, gid, frame, C.byref(a), C.byref(pw), C.byref(nan), None))
        return np.ctypeslib.as_array(a, shape=(self.h_audio,)).copy(), pw.value, nan.value

    def link_stats(self):
        b, ms = C.c_double(0), C.c_double(0)
        check(self.lib.psdr_group_link_stats(self.h, C.byref(b), C.byref(ms)))
        return b.value, ms.value

    def close(self):
        if self.h:
            self.lib.psdr_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SpectrumEngine:
    """The frame loop of broadcast_server::fft_task (src/fft.cpp:47-105) over a raw sample
    ring that lives in HBM, batched F frames per launch, with the signal_loop /
    waterfall_loop fan-out (src/websocket.cpp:156-185,207-236) executed on the GPU."""

    def __init__(self, sps, fft_size, is_real, input_format="s16", audio_sps=12000,
                 waterfall_size=1024, brightness_offset=0, max_batch=16, max_clients=256,
                 max_waterfall_clients=64, device=0):
        p = derived_params(sps, fft_size, is_real, audio_sps, waterfall_size)
        self.params = p
        self.sps, self.fft_size, self.is_real = sps, fft_size, bool(is_real)
        self.input_format = input_format
        self.ctx = Context(fft_size, is_real, p["downsample_levels"], brightness_offset,
                           additional_size=p["audio_fft_size"], audio_fft_size=p["audio_fft_size"],
                           audio_rate=audio_sps, input_format=input_format, device=device,
                           max_batch=max_batch, max_clients=max_clients,
                           max_waterfall_clients=max_waterfall_clients, skip_num=p["skip_num"],
                           waterfall_size=waterfall_size)
        self.frame_num = 0
        self.audio_clients = []
        self.waterfall_clients = []
        self.ring = None
        self.ring_halves = 0

    def add_audio_client(self, l, m, r, mode="USB"):
        c = AudioClient(self.ctx)
        c.set_audio_demodulation(mode)
        c.set_audio_range(l, m, r)
        self.audio_clients.append(c)
        return c

    def add_waterfall_client(self, level=None, l=None, r=None, detector=None):
        w = WaterfallClient(self.ctx)
        if level is not None:
            w.set_waterfall_range(level, l, r)
        if detector is not None:
            w.set_detector(detector)
        self.waterfall_clients.append(w)
        return w

    def upload_ring(self, raw):
        """raw: numpy array of whole half-frames in input_format; becomes the device ring."""
        raw = np.ascontiguousarray(raw, FORMAT_DTYPES[self.input_format])
        hb = self.ctx.half_frame_bytes()
        assert raw.nbytes % hb == 0, "ring must hold whole half-frames"
        if self.ring is not None:
            self.ctx.dev_free(self.ring)
        self.ring = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.ring, raw)
        self.ring_halves = raw.nbytes // hb

    def step(self, first_half, nframes, demod=True, waterfall=True):
        """frames [first_half, first_half+nframes) of the ring: FFT + pyramid, then the
        per-client fan-out.  Asynchronous; results are read through the client objects."""
        assert first_half + nframes + 1 <= self.ring_halves
        self.ctx.process_batch(self.ring, nframes, first_half * self.ctx.half_frame_bytes())
        if demod and self.audio_clients:
            self.ctx.demod_batch(self.frame_num)
        if waterfall and self.waterfall_clients:
            self.ctx.waterfall_batch(self.frame_num)
        self.frame_num += nframes

    def close(self):
        if self.ring is not None:
            self.ctx.dev_free(self.ring)
            self.ring = None
        self.ctx.close()

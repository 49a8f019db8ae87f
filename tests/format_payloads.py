"""One sample stream written in several input formats that the converter maps to the SAME f32 values.

All six formats convert to f32 exactly (src/samplereader.cpp:29-40: integers over 2^(bits-1), unsigned ones after an MSB
flip), so whatever follows the conversion - spectrum, int8 pyramid, audio, waterfall - must be bit-identical between the
members of a family.  Three families, all drawn from helpers.synth_stream:

  A  8-bit values  a = quantize_raw(x, "s8"), sigma 2^-5:   s16 = a * 256, u16 = a * 256 + 32768, s8 = a, u8 = a + 128,
                                                           f32 = f64 = a / 128                        (six members)
  B  16-bit values b = quantize_raw(x, "s16"):              s16 = b, u16 = b + 32768, f32 = f64 = b / 32768
                                                           (four members; the low bytes A leaves at zero)
  C  arbitrary floats:                                      f64 = x at full double precision, f32 = x.astype(float32)
                                                           (two members; the kernel's (float)double and numpy's astype
                                                           both round to nearest even)

The FIRST member of a family is the one the others are compared with (A and B: s16, the format every other test runs).
A and B carry the extreme codes (-128 / 127, -32768 / 32767) in both components of a sample pair (I and Q; for real input
the two real samples that share a slot of the packed transform): at the first and the last pair of the first half-frame,
at the first pair of the second half-frame (the middle of frame 0, where the window is 1 - at the stream's first sample it
is 0) and at two pairs inside half-frame 2 - where a sign extension or an MSB flip that is off shows.

tests/test_format_payloads.py checks the premise against the oracle's converter (bit-pinned to the reference's);
tests/test_gpu_format_invariance.py demands the identity of the GPU."""
import numpy as np

from helpers import FMT_DTYPE, quantize_raw, synth_stream

FAMILIES = {"A": ("s16", "u16", "s8", "u8", "f32", "f64"), "B": ("s16", "u16", "f32", "f64"), "C": ("f32", "f64")}
INTEGER_FORMATS = ("u8", "s8", "u16", "s16")
EXTREMES = {"A": (-128, 127), "B": (-32768, 32767)}
BITS = {"u8": 8, "s8": 8, "u16": 16, "s16": 16}
SIGMA_A = 2.0 ** -5   # as test_gpu_parity.test_process_batch_formats: 8-bit samples need a signal above their step


def half_frame_bytes(N, is_real, fmt):
    """bytes of one raw half-frame (N/2 samples; an IQ sample is two values)"""
    return (N // 2) * (1 if is_real else 2) * np.dtype(FMT_DTYPE[fmt]).itemsize


def plant_positions(N, is_real):
    """(index of the pair's first value in the interleaved stream, which extreme goes to each component): 0 = lowest code,
    1 = highest.  The stream is taken as pairs of values in both layouts."""
    per_half = (N // 2) * (1 if is_real else 2)   # values per half-frame
    inside = 2 * per_half + 2 * ((per_half // 2) // 3)   # a pair a third into half-frame 2 (frames 1 and 2)
    return [(0, (0, 1)), (per_half - 2, (1, 0)), (per_half, (1, 0)), (inside, (0, 0)), (inside + 2, (1, 1))]


def _plant(v, fam, N, is_real):
    lo_hi = EXTREMES[fam]
    for at, which in plant_positions(N, is_real):
        v[at], v[at + 1] = lo_hi[which[0]], lo_hi[which[1]]


def family(fam, N, is_real, nframes, seed):
    """[(format, raw samples)] of family `fam` over nframes + 1 half-frames, the reference member first"""
    ns = (nframes + 1) * (N // 2)
    if fam == "A":
        a = quantize_raw(synth_stream(ns, is_real, seed=seed, sigma=SIGMA_A, fft_size=N), "s8", is_real).astype(np.int32)
        _plant(a, fam, N, is_real)
        f64 = a / 128.0
        return [("s16", (a * 256).astype(np.int16)), ("u16", (a * 256 + 32768).astype(np.uint16)), ("s8", a.astype(np.int8)),
                ("u8", (a + 128).astype(np.uint8)), ("f32", f64.astype(np.float32)), ("f64", f64)]
    if fam == "B":
        b = quantize_raw(synth_stream(ns, is_real, seed=seed, fft_size=N), "s16", is_real).astype(np.int32)
        _plant(b, fam, N, is_real)
        f64 = b / 32768.0
        return [("s16", b.astype(np.int16)), ("u16", (b + 32768).astype(np.uint16)), ("f32", f64.astype(np.float32)), ("f64", f64)]
    if fam == "C":
        x = synth_stream(ns, is_real, seed=seed, fft_size=N)
        return [("f32", quantize_raw(x, "f32", is_real)), ("f64", quantize_raw(x, "f64", is_real))]
    raise ValueError(fam)

"""The cases of the audio-row kernels' shape tests (k_audio_nb, k_audio_nr, k_audio_filter): long frames, high and sparse slots.
tests/test_audio_rows_shapes_host.py anchors the host table programs - the GPU tests' expected values - at these frame lengths
and checks this table without a GPU; tests/test_gpu_audio_rows_long.py and tests/test_gpu_audio_rows_slots.py run it
(tests/test_gpu_audio_rows_reuse.py, the reused slot, shares the record file and the parameters).

Long frames: one 2^12-point IQ context per n, f32 input, tests/test_gpu_squelch.py's stream (unit noise, two keyed tones in the
window) and its 100-bin window.  What each n reaches, against the kernels' fixed units (256-sample blocks; the noise reduction's
group spans 640 samples, the blanker's 1072 with 824 samples of carried history; the filter's block is 1024):
  n =  512, h =  256  a frame is exactly one block: frame boundaries fall on block and hop boundaries
  n =  720, h =  360  longer than a block, shorter than both group spans; the compile-time IDFT plan
  n = 1036, h =  518  h % 4 != 0: the 8-byte path with long frames
  n = 2400, h = 1200  longer than the blanker's span, its history and the filter's block; a flagged frame blanks whole groups; a
                      one-frame batch holds two groups
Every n runs the batches BATCHES.  One NaN sample sits in the middle of the stream: the two frames that overlap its half-frame are
flagged, side by side.

stream_rules holds what a blanker run must be to be worth comparing against: the stream passes the blanker's delay by two blocks
and ends inside a block, one batch is a single frame, and the host program's trace has at least 8 centres, one gap across a block
boundary and one across a batch boundary.  At h = 256 no frame count ends inside a 256-sample block; there the rule kept is the
one that matters to the kernel: the stream ends with a block begun and not complete - its last 232 samples wait in the carried
history for the 24 the block still reads."""
import functools
import json
import os

import numpy as np

import anb_model as ANB
from conftest import ROOT

SHAPE, N, L0, RATE, LEVELS = "iq12", 1 << 12, 1000, 12000, 4
LONG_N = (512, 720, 1036, 2400)
BATCHES = (1, 3, 2, 4)
MAX_BATCH = 4
NAN_HALF = 6                      # the NaN sample's half-frame: frames 5 (the third batch's last) and 6 (the fourth's first) hold it
SEEDS = {512: 5, 720: 7, 1036: 5, 2400: 12}  # the first seed from 5 on with which every condition holds (test_audio_rows_shapes_host.py::test_the_case_table)
PARITY = (2.0, 15)                # the blanker's lowest threshold and widest gap: detections in nearly every block
NRP = (14.0, 1.5)
CPU_KINDS = ("USB", "LSB", "AM", "FM")   # the kinds whose rows the CPU oracle gives: the conditions on the input are chosen for these

# high and sparse slots
SLOTS, KEPT, LATE_SLOT, LATE_BATCH = 600, (0, 1, 63, 64, 255, 256, 598, 599), 597, 2
SLOT_N = (360, 12)


def key_of(nframes):
    """which half-frames carry the two tones: off for the first, then three on, one off"""
    return tuple(1 if i % 4 else 0 for i in range(nframes + 1))


def raw_of(n):
    from test_gpu_squelch import stream
    return stream(SHAPE, key=key_of(sum(BATCHES)), nan_half=NAN_HALF, seed=SEEDS[n])


def window():
    return (L0, L0 + 50.3, L0 + 100)


def stream_rules(h, batches, trace, width=PARITY[1]):
    """the conditions of the module docstring on a blanker run of `batches` frames of h samples with the host program's `trace`,
    as the list of the ones that do not hold"""
    T = h * sum(batches)
    broken = []
    if T < ANB.D + 2 * ANB.B:
        broken.append("shorter than the delay and two blocks")
    if T % ANB.B == 0 and h % ANB.B != 0:
        broken.append("ends on a block boundary")
    if ANB.blocks_done(T) * ANB.B + ANB.E == T:
        broken.append("ends where a block becomes complete")
    if 1 not in batches:
        broken.append("no batch of one frame")
    c = np.asarray(trace["centres"])
    pl = (width - 1) // 2
    lo, hi = c - pl, c + pl
    bounds = np.cumsum([b * h for b in batches])[:-1]
    if len(c) < 8:
        broken.append("fewer than 8 centres")
    if not np.any(lo // ANB.B != hi // ANB.B):
        broken.append("no gap crosses a block boundary")
    if not np.any((lo[:, None] < bounds[None, :]) & (hi[:, None] >= bounds[None, :])):
        broken.append("no gap crosses a batch boundary")
    return broken


def unusable_blocks(trace):
    return int(np.count_nonzero(np.asarray(trace["order"]) < 0))


def record(test, **figures):
    d = os.path.join(ROOT, "build", "records")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "audio_rows_shapes.jsonl"), "a") as f:
        f.write(json.dumps(dict(test=test, **figures)) + "\n")


@functools.lru_cache(maxsize=None)
def oracle_rows(n, kind, seed=None):
    """the CPU oracle's rows [F][h] and NaN flags [F] of a `kind` client on the long-frame stream of n"""
    from oracle import oracle as O
    from test_gpu_squelch import stream
    nf = sum(BATCHES)
    raw = stream(SHAPE, key=key_of(nf), nan_half=NAN_HALF, seed=SEEDS[n] if seed is None else seed)
    halves = raw.view(np.complex64).reshape(nf + 1, N // 2)
    fo = O.FFT(N, False, LEVELS, 0, n)
    o = O.AudioClient(False, n, RATE, N)
    o.set_audio_demodulation(kind)
    o.set_audio_range(*window())
    rows, flags = np.zeros((nf, n // 2), np.float32), np.zeros(nf, np.int32)
    for f in range(nf):
        fo.load(halves[f], halves[f + 1])
        fo.execute()
        audio, _, _, dropped = o.send_audio(fo.output().copy(), f, fft=fo, stats=False)
        flags[f] = int(dropped or np.isnan(audio).any())
        rows[f] = audio
    return rows, flags

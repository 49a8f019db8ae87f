"""The cases of the decoders' shape tests (k_audio_tone, k_audio_cw): every CW hop length, the shortest and the longest tone window,
frames longer than a block or a hop, frame lengths that are no multiple of 4, and frames so short that a batch completes nothing.
tests/test_decoder_shapes_host.py anchors the host table programs and the numpy models at these rates, frame lengths and batches and
checks this table without a GPU; tests/test_gpu_cw_shapes.py and tests/test_gpu_tone_shapes.py run it.

All of it in the smallest context the decoders' rigs make: a 2^12-point IQ transform, f32 input, a filler AM client in slot 0 and a
USB client in slot 1 whose window starts at client bin L0 (its lower edge is audio frequency zero) and is 100 bins wide - n / 4
bins at n = 2400, where PITCH and TONE_HZ lie 140 and 120 bins above the edge, and at n = 12 and n = 4.

CW cases (audio_rate, n); H = cw_hop(audio_rate), h = n / 2:
  ( 4000,  360)  H =  32, h =  180  5 or 6 hops per frame: more than CW_GROUP, a one-frame batch runs the group loop twice; the fill loop
                                    `n = lane; n < H; n += 64` leaves half of each wave idle
  (16000,  360)  H = 128, h =  180  the hop length nothing had run, at the first rate of its class
  (32000,  360)  H = 256, h =  180  a hop spans two frames; the carried partial hop passes 192 samples: all four waves store it
  (48000,  512)  H = 256, h =  256  frame = hop = CW_HMAX, the last legal rate
  (12000,  720)  H =  64, h =  360  a long frame
  (12000, 1036)  H =  64, h =  518  h % 4 = 2
  (12000, 2400)  H =  64, h = 1200  18 or 19 hops per frame: five groups in a one-frame batch; emit()'s frame range is empty for most D
  (12000,   12)  H =  64, h =    6  batches that complete no hop
Tone cases (audio_rate, n); nb = tone_nb(audio_rate), ring = nb + 3:
  ( 2000,  360)  nb =  4, h =  180  ring = 7: a group of four blocks wraps the ring inside the group
  ( 2000, 2400)  nb =  4, h = 1200  a frame holds more blocks than the window is long
  (48000,  512)  nb = 75, h =  256  ring = 78, the longest window sum
  ( 8000, 1036)  nb = 13, h =  518  h % 4 = 2
  (12000,  720)  nb = 19, h =  360  a long frame
  (12000, 2400)  nb = 19, h = 1200  4 or 5 blocks per frame: two groups in a one-frame batch
  (12000,   12)  nb = 19, h =    6  42 or 43 frames per block: batches that complete no block

Both tables also hold (12000, 4): h = 2, 128 frames per block - more than 64, so k_audio_tone's emit() takes a second step of its
stride of 64 frames per wave - and 32 per hop (k_audio_cw's stride would need H >= 128 at n = 4: not reached).  createplan.h plans it (tests/test_decoder_shapes_host.py::test_the_case_tables); its window is one bin wide.

Input, CW: tests/test_gpu_cw_decoder.py's builder with the rate as a parameter - unit noise and a carrier of amplitude 4, PITCH above
the window's lower edge, keyed in the raw samples with TEXT at WPM.  The lead is 1.1 x the floor ring's 128 hops, stretched so that the
stream is a whole number of frames and ends 4.15 dots behind the text (the last character's space, no word space); one NaN sample
sits in the middle of the word gap.  Tone: tests/test_gpu_tone_decoder.py's - unit noise and a carrier TONE_HZ above the lower edge
(tone 12), on for the first three fifths of the stream and off for the rest; the stream is five windows (5 nb 256 samples) long and
MIN_FRAMES frames at least; one NaN sample in the middle of the part with the tone.

Batches: every case runs whole - one batch - and split by split_of(): one-frame batches, 5 and 6 frames in turn (each ends inside a
hop or block wherever h is no multiple of it), a batch of a third of the stream, the same again, and the rest; at h = 6 and h = 2 also
batches of 20 and 41 frames (fewer than the 42.7 a block takes at h = 6) and one of more than 200.

cw_rules and tone_rules hold what a split run must be to be worth comparing: they are evaluated on the model's records, never on the
kernel's, and list the conditions that do not hold.  Nothing may be skipped: every case runs and every condition holds.  "Long frame"
in a condition means a frame that can complete more than a group: h > CW_GROUP H (every CW case but h = 180 at H >= 128, h = 256 and
h = 6), h > TONE_GROUP 256 (h = 1200)."""
import functools
import json
import math
import os

import numpy as np

import cw_model as CW
import tone_model as TM
from conftest import ROOT

SHAPE, N, L0, LEVELS = "iq12", 1 << 12, 1000, 4
CW_GROUP, TONE_GROUP, CW_HMAX = 4, 4, 256  # cwplan.h, toneplan.h (held to the headers by tests/test_decoder_shapes_host.py)
CW_CASES = ((4000, 360), (16000, 360), (32000, 360), (48000, 512), (12000, 720), (12000, 1036), (12000, 2400), (12000, 12), (12000, 4))
TONE_CASES = ((2000, 360), (2000, 2400), (48000, 512), (8000, 1036), (12000, 720), (12000, 2400), (12000, 12), (12000, 4))
CW_TRUTH = tuple(c for c in CW_CASES if c != (12000, 12))  # the text read is the text sent (at h = 6 the model alone is held)
TONE_GATED = ((2000, 360), (48000, 512), (8000, 1036), (12000, 720))          # a case per rate: gate = 1 and the post chain on
TWIN = (2000, 360)

TEXT, WPM, PITCH = "AN K", 25.0, 700.0
CW_CFG = dict(wpm=WPM)
END_DOTS = 4.15
TONE, TONE_HZ = 12, 100.0
TONE_CFG = dict(gate=0, hang_blocks=2)
MIN_FRAMES = 48
SEED = 11


def window(n):
    return (L0, L0 + 0.3, L0 + (100 if 200 <= n < 2400 else n // 4))


def split_of(nf, h):
    """the split run's batches"""
    third = max(7, nf // 3, 201 if h <= 6 else 0)
    want = [1, 1, 5, 6] + ([20, 41] if h <= 6 else []) + [third, 1, 1, 5, 6, 1]
    out, left = [], nf
    for b in want:
        if left <= 0:
            break
        out.append(min(b, left))
        left -= out[-1]
    if left > 0:
        out.append(left)
    assert sum(out) == nf
    return tuple(out)


def bounds(batches, h):
    """the stream position behind every batch but the last"""
    return np.cumsum([b * h for b in batches])[:-1]


def single_frame_units(batches, h, unit):
    """the units (hops, blocks) that each one-frame batch completes"""
    at = np.concatenate([[0], np.cumsum(batches)])[:-1]
    return [((f + 1) * h) // unit - (f * h) // unit for f, b in zip(at, batches) if b == 1]


def batch_units(batches, h, unit):
    at = np.concatenate([[0], np.cumsum(batches)])
    return [(int(at[i + 1]) * h) // unit - (int(at[i]) * h) // unit for i in range(len(batches))]


# ---- CW ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cw_timing(rate, n):
    """(frames, lead in seconds, the keying's runs as (on, start, end) in seconds, the middle of the word gap in seconds)"""
    h, H = n // 2, CW.hop_of(rate)
    dot = 1.2 / WPM
    keyed = sum(d for _, d in CW.keying(TEXT)) * dot
    nf = math.ceil((1.1 * CW.RING * H / rate + keyed + END_DOTS * dot) * rate / h)
    lead = nf * h / rate - keyed - END_DOTS * dot
    assert lead >= 1.1 * CW.RING * H / rate
    t, runs = lead, []
    for on, dots in CW.keying(TEXT):
        runs.append((on, t, t + dots * dot))
        t += dots * dot
    gap, = [r for r in runs if not r[0] and r[2] - r[1] > 6 * dot]
    return nf, lead, tuple(runs), (gap[1] + gap[2]) / 2


@functools.lru_cache(maxsize=1)  # (the whole and the split run of a case, one behind the other)
def cw_raw(rate, n, seed=SEED):
    """f32 half-frames, flat: unit noise plus the keyed carrier PITCH above client bin L0"""
    nf, _, runs, nan_t = cw_timing(rate, n)
    fs = rate * (N // 2) / (n // 2)  # a frame is N / 2 raw samples and n / 2 audio samples
    ns = (nf + 1) * (N // 2)
    rng = np.random.default_rng(seed)
    x = np.empty(ns, np.complex64)
    x.real, x.imag = rng.standard_normal(ns, dtype=np.float32), rng.standard_normal(ns, dtype=np.float32)
    c = L0 + PITCH * n / rate  # client bin c of an IQ spectrum is frequency index (c + N/2 + 1) mod N
    w = 2 * np.pi * ((c + N // 2 + 1) % N) / N
    for on, a, b in runs:
        if on:
            t = np.arange(int(round(a * fs)), int(round(b * fs)), dtype=np.float64)
            x[int(t[0]):int(t[0]) + len(t)] += (4.0 * np.exp(1j * w * t)).astype(np.complex64)
    raw = x.view(np.float32)
    raw[2 * int(round(nan_t * fs))] = np.nan
    return raw


def cw_synthetic(rate, n, seed=SEED):
    """(rows f32 [F * h], flags [F]) of the case without a GPU: cw_model.keyed_sine with the case's lead in noise, cut into the case's
    frames, the frame that holds the middle of the word gap flagged"""
    nf, lead, _, nan_t = cw_timing(rate, n)
    h = n // 2
    x = CW.keyed_sine(TEXT, WPM, rate, pitch=PITCH, lead=lead, tail=(END_DOTS + 1) * 1.2 / WPM)[:nf * h]
    assert len(x) == nf * h
    x = x + 0.01 * np.random.default_rng(seed).standard_normal(len(x))
    flags = np.zeros(nf, np.int32)
    flags[int(nan_t * rate) // h] = 1
    return x.astype(np.float32), flags


def cw_rules(rate, h, batches, rec, text, flags):
    """the module docstring's conditions on a CW run of `batches` frames of h samples with the model's records and text, as the list of
    the ones that do not hold"""
    H = CW.hop_of(rate)
    broken = []
    key = np.asarray(rec["key"])
    if not (key.any() and not key.all()):
        broken.append("key does not take both values")
    if len(text) < 3 or " " not in text:
        broken.append("the text is shorter than 3 characters or holds no space")
    if h % H and not np.any(bounds(batches, h) % H):
        broken.append("no batch boundary inside a hop")
    if 1 not in batches:
        broken.append("no batch of one frame")
    if not np.asarray(flags).any():
        broken.append("no flagged frame")
    if h > CW_GROUP * H and not any(u > CW_GROUP for u in single_frame_units(batches, h, H)):
        broken.append("no one-frame batch completes more than CW_GROUP hops")
    if h < H and 0 not in batch_units(batches, h, H):
        broken.append("no batch completes no hop")
    return broken


# ---- tone -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tone_timing(rate, n):
    """(frames, the carrier's last frame + 1, the NaN sample's half-frame)"""
    h = n // 2
    nf = max(math.ceil(5 * TM.nb_of(rate) * TM.B / h), MIN_FRAMES)
    off = math.ceil(3 * nf / 5)
    return nf, off, off // 2


@functools.lru_cache(maxsize=1)
def tone_raw(rate, n, seed=SEED):
    """f32 half-frames, flat: unit noise plus a carrier TONE_HZ above client bin L0, keyed off behind three fifths of the stream"""
    nf, off, nan_half = tone_timing(rate, n)
    ns = (nf + 1) * (N // 2)
    rng = np.random.default_rng(seed)
    x = np.empty(ns, np.complex64)
    x.real, x.imag = rng.standard_normal(ns, dtype=np.float32), rng.standard_normal(ns, dtype=np.float32)
    c = L0 + TONE_HZ * n / rate
    t = np.arange(off * (N // 2), dtype=np.float64)
    x[:len(t)] += (4.0 * np.exp(2j * np.pi * ((c + N // 2 + 1) % N) / N * t)).astype(np.complex64)
    raw = x.view(np.float32)
    raw[2 * (nan_half * (N // 2) + 17)] = np.nan
    return raw


def tone_synthetic(rate, n):
    """(rows f32 [F * h], flags [F]) of the case without a GPU: tone_model.tone_inputs' windows of tone 12 for three fifths of the
    case's frames, tone_model.noise_inputs' for the rest, one frame in the part with the tone flagged"""
    nf, off, nan_half = tone_timing(rate, n)
    h = n // 2
    win = TM.nb_of(rate) * TM.B
    won, woff = -(-off * h // win), -(-(nf - off) * h // win)
    x, k = TM.tone_inputs(rate, phases=won)
    x = np.concatenate([x[k == TONE].reshape(-1)[:off * h], TM.noise_inputs(rate, windows=woff).reshape(-1)[:(nf - off) * h]])
    assert len(x) == nf * h
    flags = np.zeros(nf, np.int32)
    flags[nan_half] = 1
    return x.astype(np.float32), flags


def tone_groups(batches, h, ring):
    """(ring row of the group's first block, blocks in the group) of every group of the run"""
    out, pos = [], 0
    for b in batches:
        b0, b1 = pos // TM.B, (pos + b * h) // TM.B
        out += [(bg % ring, min(TONE_GROUP, b1 - bg)) for bg in range(b0, b1, TONE_GROUP)]
        pos += b * h
    return out


def tone_rules(rate, h, batches, rec, flags):
    """the module docstring's conditions on a tone run of `batches` frames of h samples with the model's records, as the list of the
    ones that do not hold"""
    nb = TM.nb_of(rate)
    ring = nb - 1 + TONE_GROUP
    broken = []
    op = np.asarray(rec["open"])
    if not (op.any() and not op[int(np.argmax(op)):].all()):
        broken.append("the gate does not open and later close")
    if sum(batches) * h // TM.B < 2 * ring + TONE_GROUP:
        broken.append("fewer than 2 ring + TONE_GROUP blocks")
    if h % TM.B and not np.any(bounds(batches, h) % TM.B):
        broken.append("no batch boundary inside a block")
    if 1 not in batches:
        broken.append("no batch of one frame")
    if not np.asarray(flags).any():
        broken.append("no flagged frame")
    if h > TONE_GROUP * TM.B and not any(u > TONE_GROUP for u in single_frame_units(batches, h, TM.B)):
        broken.append("no one-frame batch completes more than TONE_GROUP blocks")
    if h < TM.B and 0 not in batch_units(batches, h, TM.B):
        broken.append("no batch completes no block")
    if rate == 2000 and not any(bm + 3 >= ring and bm + cnt > ring for bm, cnt in tone_groups(batches, h, ring)):
        broken.append("no group wraps the ring inside the group")
    return broken


def record(test, **figures):
    d = os.path.join(ROOT, "build", "records")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "decoder_shapes.jsonl"), "a") as f:
        f.write(json.dumps(dict(test=test, **figures)) + "\n")


# ---- the GPU rig ------------------------------------------------------------------------------------------------------------------
def open_ctx(rate, n, maxb, raw, max_clients=3, post=False):
    """tests/test_gpu_squelch.py's rig with the case's audio_rate, audio_fft_size and window"""
    from phantomsdr_amd import AudioClient
    from helpers import set_client_kind
    from test_gpu_squelch import Ctx

    class DCtx(Ctx):
        def __init__(self):
            super().__init__(SHAPE, n, max_clients, maxb=maxb, post=post, raw=raw, rate=rate)

        def add(self, kind="USB", cw=None, tone=None):
            g = AudioClient(self.ctx)
            set_client_kind(g, kind)
            g.set_audio_range(*window(n))
            if cw is not None:
                g.set_cw_decoder(True, **cw)
            if tone is not None:
                g.set_tone_decoder(True, **tone)
            return g

    return DCtx()


def cat(parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(len(parts[0])))

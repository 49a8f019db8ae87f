"""The scripted signal of tests/test_gpu_post_chain_edges.py and what it must drive the post chain into - shared with the CPU
check of the script itself (tests/test_post_chain_edges_script.py: the oracle's demodulator in the GPU's place).

A frame's spectrum is a fixed unit pattern times the frame's amplitude; amplitude 0 is an all-zero row, hence exactly zero
audio.  Lengths in look-ahead lengths LA = audio_rate / 5 samples and h = n / 2 samples per frame (la = ceil(LA / h) frames):

  a  la + 4 frames  1e-3    noise-like level: the AGC opens
  b  8              0       silence
  c  3              1e-4    the gains the silence left behind saturate the PCM in both signs, t still inside int32
  d  la + 8         0       the gain climbs with nothing in the window
  e  3              1       t beyond +-2^31
  f  la + 4         1e-39   denormal audio
  g  6              1e-3    recovery

Three clients: USB on one off-centre bin (a tone, symmetric in sign), AM on a carrier alone (a DC step where the carrier
switches, audio of one magnitude between), FM on the same carrier (constant audio, all-zero audio on silent frames).  Events,
all at batch boundaries inside (d): two frames in, the USB client becomes LSB (the mirrored window, the AGC reset); the AM
client is paused for four frames (two batches) placed so that its first resumed batch puts out the step at the start of (c)."""
import numpy as np

from oracle import oracle as O

N = 1 << 14
TINY = np.float32(1.1754944e-38)   # the smallest normal float32
USB_MID, TONE, CARRIER = 3001, 36, 6301   # odd bins: an IQ context leaves their sign alone in every frame
SEGMENTS = (("a", 4, 1e-3), ("b", 8, 0.0), ("c", 3, 1e-4), ("d", 8, 0.0), ("e", 3, 1.0), ("f", 4, 1e-39), ("g", 6, 1e-3))
WITH_LA = "adf"   # the segments that last la frames more
PAUSE_FRAMES = 4
# (d)'s eight frames of climb are 120 ms at 12 kHz and 5 ms at 192 kHz, where the gain gets to 1e-5 of what it gets to at
# 12 kHz: the burst is three decades louder there, so that it still leaves int32 (checked with the oracle's demodulator in
# the GPU's place, tests/test_post_chain_edges_script.py)
BURST = {192000: 1e3}


class Script:
    def __init__(self, rate, n):
        self.rate, self.n, self.h = rate, n, n // 2
        self.LA = rate // 5
        self.la = -(-self.LA // self.h)
        self.start, amp, f = {}, [], 0
        for name, extra, a in SEGMENTS:
            a = BURST.get(rate, a) if name == "e" else a
            self.start[name] = f
            k = extra + (self.la if name in WITH_LA else 0)
            amp += [a] * k
            f += k
        self.nframes = f
        self.amp = np.array(amp, np.float64)
        self.reset_at = self.start["d"] + 2
        # the first resumed batch starts LA / h frames of the client's own stream behind the start of (c), less one
        self.pause_from = self.start["c"] + self.LA // self.h - 1
        self.pause_to = self.pause_from + PAUSE_FRAMES
        assert self.reset_at <= self.pause_from and self.pause_to <= self.start["e"]
        w = n // 2 - 2
        self.windows = {"USB": (USB_MID, float(USB_MID), USB_MID + w), "LSB": (USB_MID - w, float(USB_MID), USB_MID),
                        "AM": (CARRIER - w, float(CARRIER), CARRIER + w), "FM": (CARRIER - w, float(CARRIER), CARRIER + w)}
        self.pattern = np.zeros(N, np.complex64)
        self.pattern[[USB_MID + TONE, USB_MID - TONE, CARRIER]] = 1.0

    def rows(self, f0, nb):
        """the spectra of frames [f0, f0 + nb)"""
        return (self.amp[f0:f0 + nb, None].astype(np.float32) * self.pattern[None, :]).astype(np.complex64)

    def segment(self, name):
        k = [s[0] for s in SEGMENTS].index(name)
        end = self.start[SEGMENTS[k + 1][0]] if k + 1 < len(SEGMENTS) else self.nframes
        return range(self.start[name], end)

    def batches(self, F, single=()):
        """batch starts: multiples of F, the events' frames, and every frame of `single`"""
        cuts = set(range(0, self.nframes, F)) | {self.reset_at, self.pause_from, self.pause_from + PAUSE_FRAMES // 2, self.pause_to}
        cuts |= set(single) | {self.nframes}
        cuts = sorted(cuts)
        return [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]

    def paused(self, f):
        return self.pause_from <= f < self.pause_to


class Twins:
    """The reference chains of one run, fed frame by frame with the float audio rows of the three clients (None for a frame
    the AM client sat out), and what they say about the regimes the signal reached.  Client 0: USB, LSB from reset_at on;
    1: AM; 2: FM.  The AM client's chain is the twin that skipped the paused frames; `fed_silence` got zero rows instead."""

    def __init__(self, script):
        self.s = script
        self.chains = [O.PostChain(script.rate) for _ in range(3)]
        self.fed_silence = O.PostChain(script.rate)
        self.pcm = [[] for _ in range(3)]      # per client: (frame, pcm row, the AGC's float output)
        self.silence_pcm = {}
        self.denormal_frames = 0

    def feed(self, f, audio):
        """-> the PCM rows the GPU must have for frame f (None for the paused client)"""
        s = self.s
        if f == s.reset_at:
            self.chains[0].reset_agc()
        want = []
        for ci, row in enumerate(audio):
            if ci == 1:
                self.silence_pcm[f] = self.fed_silence.process(row if row is not None else np.zeros(s.h, np.float32))
            if row is None:
                want.append(None)
                continue
            pcm, y = self.chains[ci].process(row, with_agc_out=True)
            self.pcm[ci].append((f, pcm, y))
            want.append(pcm)
        if f in s.segment("f"):
            x = np.abs(audio[0])
            self.denormal_frames += int(0 < x.max() < TINY)
        return want

    def regimes(self):
        """every figure a run must reach, by name -> (value, the least it may be)"""
        s = self.s
        pcm = np.concatenate([p for c in self.pcm for _, p, _ in c])
        t = np.concatenate([y for c in self.pcm for _, _, y in c]).astype(np.float64) * 16384.0
        inside = np.abs(t) < 2.0 ** 31
        after_reset = np.concatenate([p for f, p, _ in self.pcm[0] if f >= s.reset_at])[:s.LA]
        resumed = [f for f, _, _ in self.pcm[1] if f >= s.pause_to][:2]
        first = {f: p for f, p, _ in self.pcm[1]}
        differs = sum(int(np.count_nonzero(first[f] != self.silence_pcm[f])) for f in resumed)
        return {
            "PCM samples at +32767": (int(np.count_nonzero(pcm == 32767)), 10),
            "PCM samples at -32768": (int(np.count_nonzero(pcm == -32768)), 10),
            "AGC outputs with y * 16384 > 2^31": (int(np.count_nonzero(t > 2.0 ** 31)), 10),
            "AGC outputs with y * 16384 < -2^31": (int(np.count_nonzero(t < -2.0 ** 31)), 10),
            "samples at +32767 with t inside int32": (int(np.count_nonzero((pcm == 32767) & inside)), 10),
            "samples at -32768 with t inside int32": (int(np.count_nonzero((pcm == -32768) & inside)), 10),
            "frames of (f) whose USB audio is non-zero and all denormal": (self.denormal_frames, 1),
            # (LA - 1: the reference puts out 0 while its buffer holds fewer than LA samples, src/utils/audioprocessing.cpp:40-54;
            # the LA-th sample behind a reset is the first one times the first step of the gain - in "silence" the DC
            # blocker's f32 residue, which need not round to 0)
            "zero PCM samples among the first LA - 1 behind the reset": (int(np.count_nonzero(after_reset[:s.LA - 1] == 0)) if after_reset.size == s.LA else 0, s.LA - 1),
            "samples of the first two resumed frames that differ from the twin fed silence": (differs, 1),
            "non-zero PCM samples of the first two resumed frames": (sum(int(np.count_nonzero(first[f])) for f in resumed), 1),
        }

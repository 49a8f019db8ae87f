"""Waterfall detectors on the GPU (include/psdr.h: psdr_wf_detector): peak-hold and mean over the frames between two sent
rows.  Every expectation is tests/wf_detector_model.py applied to ctx.read_quantized(f) / ctx.quantized_level(...) of each
frame - the yardstick test_waterfall_batch uses - and every comparison is bit-exact: the maximum and the integer mean of
given int8 values have no tolerance to measure.

The stream carries a tone that is keyed on for fewer than skip_num frames OFF the sent frames, and the tests assert that
PEAK shows it where SAMPLE does not: a detector that silently sampled would fail them.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import quantize_raw, synth_stream

import wf_detector_model as M

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

DET = {M.SAMPLE: "sample", M.PEAK: "peak", M.MEAN: "mean"}
TONE_F = 0.05      # cycles per sample of the keyed tone


def levels_for(R, waterfall_size=1024):
    lv, cur = 0, R
    while cur >= waterfall_size:
        lv += 1
        cur //= 2
    return max(lv, 1)


def tone_bin(N, is_real):
    """index of the keyed tone at level 0, in the clients' coordinates (IQ: bin k is client bin (k - N/2 - 1) mod N)"""
    k = int(round(TONE_F * N))
    return k if is_real else (k - (N // 2 + 1)) % N


def keyed_stream(N, is_real, nframes, seed, keyed_halves):
    """synth_stream plus a strong tone during the half-frames `keyed_halves` (frame f = halves f, f + 1)"""
    h = N // 2
    x = synth_stream((nframes + 1) * h, bool(is_real), seed=seed, fft_size=N)
    t = np.arange(h, dtype=np.float64)
    for k in keyed_halves:
        ph = 2 * np.pi * TONE_F * (t + k * h)
        x[k * h:(k + 1) * h] += 0.05 * (np.cos(ph) if is_real else np.exp(1j * ph))
    return quantize_raw(x, "s16", bool(is_real))


class Rig:
    """one context + its stream; batch() processes frames and reports them to psdr_waterfall_batch, keeping what the
    model needs: every processed frame's pyramid and the list of calls"""

    def __init__(self, N, is_real, skip, F, nframes, keyed_halves=(), levels=None, nwf=16, seed=11):
        from phantomsdr_amd import Context
        self.N, self.is_real, self.skip = N, is_real, skip
        self.R = N // 2 if is_real else N
        self.levels = levels or levels_for(self.R)
        self.ctx = Context(N, is_real, self.levels, input_format="s16", max_batch=F, max_waterfall_clients=nwf, skip_num=skip)
        raw = keyed_stream(N, is_real, nframes, seed, keyed_halves)
        self.d = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.d, raw)
        self.q, self.calls, self.holding, self.clients = [], [], [], []

    def add(self, level=None, l=None, r=None, det=None):
        from phantomsdr_amd import WaterfallClient
        w = WaterfallClient(self.ctx)
        if level is not None:
            w.set_waterfall_range(level, l, r)
        w.det = M.SAMPLE
        if det is not None:
            self.set_det(w, det)
        self.clients.append(w)
        return w

    @staticmethod
    def set_det(w, det):
        w.set_detector(DET[det])
        w.det = det

    def batch(self, start, nf, first=None, keep=True):
        """frames start .. start + nf - 1 of the stream, reported as frames first .. (default: their own numbers)"""
        first = start if first is None else first
        self.ctx.process_batch(self.d, nf, offset_bytes=start * self.ctx.half_frame_bytes())
        self.ctx.waterfall_batch(first)
        self.q += [self.ctx.read_quantized(f) for f in range(nf)]
        self.calls.append((first, nf))
        self.holding.append(any(w.det != M.SAMPLE for w in self.clients if w.id >= 0))
        return [first + f for f in range(nf) if (first + f) % self.skip == 0]

    def rows_of(self, w):
        return np.stack([self.ctx.quantized_level(q, w.level)[w.l:w.r] for q in self.q])

    def expect(self, w, det=None):
        """the rows the LAST call gathers for client w with its window and detector at that call"""
        return M.expected_rows(self.rows_of(w), self.calls, self.skip, w.det if det is None else det, self.holding)[-1]

    def check(self, w, tag=""):
        got, label = w.read_waterfall()
        want = self.expect(w)
        assert got.shape == want.shape, (tag, got.shape, want.shape)
        assert label == (w.l << w.level, w.r << w.level)
        assert np.array_equal(got, want), f"{tag} client {w.id} level {w.level} [{w.l}, {w.r}) {DET[w.det]}: " \
                                          f"{int((got != want).sum())} of {got.size} bytes differ"
        return got

    def close(self):
        self.ctx.dev_free(self.d)
        self.ctx.close()


def _shape_clients(rig, dets=(M.PEAK, M.MEAN)):
    """every level (the tiled ones, the first level-major one and the top among them), aligned and unaligned starts, odd
    widths, width 1, the whole level"""
    rng = np.random.default_rng(5)
    out = []
    for lv in range(rig.levels):
        ln = rig.R >> lv
        spans = [(0, ln)] if ln <= 4096 else []
        if ln >= 8:
            l = int(rng.integers(0, ln - 4))
            spans += [(l | 1, min(ln, (l | 1) + int(rng.integers(1, min(ln - (l | 1), 1500) + 1)))), (l, l + 1),
                      ((l & ~3) + 2, min(ln, (l & ~3) + 2 + 7)), (l & ~3, min(ln, (l & ~3) + 64))]
        for i, (l, r) in enumerate(spans):
            out.append(rig.add(lv, l, r, dets[(lv + i) % len(dets)]))
    return out


@pytest.mark.parametrize("is_real", [0, 1])
def test_every_level_and_alignment_full_depth(is_real):
    """2^16-point IQ (tiled records for the low levels) and real input (level-major buffer) with the pyramid as deep as it
    goes (the top levels are 1, 2, 4 values long), skip_num 6, two batches: windows inside a batch and across the cut."""
    N, F, skip = 1 << 16, 8, 6
    R = N // 2 if is_real else N
    rig = Rig(N, is_real, skip, F, 2 * F, keyed_halves=(3, 4, 9, 10), levels=int(np.log2(R)) + 1, nwf=96)
    try:
        cl = _shape_clients(rig)
        assert len(cl) <= 96
        for b in range(2):
            sent = rig.batch(b * F, F)
            for w in cl:
                assert rig.check(w, f"batch {b}").shape[0] == len(sent)
    finally:
        rig.close()


@pytest.mark.parametrize("is_real", [0, 1])
@pytest.mark.parametrize("skip", [1, 2, 6, 11])
def test_detectors_differ_from_sample_only_as_the_contract_says(is_real, skip):
    """skip_num 1: every detector equals SAMPLE.  2, 6: windows inside and across batches of 4.  11: larger than the batch -
    a window spans three batches and the carry is accumulated twice before it is used.  A tone keyed on for two frames
    off the sent frames is on the PEAK row, far above the SAMPLE row, and lifts the MEAN row."""
    N, F, nb = 1 << 16, 4, 6
    R = N // 2 if is_real else N
    # frames 13, 14, 15 see the tone (halves 14, 15); sent frames of skip 2 / 6 / 11: 12, 16 / 12, 18 / 11, 22
    rig = Rig(N, is_real, skip, F, nb * F, keyed_halves=(14, 15))
    try:
        tb = tone_bin(N, is_real)
        cl = {}
        for det in (M.SAMPLE, M.PEAK, M.MEAN):
            cl[det] = [rig.add(0, tb - 301, tb + 200, det), rig.add(rig.levels - 1, 0, R >> (rig.levels - 1), det),
                       rig.add(2, (tb >> 2) - 77, (tb >> 2) + 78, det)]
        seen = {}
        for b in range(nb):
            sent = rig.batch(b * F, F)
            for det, ws in cl.items():
                for i, w in enumerate(ws):
                    got = rig.check(w, f"skip {skip} batch {b}")
                    for si, s in enumerate(sent):
                        seen[(det, i, s)] = got[si]
        for (det, i, s), row in seen.items():
            if skip == 1:
                assert np.array_equal(row, seen[(M.SAMPLE, i, s)])
        if skip > 1:
            s = {2: 14, 6: 18, 11: 22}[skip]      # the first sent frame whose window holds frame 14 (tone in both halves)
            if skip == 2:
                return                            # frame 14 is itself sent: SAMPLE sees the tone too
            j = 301                               # the tone's bin in the level-0 client's row
            sa, pk, mn = (int(seen[(d, 0, s)][j]) for d in (M.SAMPLE, M.PEAK, M.MEAN))
            assert pk >= sa + 20, f"PEAK {pk} does not show the keyed tone SAMPLE {sa} misses"
            assert mn > sa, (mn, sa)
            assert not np.array_equal(seen[(M.PEAK, 0, s)], seen[(M.SAMPLE, 0, s)])
            assert not np.array_equal(seen[(M.MEAN, 0, s)], seen[(M.SAMPLE, 0, s)])
            assert not np.array_equal(seen[(M.MEAN, 0, s)], seen[(M.PEAK, 0, s)])
    finally:
        rig.close()


@pytest.mark.parametrize("is_real", [0, 1])
def test_batch_split_invariance(is_real):
    """the same 12 frames as one batch, as batches of 4 and frame by frame (a call on every frame, like the server's
    loop): identical rows - the property the carry exists for"""
    N, T, skip = 1 << 16, 12, 6
    R = N // 2 if is_real else N
    tb = tone_bin(N, is_real)
    results = []
    for F in (T, 4, 1):
        rig = Rig(N, is_real, skip, F, T, keyed_halves=(8, 9))
        try:
            cl = [rig.add(0, tb - 100, tb + 155, M.PEAK), rig.add(1, 13, 13 + 2001, M.MEAN),
                  rig.add(rig.levels - 1, 0, R >> (rig.levels - 1), M.PEAK), rig.add(rig.levels - 1, 5, 900, M.MEAN),
                  rig.add(3, 40, 41, M.SAMPLE)]
            acc = [[] for _ in cl]
            for b in range(T // F):
                rig.batch(b * F, F)
                for i, w in enumerate(cl):
                    acc[i].append(rig.check(w, f"F {F} batch {b}"))
            results.append([np.concatenate(a) for a in acc])
            assert all(a.shape[0] == 2 for a in results[-1])          # frames 0 and 6
        finally:
            rig.close()
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert np.array_equal(a, b)


def test_frame_numbers_gaps_and_repeats():
    """first_frame_num that is no multiple of skip_num; a gap between two calls starts a new run (the first row covers the
    new run's frames only); so does a repeated call for the same batch"""
    N, F, skip = 1 << 16, 5, 4
    rig = Rig(N, 0, skip, F, 4 * F, keyed_halves=(2, 3))
    try:
        tb = tone_bin(N, 0)
        cl = [rig.add(0, tb - 50, tb + 51, M.PEAK), rig.add(0, tb - 50, tb + 51, M.MEAN), rig.add(rig.levels - 1, 1, 1000, M.PEAK)]
        rig.batch(0, F, first=3)              # frames 3..7: sent 4 (window: 3, 4)
        for w in cl:
            assert rig.check(w, "unaligned start").shape[0] == 1
        rig.batch(F, F, first=8)              # continues: 8..12, sent 8 (5..8 across the cut), 12
        for w in cl:
            assert rig.check(w, "continued").shape[0] == 2
        rig.batch(2 * F, F, first=21)         # gap: 21..25, sent 24 covers 21..24 only
        for w in cl:
            assert rig.check(w, "after a gap").shape[0] == 1
        rig.batch(3 * F, F, first=26)         # continues: 26..30, sent 28 = 25..28
        for w in cl:
            rig.check(w, "continued after the gap")
        rig.batch(3 * F, F, first=26)         # the same batch again: a new run, 28 = 26..28
        for w in cl:
            rig.check(w, "repeated")
    finally:
        rig.close()


def test_window_detector_and_client_changes_inside_a_window():
    """between two batches of a run: a window message, a detector change, a client that attaches, an id removed and added
    again - the next sent row is complete for the range and detector in force at that call"""
    N, F, skip = 1 << 16, 4, 6
    rig = Rig(N, 0, skip, F, 5 * F, keyed_halves=(8, 9))
    try:
        tb = tone_bin(N, 0)
        keeper = rig.add(rig.levels - 1, 0, 64, M.PEAK)      # keeps the carry alive throughout
        a = rig.add(0, 100, 1124, M.PEAK)
        b = rig.add(2, 7, 7 + 333, M.MEAN)
        c = rig.add(1, 900, 1500, M.SAMPLE)
        rig.batch(0, F)                        # 0..3: sent 0
        for w in (keeper, a, b, c):
            rig.check(w, "batch 0")
        rig.batch(F, F)                        # 4..7: sent 6
        for w in (keeper, a, b, c):
            rig.check(w, "batch 1")
        # frames 7 (carried), then the changes, then 8..11; sent 12 is in the batch after
        assert a.on_window_message(tb - 400, tb + 624)       # retune + zoom: another level, another range
        rig.set_det(b, M.PEAK)
        rig.set_det(c, M.MEAN)                               # was SAMPLE: its row must hold the carried frames too
        rig.batch(2 * F, F)
        late = rig.add(0, tb - 10, tb + 11, M.PEAK)          # attaches in the middle of window (6, 12]
        old_id = b.id
        b.on_close()
        rig.clients.remove(b)
        b2 = rig.add(2, 7, 7 + 333, M.MEAN)
        assert b2.id == old_id
        rig.batch(3 * F, F)                    # 12..15: sent 12 = frames 7..12 of three batches
        for w in (keeper, a, c, late, b2):
            assert rig.check(w, "after the changes").shape[0] == 1
        # the late client's row holds the keyed tone of frames 7..9, which only the carry has seen
        got = late.read_waterfall()[0][0]
        s12 = rig.ctx.quantized_level(rig.q[12], 0)[late.l:late.r]
        assert int(got[10]) >= int(s12[10]) + 20
        # every client back on SAMPLE: today's rows, and the carry stops; a detector afterwards starts from that call
        for w in (keeper, a, c, late, b2):
            rig.set_det(w, M.SAMPLE)
        rig.batch(4 * F, F, first=16)          # 16..19: sent 18 (SAMPLE)
        for w in (keeper, a, c, late, b2):
            got = rig.check(w, "all sample")
            assert np.array_equal(got[0], rig.ctx.quantized_level(rig.q[18], w.level)[w.l:w.r])
    finally:
        rig.close()


def test_detector_after_sample_only_calls_starts_a_new_run():
    """no history is kept while nobody asks for it: the first call with a detector starts the run"""
    N, F, skip = 1 << 16, 4, 6
    rig = Rig(N, 0, skip, F, 4 * F, keyed_halves=(8, 9))
    try:
        tb = tone_bin(N, 0)
        w = rig.add(0, tb - 64, tb + 64)
        rig.batch(0, F)
        rig.batch(F, F)                        # ... 7
        rig.check(w, "sample")
        rig.set_det(w, M.PEAK)
        rig.batch(2 * F, F)                    # 8..11: the run starts here
        rig.batch(3 * F, F)                    # sent 12 = 8..12, without frame 7
        assert rig.holding == [False, False, True, True]
        rig.check(w, "fresh run")
    finally:
        rig.close()


@pytest.mark.parametrize("is_real", [0, 1])
def test_sixty_four_mixed_clients(is_real):
    """64 random clients with mixed detectors in one call; the SAMPLE clients among them get today's rows"""
    N, F, skip = 1 << 16, 7, 3
    R = N // 2 if is_real else N
    rig = Rig(N, is_real, skip, F, 2 * F, keyed_halves=(4,), nwf=64)
    try:
        rng = np.random.default_rng(64 + is_real)
        for i in range(64):
            lv = int(rng.integers(0, rig.levels))
            ln = R >> lv
            l = int(rng.integers(0, ln - 1))
            r = int(rng.integers(l + 1, min(ln, l + 3000) + 1))
            rig.add(lv, l, r, int(rng.integers(0, 3)))
        assert {w.det for w in rig.clients} == {0, 1, 2}
        for b in range(2):
            sent = rig.batch(b * F, F, first=b * F + 1)
            for w in rig.clients:
                got = rig.check(w, f"batch {b}")
                if w.det == M.SAMPLE:
                    for si, s in enumerate(sent):
                        assert np.array_equal(got[si], rig.ctx.quantized_level(rig.q[s - 1], w.level)[w.l:w.r])
    finally:
        rig.close()


def test_fetch_path_agrees_with_read_waterfall():
    N, F, skip = 1 << 16, 6, 4
    rig = Rig(N, 0, skip, F, 2 * F, keyed_halves=(2,))
    try:
        cl = [rig.add(0, 1001, 2100, M.PEAK), rig.add(rig.levels - 1, 0, 1024, M.MEAN), rig.add(3, 0, 77, M.SAMPLE)]
        for b in range(2):
            rig.batch(b * F, F)
            rig.ctx.fetch_begin(rig.ctx.FETCH_WATERFALL)
            rig.ctx.fetch_end()
            for w in cl:
                rows, lv, l, r = rig.ctx.fetched_waterfall(w.id)
                assert (lv, l, r) == (w.level, w.l, w.r)
                assert np.array_equal(rows, rig.check(w, f"batch {b}"))
    finally:
        rig.close()


def test_arguments_are_checked():
    from phantomsdr_amd import Context, PsdrError, WaterfallClient
    ctx = Context(1 << 16, 0, 7, input_format="s16", max_batch=1, max_waterfall_clients=2, skip_num=(1 << 24) + 1)
    try:
        w = WaterfallClient(ctx)
        for bad in (-1, 3, 99):
            with pytest.raises(PsdrError) as e:
                w.set_detector(bad)
            assert e.value.code == -1
        with pytest.raises(PsdrError) as e:
            ctx.set_option(ctx.OPT_WATERFALL_DETECTOR, 3)
        assert e.value.code == -1
        assert ctx.lib.psdr_waterfall_set_detector(ctx.h, 1, 1) == -1      # no such client
        w.set_detector("peak")
        with pytest.raises(PsdrError) as e:                                # 32-bit sums: skip_num <= 2^24
            w.set_detector("mean")
        assert e.value.code == -6
        ctx.set_option(ctx.OPT_WATERFALL_DETECTOR, 1)                      # new clients start on PEAK
        w2 = WaterfallClient(ctx)
        assert w2.id == 1
    finally:
        ctx.close()


def test_option_sets_the_detector_of_new_clients():
    N, F, skip = 1 << 16, 4, 6
    rig = Rig(N, 0, skip, F, 2 * F, keyed_halves=(3, 4))
    try:
        w0 = rig.add(0, 500, 900)
        rig.ctx.set_option(rig.ctx.OPT_WATERFALL_DETECTOR, M.PEAK)
        w1 = rig.add(0, 500, 900)
        w1.det = M.PEAK                       # (what the option gave it)
        for b in range(2):
            rig.batch(b * F, F)
            rig.check(w0, "existing client stays on sample")
            rig.check(w1, "new client on peak")
    finally:
        rig.close()


def test_cfg2_fullsize_detectors_vs_model_and_oracle():
    """2^20-point IQ, skip_num 6, the bench's four cfg2 waterfall clients, PEAK and MEAN: bit-exact against the model on the
    GPU's own per-frame pyramid, and against the same model on the ORACLE's per-frame pyramid within the bound the
    full-size test uses for gathered rows (tests/test_gpu_fullsize.py:123: `d.max() <= 1 and (d != 0).mean() <= 5e-3` per
    frame).  Maximum and rounded mean are monotone, so frames that differ by at most 1 LSB give rows that differ by at
    most 1 LSB; a row that stands for n frames may differ wherever any of its frames does: its share cap is n times the
    per-frame cap (union bound)."""
    import bench as B
    from oracle import oracle as O
    from phantomsdr_amd import SpectrumEngine
    LSB_CAP, SHARE_CAP = 1, 5e-3              # tests/test_gpu_fullsize.py:123
    wl = B.WORKLOADS["cfg2"]
    N, fmt, splits = wl["fft_size"], wl["fmt"], (5, 4, 5)
    T = sum(splits)
    eng = SpectrumEngine(wl["sps"], N, False, input_format=fmt, max_batch=max(splits), max_clients=1,
                         max_waterfall_clients=2 * wl["waterfall"])
    try:
        p = eng.params
        levels, skip = p["downsample_levels"], p["skip_num"]
        assert skip == 6
        waterfalls = B.make_waterfalls(wl, p, seed=0x5D5D0002)
        raw = keyed_stream(N, False, T, 77, keyed_halves=(9, 10))
        eng.upload_ring(raw)
        conv = O.convert(raw, fmt).view(np.complex64).reshape(T + 1, N // 2)
        fo = O.FFT(N, False, levels, 0, p["audio_fft_size"])
        gwf = [(eng.add_waterfall_client(lv, l, r, detector=DET[det]), det, lv, l, r)
               for det in (M.PEAK, M.MEAN) for lv, l, r in waterfalls]
        q_gpu = [[] for _ in gwf]
        q_orc = [[] for _ in gwf]
        calls, frame = [], 0
        for nf in splits:
            first = eng.frame_num
            eng.step(frame, nf, demod=False)
            calls.append((first, nf))
            for f in range(nf):
                fo.load(conv[frame], conv[frame + 1])
                fo.execute()
                qg = eng.ctx.read_quantized(f)
                for i, (_, _, lv, l, r) in enumerate(gwf):
                    q_gpu[i].append(eng.ctx.quantized_level(qg, lv)[l:r].copy())
                    q_orc[i].append(fo.quantized_level(lv)[l:r].copy())
                frame += 1
            for i, (w, det, lv, l, r) in enumerate(gwf):
                got = w.read_waterfall()[0]
                want = M.expected_rows(np.stack(q_gpu[i]), calls, skip, det)[-1]
                assert np.array_equal(got, want), f"cfg2 waterfall {i} {DET[det]} batch at {first}"
                orc = M.expected_rows(np.stack(q_orc[i]), calls, skip, det)[-1]
                sent = [t for t in range(first, first + nf) if t % skip == 0]
                assert got.shape[0] == len(sent)
                for si, s in enumerate(sent):
                    n = min(skip, s + 1)                              # frames the row stands for (the run starts at 0)
                    d = np.abs(got[si].astype(np.int16) - orc[si].astype(np.int16))
                    print(f"cfg2 {DET[det]} client {i} frame {s}: n {n} max diff {d.max()} share {(d != 0).mean():.2e}")
                    assert d.max() <= LSB_CAP and (d != 0).mean() <= n * SHARE_CAP, f"waterfall {i} frame {s} vs oracle"
    finally:
        eng.close()

"""The band scan's device-only parts on masks that reach them (tests/band_scan_masks.py has the inputs, the sweep and the counters;
tests/test_band_scan_masks_host.py shows on the CPU oracle's values that the inputs are what they claim).  As in
tests/test_gpu_band_scan.py, whose Rig runs everything here, every expectation is tests/scan_model.py fed the GPU's OWN
read_quantized frames and every comparison is exact - trace, floors, total, every field of the list, the frame number.  What the
masks exercised is counted by cover() on the GPU's own values and held to the conditions of the host test: k_scan_emit's per-lane
atomics (words of several runs), its wave maximum (words of one run), a cap that falls between two starts of a word, runs across
the border of a k_scan_mark thread's stretch, tied peaks, the all-cold word inside a run at gap 64, zero runs, a list that is
cleared, and batches that nobody reads between psdr_process_batch and psdr_scan_batch.

The Python binding is ctypes over the C calls: process_batch and scan_batch enqueue and return, they wait for no stream."""
import ctypes as C

import numpy as np
import pytest

import band_scan_masks as B
import scan_model as M
from test_gpu_band_scan import Rig

pytestmark = pytest.mark.gpu


def pairs_of(runs):
    return {(int(r["first"]), int(r["end"])) for r in runs}


def check_filter_and_cap(rig, runs, tag):
    """psdr_read_signals' min_width filter and its cap argument on a list longer than the cap holds"""
    ctx = rig.ctx
    for k in (1, 2, 5):
        sig, total, fn = ctx.read_signals(min_width=k)
        want, passed, wtotal = M.listed(runs, k)
        assert total == wtotal > M.CAP and fn == rig.last, (tag, k, total, wtotal)
        assert len(sig) == passed and np.array_equal(sig.astype(M.SIGNAL), want), (tag, k, len(sig), passed)
    want, passed, wtotal = M.listed(runs, 2)
    cap = passed // 2
    assert cap > 0
    out = np.full(cap + 1, 0xFFFFFFFF, M.SIGNAL)  # one entry more than the call may write
    n, total, fn = C.c_int(0), C.c_int(0), C.c_uint64(0)
    rc = ctx.lib.psdr_read_signals(ctx.h, 2, out.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(total), C.byref(fn))
    assert rc == 0 and n.value == passed and total.value == wtotal and fn.value == rig.last, (tag, rc, n.value, passed, total.value)
    assert np.array_equal(out[:cap], want[:cap]) and out[cap]["first"] == 0xFFFFFFFF and out[cap]["floor"] == 0xFFFFFFFF, tag


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,is_real,level", B.SHAPES)
def test_noise_masks_every_threshold_and_gap(N, is_real, level):
    """white noise under every (threshold, gap) of the sweep, on one frame as it is (avg_shift 0: whole counts, full of ties) and
    on three frames at avg_shift 3; psdr_create takes IQ 2^17, the smallest shape with two mask words per k_scan_mark thread"""
    rig = Rig(N, is_real, 3, 3, raw=B.noise(N, is_real, 3))
    n = rig.R >> level
    per = B.words_per_thread(n)
    try:
        for nf, a in B.NOISE_TRACES:
            rig.process(0, nf)
            covers, over = {}, None
            for t, g in B.sweep():
                rig.set(level, avg_shift=a, threshold=t, gap=g)
                rig.scan(0)  # the same batch again under the new setting
                runs = rig.check(f"frames {nf} threshold {t} gap {g}")
                covers[(t, g)] = B.cover(rig.s, t, g, per, runs=runs)
                if covers[(t, g)]["cap_inside_word"] and over is None:
                    over = (t, g)
                    check_filter_and_cap(rig, runs, f"frames {nf} threshold {t} gap {g}")
            print(f"noise {N} real {is_real} level {level} frames {nf}: pairs reaching", {k: sum(1 for c in covers.values() if c[k]) for k in B.COUNTERS})
            assert not B.broken_rules(n, covers, a), B.broken_rules(n, covers, a)
            assert (over is not None) == (n // 2 > M.CAP)
    finally:
        rig.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,is_real,level", [(1 << 12, False, 0), (1 << 13, True, 2), (1 << 17, False, 0)])
def test_zero_runs(N, is_real, level):
    """threshold 255: no run, nothing listed, floors and trace as ever.  Between two such evaluations a sparse setting with long
    runs and then a dense one with short runs: an entry of the list that kept the long run's key would show a wrong peak"""
    rig = Rig(N, is_real, 1, 1, raw=B.noise(N, is_real, 3))
    try:
        rig.process(0, 1)
        seen = []
        for t, g in ((255, 2), (16, 64), (1, 0), (255, 2), (1, 0), (255, 64)):
            rig.set(level, avg_shift=0, threshold=t, gap=g)
            rig.scan(0)
            runs = rig.check(f"threshold {t} gap {g}")
            sig, total, fn = rig.ctx.read_signals()
            seen.append(total)
            if t == 255:
                assert len(runs) == 0 and total == 0 and len(sig) == 0 and fn == 0
                sig0, total0, _ = rig.ctx.read_signals(min_width=0)
                assert len(sig0) == 0 and total0 == 0
            else:
                assert total == len(runs) > 0 and len(sig) == min(total, M.CAP)
        assert seen[1] < seen[2] == seen[4]  # few long runs, then many short ones
    finally:
        rig.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,is_real", [(1 << 12, False), (1 << 13, True)])
def test_gap_edges_on_the_device(N, is_real):
    rig = Rig(N, is_real, 1, 1, raw=B.gap_edges(N, is_real, 1))
    lo, hi = 64 * B.ALIGNED_WORD - 3, 64 * (B.ALIGNED_WORD + 1)  # the first bins of the two blobs around the all-cold word
    try:
        rig.process(0, 1)
        for gap in B.EDGE_GAPS:
            rig.set(0, avg_shift=0, threshold=B.EDGE_THR, gap=gap)
            rig.scan(0)
            runs = rig.check(f"gap {gap}")
            have = pairs_of(rig.ctx.read_signals()[0])
            assert have == pairs_of(runs)
            for want in B.gap_edge_runs(gap):
                assert want in have, (gap, want, sorted(have))
            c = B.cover(rig.s, B.EDGE_THR, gap, 1, runs=runs)
            assert c["cold_eq_gap"] and (c["cold_eq_gap1"] or gap == 64), (gap, c)
            assert c["cold_words_inside"] == (1 if gap == 64 else 0), (gap, c)
            if gap == 64:  # one run over both blobs and the cold word between, its peak in the upper, stronger blob
                sig = rig.ctx.read_signals()[0]
                (r,) = sig[sig["first"] == lo]
                assert (int(r["end"]), int(r["peak_bin"])) == (hi + 3, hi + 1) and r["peak"] == rig.s[hi + 1] > rig.s[lo:lo + 3].max()
            else:
                assert (lo, lo + 3) in have and (hi, hi + 3) in have
    finally:
        rig.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", B.DECAY_SHIFTS)
def test_long_decay_at_both_shift_ends(a):
    """a comb that stops: the trace's step is the arithmetic shift of a negative difference for the rest of the stream"""
    N, nf = 1 << 12, B.DECAY_FRAMES
    rig = Rig(N, False, max(B.DECAY_BATCHES), nf, raw=B.decay(N, nf))
    try:
        rig.set(0, avg_shift=a, threshold=12, gap=2)
        at, top = 0, None
        for k in B.DECAY_BATCHES:
            rig.batch(at, k)
            at += k
            rig.check(f"shift {a} frames {at}")
            if at <= B.decay_on(nf):
                top = rig.s.copy()  # the comb is still whole
        comb = np.array(B.decay_comb(N))
        assert at == nf and top is not None
        print(f"decay shift {a}: bins fallen by more than 2^8 steps {B.fallen(top, rig.s)}")
        assert B.fallen(top, rig.s) >= len(comb) and np.all(top[comb] - rig.s[comb] > 1 << 8)
    finally:
        rig.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
UNREAD_BATCHES = (1, 2, 1, 2, 2, 1, 2)  # max_batch = 2: each of the two result sets is written three or four times


@pytest.mark.parametrize("beside", (False, True))
@pytest.mark.parametrize("N", (1 << 12, 1 << 17))
def test_unread_batches(N, beside):
    """Pass A reads every batch back (Rig.batch) and keeps the model.  Pass B makes the same calls under a new psdr_scan_set with
    nothing read and no synchronising call between the batches - process_batch and scan_batch only enqueue - so the scan's reads
    of the pyramid on the side stream are ordered against the next batches' writes by psdr_scan_batch's side_done and the
    result-set events alone; it is checked once, behind the last batch, against pass A's model.  beside: a USB client and a
    waterfall client, waterfall_batch and demod_batch enqueued for every batch of pass B as well"""
    nf = sum(UNREAD_BATCHES)
    kw = dict(audio_fft_size=360, max_clients=2, max_waterfall_clients=2) if beside else {}
    rig = Rig(N, False, 2, nf, raw=B.noise(N, False, nf), **kw)
    try:
        ctx = rig.ctx
        if beside:
            from phantomsdr_amd import AudioClient, WaterfallClient
            au = AudioClient(ctx)
            au.set_audio_demodulation("USB")
            au.set_audio_range(1000, 1000.0, 1060)
            wf = WaterfallClient(ctx)
            wf.set_waterfall_range(1, 100, 1500)
        cfg = dict(avg_shift=3, threshold=8, gap=2)
        rig.set(0, **cfg)
        at = 0
        for k in UNREAD_BATCHES:
            rig.batch(at, k)
            at += k
        runs_a = rig.check("pass A")
        s_a, sig_a = rig.s.copy(), rig.ctx.read_signals()
        assert len(runs_a) > 100 and B.cover(s_a, cfg["threshold"], cfg["gap"], B.words_per_thread(N), runs=runs_a)["multi_run_words"]
        rig.set(0, **cfg)
        at = 0
        for k in UNREAD_BATCHES:
            rig.process(at, k)
            rig.scan(at, read=False)
            if beside:
                ctx.waterfall_batch(at)
                ctx.demod_batch(at)
            at += k
        rig.s = s_a
        runs_b = rig.check("pass B, unread")
        sig_b = rig.ctx.read_signals()
        assert np.array_equal(runs_b, runs_a) and np.array_equal(sig_b[0], sig_a[0]) and sig_b[1:] == sig_a[1:] and sig_b[2] == nf - 1
    finally:
        rig.close()

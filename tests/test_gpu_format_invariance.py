"""Every sample format through every first-pass kernel, bit for bit.

pass1_body (csrc/fft_pass.h) is the only kernel that reads raw samples: 13 (L, T) families x three slot widths (SB = 2, 4,
8 bytes per complex sample) x two copies of the fill body (with and without the unsigned formats' MSB flip), and a second
load path for f64 in the SB = 8 instantiations.  The load addressing depends on format and shape together.  The oracle
here needs no tolerance: all six formats convert to f32 exactly and the integer formats' 2^-(bits-1) rides in the window
weights as a power of two, so members of one payload family (tests/format_payloads.py; the premise is checked on the CPU
by tests/test_format_payloads.py) must give the same spectrum, pyramid, audio and waterfall bits.

  a. every accepted shape x every member of families A (8-bit values, six formats), B (16-bit values, four) and C
     (arbitrary floats, f32 / f64): 3 frames in batches of 2 + 1 - frame index 1 and the second batch's byte offset in each
     format's units.  One truth anchor per family and shape (the first member against the float64 transform), so that a
     family agreeing with itself while wrong is still caught.  Figures: build/records/format_invariance.jsonl.
  b. float input launches extra kernels behind every IDFT family (demod.hip: can_be_nonfinite - the replay launch of
     k_demod_chain_fixed, k_demod_ola_seq).  On finite data they must change nothing: audio, power, NaN flags, waterfall
     rows and the post chain's PCM (int32 and int16 rows) of s16 against f32 and of f32 against f64.
  c. the ingest ring in the formats whose half-frames are the smallest and the largest (u8, u16, f64)."""
import json
import os
import time

import numpy as np
import pytest

from format_payloads import FAMILIES, family
from oracle import oracle as O
from test_gpu_abi import ring_ingest_against_flat_upload
from test_gpu_parity import levels_for, tone_bin
from test_gpu_plan_sweep import GPU_L2, GPU_OVER_ORACLE, SHAPES, SPEC_L2, SPEC_TOL, _process, _tag
from test_gpu_truth_f64 import _ref_window, _truth_spectrum

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(row):
    d = os.path.join(ROOT, "build", "records")
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "format_invariance.jsonl"), "a") as f:
            f.write(json.dumps(row) + "\n")
    except OSError:
        pass


def _diff(a, b):
    """(number of differing words, index of the first) of two equally shaped arrays compared as stored"""
    bad = np.flatnonzero(a != b)
    return (int(bad.size), int(bad[0])) if bad.size else (0, -1)


# ---- a. every format through every shape ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,is_real", SHAPES, ids=[_tag(*s) for s in SHAPES])
def test_every_format_through_every_shape(N, is_real):
    """Within a family every member's spectrum (as uint32 words) and int8 pyramid equal the first member's, frame by frame.
    The first member's last frame (in the second batch) against DFT_N(f32(x) * f32(w)) / N in complex128: family B (s16,
    the stream the plan sweep measured) under the plan sweep's bounds unchanged - SPEC_TOL, SPEC_L2, GPU_L2 = 5e-7,
    GPU_OVER_ORACLE = 3; families A and C under SURVEY B.6 (1e-4 of the peak, 1e-5 relative L2) and GPU_OVER_ORACLE against
    the oracle's own distance from the truth.  (Nobody had measured the GPU's absolute L2 on 8-bit or full-mantissa
    payloads: recorded, not bounded tighter.)
    A spectrum bin b of an IQ frame is client-order bin c = (b - N/2 - 1) mod N = c1 + M1 * c2 (real: b itself on the packed
    N/2-point transform): row c1 of pass 1's tile, column n2 summed over - a wrong sample shows in every bin, a wrong row or
    frame stride in the bins of the rows it feeds."""
    from phantomsdr_amd import Context
    R = N // 2 if is_real else N
    F, splits = 3, (2, 1)
    levels = levels_for(R)
    nb = N // 2 if is_real else N
    shape = _tag(N, is_real)
    w, wsrc = _ref_window(N)
    fo = O.FFT(N, is_real, levels, 0, 0)
    failures, t0 = [], time.time()
    for fam in sorted(FAMILIES):
        members = family(fam, N, is_real, F, seed=6000 + N.bit_length() + (100 if is_real else 0))
        first = None
        for fmt, raw in members:
            ctx = Context(N, is_real, levels, input_format=fmt, max_batch=max(splits))
            try:
                assert ctx.half_frame_bytes() * (F + 1) == raw.nbytes, (shape, fmt)
                spec, q = _process(ctx, raw, splits)
            finally:
                ctx.close()
            if first is None:
                first = (fmt, spec, q)
                conv = O.convert(raw, fmt)
                halves = (conv if is_real else conv.view(np.complex64)).reshape(F + 1, N // 2)
                continue
            for f in range(F):
                ns, bs = _diff(spec[f].view(np.uint32), first[1][f].view(np.uint32))
                nq, bq = _diff(q[f], first[2][f])
                if ns or nq:
                    failures.append(f"{shape} family {fam}: {fmt} against {first[0]}, frame {f}: {ns} of {2 * spec[f].size} spectrum "
                                    f"words differ, first in bin {bs // 2}; {nq} of {q[f].size} pyramid bytes, first at {bq}")
        # the anchor: the family's first member, last frame (the second batch), against the float64 truth
        f = F - 1
        Xt = _truth_spectrum(halves[f], halves[f + 1], w, N, is_real)
        fo.load(halves[f], halves[f + 1])
        fo.execute()
        Xo = fo.output()[: len(Xt)].copy()
        Xg = first[1][f]
        peak, nrm = np.abs(Xt[:nb]).max(), np.linalg.norm(Xt[:nb])
        eg, eo = np.abs(Xg[:nb] - Xt[:nb]).max() / peak, np.abs(Xo[:nb] - Xt[:nb]).max() / peak
        lg, lo = np.linalg.norm(Xg[:nb] - Xt[:nb]) / nrm, np.linalg.norm(Xo[:nb] - Xt[:nb]) / nrm
        row = dict(test="anchor", shape=shape, fft_size=N, is_real=is_real, family=fam, member=first[0], frame=f, window=wsrc,
                   spec_max_gpu=float(eg), spec_max_orc=float(eo), spec_l2_gpu=float(lg), spec_l2_orc=float(lo),
                   l2_ratio=float(lg / lo), below_gpu_l2=bool(lg <= GPU_L2))
        _record(row)
        print(json.dumps(row))
        tag = f"{shape} family {fam} ({first[0]}) frame {f}"
        if not (eo <= SPEC_TOL and lo <= SPEC_L2):
            failures.append(f"{tag}: oracle spectrum against float64: max {eo:.2e} of the peak, L2 {lo:.2e}")
        if not (eg <= SPEC_TOL and lg <= SPEC_L2):
            failures.append(f"{tag}: GPU spectrum against float64: max {eg:.2e} of the peak, L2 {lg:.2e}")
        if fam == "B" and not lg <= GPU_L2:
            failures.append(f"{tag}: GPU relative L2 {lg:.2e} against float64 (oracle {lo:.2e})")
        if not lg <= GPU_OVER_ORACLE * lo:
            failures.append(f"{tag}: GPU relative L2 {lg:.2e} is {lg / lo:.2f} x the oracle's {lo:.2e}")
        if is_real:  # the un-normalised bin N/2 (src/fft_impl.cpp:156-160 never visits it)
            if not abs(Xg[N // 2] - Xt[N // 2]) <= 1e-4 * np.abs(Xt[N // 2:]).max() + 1e-4 * peak * N:
                failures.append(f"{tag}: bin N/2")
        del members, first, halves
    print(json.dumps(dict(test="wall", shape=shape, seconds=round(time.time() - t0, 2))))
    assert not failures, "\n".join(failures)


# ---- b. float input changes no audio bit -------------------------------------------------------------------------------
# n, PSDR_DEMOD_CHAIN (None: the kernel does not look at it) - one n per IDFT family (demod.hip)
IDFT_FAMILIES = [(248, None),    # k_demod_idft_wave
                 (360, True),    # k_demod_chain_fixed (+ its replay launch for float input)
                 (360, False),   # k_demod_idft_fixed + k_demod_ola (+ k_demod_ola_seq)
                 (720, True),    # k_demod_chain_fixed
                 (1008, None)]   # k_demod_idft (generic)
DEMOD_CASES = [(n, r, ch, post) for (n, ch) in IDFT_FAMILIES for r in (0, 1) for post in (0, 1)]


def _demod_id(c):
    n, r, ch, post = c
    return f"{n}-{'real17' if r else 'iq16'}-{'any' if ch is None else ('chain' if ch else 'two')}-{'post' if post else 'nopost'}"


def _run_clients(N, is_real, n, fmt, raw, clients, wf_range, post, F, nbatches):
    """everything the clients of one context read over nbatches batches of F frames, as integer arrays"""
    from phantomsdr_amd import AudioClient, Context, WaterfallClient
    R = N // 2 if is_real else N
    # 6000: a look-ahead of 1200 samples, so that the AGC opens within 10 frames of 124 samples
    ctx = Context(N, is_real, levels_for(R), additional_size=n, audio_fft_size=n, audio_rate=6000 if post else 12000,
                  input_format=fmt, max_batch=F, max_clients=len(clients), max_waterfall_clients=1)
    out = []
    try:
        if post:
            ctx.set_option(ctx.OPT_POST_CHAIN_PCM16, 1)
            ctx.set_post_chain(True)
        d = ctx.dev_alloc(raw.nbytes)
        ctx.h2d(d, raw)
        gcl = []
        for mode, l, mid, r in clients:
            g = AudioClient(ctx)
            g.set_audio_demodulation(mode)
            g.set_audio_range(l, mid, r)
            gcl.append(g)
        wfc = WaterfallClient(ctx)
        wfc.set_waterfall_range(*wf_range)
        hb = ctx.half_frame_bytes()
        assert hb * (nbatches * F + 1) == raw.nbytes
        for b in range(nbatches):
            if post and b == nbatches - 1:
                ctx.set_option(ctx.OPT_POST_CHAIN_PCM16, 0)   # int16 rows first, int32 rows in the last batch
            ctx.process_batch(d, F, offset_bytes=b * F * hb)
            ctx.demod_batch(b * F)
            ctx.waterfall_batch(b * F)
            if post:
                ctx.fetch_begin(ctx.FETCH_PCM)
                ctx.fetch_end()
            res = {}
            for ci, g in enumerate(gcl):
                a, p, nan = g.read_audio(F)
                res[f"client {ci} audio"] = a.view(np.uint32).copy()
                res[f"client {ci} power"] = p.view(np.uint32).copy()
                res[f"client {ci} nan"] = nan.copy()
                if post:
                    res[f"client {ci} pcm"] = g.read_pcm(F).copy()
                    if b < nbatches - 1:
                        res[f"client {ci} pcm16"] = np.stack([ctx.fetched_pcm16(g.id, f) for f in range(F)])
                    else:
                        res[f"client {ci} pcm32"] = np.stack([ctx.fetched_audio(g.id, f, pcm=True)[3] for f in range(F)])
            rows, labels = wfc.read_waterfall()
            res["waterfall"] = rows.copy()
            res["waterfall labels"] = np.asarray(labels)
            out.append(res)
        ctx.dev_free(d)
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("n,is_real,chain,post", DEMOD_CASES, ids=[_demod_id(c) for c in DEMOD_CASES])
def test_float_input_changes_no_audio_bit(n, is_real, chain, post, monkeypatch):
    """Family B's s16 against its f32 member (the same values; f32 alone sets can_be_nonfinite) and family C's f32 against its
    f64 member, through two otherwise identical contexts: USB, LSB, AM and FM clients with even, odd and fractional mids, at the
    spectrum edges, and one waterfall client; 2 batches of 5 frames.  Audio rows and power as uint32 words, NaN flags (all
    0), waterfall rows and - with the post chain on - the int32 rows, the int16 rows of PSDR_OPT_POST_CHAIN_PCM16 and
    psdr_read_pcm's rows are equal."""
    if chain is not None:
        monkeypatch.setenv("PSDR_DEMOD_CHAIN", "1" if chain else "0")
    N = 1 << 17 if is_real else 1 << 16
    R = N // 2 if is_real else N
    F, nbatches = 5, 2
    am = int(tone_bin(N, is_real, 0.11))
    fm = int(tone_bin(N, is_real, 0.31 if is_real else -0.21))
    w3, w5 = n // 4, n // 2 - 3
    clients = [("USB", am, float(am), am + w3), ("USB", am + 1, am + 1.5, am + 1 + w3), ("LSB", am - w3, float(am), am),
               ("LSB", am - w3 + 1, am + 1.25, am + 1), ("AM", am - w5, float(am), am + w5),
               ("AM", am - w5 + 1, am + 1.0, am + 1 + w5), ("FM", fm - w5, float(fm), fm + w5),
               ("FM", fm - w5 + 1, fm + 1.75, fm + w5), ("USB", 0, 0.0, w3), ("LSB", R - 1 - w3, float(R - 1), R - 1),
               ("USB", 200, 200.0, 200 + n)]
    wf_range = (1, R // 6, R // 6 + 1000)
    pairs = []
    for fam, fa, fb in (("B", "s16", "f32"), ("C", "f32", "f64")):
        m = dict(family(fam, N, is_real, nbatches * F, seed=300 + n + is_real))
        pairs.append((fam, fa, m[fa], fb, m[fb]))
    for fam, fa, ra, fb, rb in pairs:
        A = _run_clients(N, is_real, n, fa, ra, clients, wf_range, post, F, nbatches)
        B = _run_clients(N, is_real, n, fb, rb, clients, wf_range, post, F, nbatches)
        opened = 0
        for b in range(nbatches):
            assert A[b].keys() == B[b].keys()
            for key in A[b]:
                u, v = A[b][key], B[b][key]
                assert u.shape == v.shape, (fam, b, key)
                nd, at = _diff(u.ravel(), v.ravel())
                assert nd == 0, f"n={n} family {fam}: {fb} against {fa}, batch {b}, {key}: {nd} of {u.size} words differ, first at {at}"
                if key.endswith("nan"):
                    assert not u.any(), (fam, b, key)
                if key.endswith("audio"):
                    assert np.isfinite(u.view(np.float32)).all(), (fam, b, key)
                if key.endswith("pcm"):
                    opened += int(np.count_nonzero(u))
            assert A[b]["waterfall"].shape == (F, 1000) and A[b]["waterfall"].std() > 0
            if post:  # the three views of the chain's output agree with each other as well
                for ci in range(len(clients)):
                    wide = A[b][f"client {ci} pcm"]
                    other = A[b].get(f"client {ci} pcm16", A[b].get(f"client {ci} pcm32"))
                    assert np.array_equal(wide, other.astype(np.int32)), (fam, b, ci)
        assert any(A[b]["client 4 audio"].any() for b in range(nbatches))
        print(json.dumps(dict(test="audio", n=n, is_real=is_real, chain=chain, post=post, family=fam, pcm_nonzero=opened)))
        if post:
            assert opened > 0, "the AGC never opened: the PCM rows compared are all zero"


# ---- c. the ingest ring in every slot width ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,is_real", [(1 << 12, 0), (1 << 21, 1)], ids=["iq12", "real21"])
@pytest.mark.parametrize("fmt", ["u8", "u16", "f64"])
def test_ring_ingest_in_every_format(fmt, N, is_real):
    """test_gpu_abi.test_ring_ingest_matches_flat_upload (a ring of 8 halves wrapped several times against a flat upload of the
    same bytes: spectra, pyramids and audio bit for bit) in the formats it does not run: half-frames of 4 KiB (u8, IQ 2^12)
    to 8 MiB (f64, fused real 2^21)."""
    ring_ingest_against_flat_upload(N, is_real, fmt)

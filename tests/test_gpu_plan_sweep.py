"""Every shape psdr_create accepts and every pyramid depth, against float64 truth and the reference quantiser.

psdr_create takes any power-of-two frame whose complex transform length is 2^12..2^22 (IQ 2^12..2^22, real 2^13..2^23)
with downsample_levels 1..log2(R)+1.  Each shape picks its own second pass and epilogue (context.hip: the (M2, T2) split,
the fused IQ / fused real / three-pass real families, tile-record levels LT, column tail) and each depth its own set of
`lv < nlevels` guards and tail launches (forward.hip: enqueue_tails).  Here:

  1. every accepted shape, 4 frames in batches of 3 + 1: the spectrum against the complex128 transform of the
     f32-windowed input (test_gpu_truth_f64._truth_spectrum, the reference's Hann table), the oracle's FFT as well;
     four audio and two waterfall clients on the shapes nothing else runs (2^22 IQ, 2^18 / 2^20 / 2^23 real);
  2. every pyramid depth that moves a boundary on one shape per epilogue family: the int8 pyramid bit-exact against
     the reference quantiser on the GPU's own spectrum, spectrum and every level's bytes identical across depths, one
     waterfall client per level at the deepest depth, the default client and the level choice of on_window_message;
  3. the reference's five shipped configuration files end to end (n = 10068, 2520, 10068, 548, 2048);
  4. (tests/test_gpu_parity.py::test_error_paths) the boundaries of psdr_create.

The measured truth figures are appended to build/records/plan_sweep.jsonl (git-ignored)."""
import json
import os

import numpy as np
import pytest

from helpers import quantize_raw, rel_err, rel_l2, synth_stream
from oracle import oracle as O
from test_gpu_fullsize import _check_audio, _check_pyramid
from test_gpu_parity import levels_for
from test_gpu_truth_f64 import _ref_window, _truth_spectrum

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPEC_TOL, SPEC_L2 = 1e-4, 1e-5   # SURVEY B.6 against the truth (test_gpu_truth_f64)
GPU_L2 = 5e-7                    # measured 1.9-3.5e-7 over all 22 shapes
GPU_OVER_ORACLE = 3.0            # measured 1.26-2.34 x

SHAPES = [(1 << k, False) for k in range(12, 23)] + [(1 << k, True) for k in range(13, 24)]


def _tag(N, is_real):
    return f"{'real' if is_real else 'iq'}{N.bit_length() - 1}"


def _record(row):
    d = os.path.join(ROOT, "build", "records")
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "plan_sweep.jsonl"), "a") as f:
            f.write(json.dumps(row) + "\n")
    except OSError:
        pass


def _stream(N, is_real, nframes, seed, fmt="s16"):
    """(raw, halves [nframes + 1][N/2] as the converter sees them)"""
    x = synth_stream((nframes + 1) * (N // 2), is_real, seed=seed, fft_size=N)
    raw = quantize_raw(x, fmt, is_real)
    conv = O.convert(raw, fmt)
    return raw, (conv if is_real else conv.view(np.complex64)).reshape(nframes + 1, N // 2)


def _process(ctx, raw, splits):
    """raw half-frames through Context.process_batch in batches of `splits` frames: (spectra, pyramids) per frame"""
    d = ctx.dev_alloc(raw.nbytes)
    spec, q = [], []
    try:
        ctx.h2d(d, raw)
        hb, first = ctx.half_frame_bytes(), 0
        for nf in splits:
            ctx.process_batch(d, nf, first * hb)
            for f in range(nf):
                spec.append(ctx.read_spectrum(f))
                q.append(ctx.read_quantized(f))
            first += nf
    finally:
        ctx.synchronize()
        ctx.dev_free(d)
    return spec, q


# ---- 1. every accepted shape against float64 truth ------------------------------------------------------------------
@pytest.mark.parametrize("N,is_real", SHAPES, ids=[_tag(*s) for s in SHAPES])
def test_every_shape_against_float64_truth(N, is_real):
    """GPU and oracle spectra of 4 frames (batches of 3 + 1: the half-frame carried across batches) against
    DFT_N(f32(x) * f32(w)) / N in complex128.  Bounds: SURVEY B.6 (1e-4 of the peak, 1e-5 relative L2) for both, and
    for the GPU relative L2 <= 5e-7 and <= 3 x the oracle's, frame by frame."""
    from phantomsdr_amd import Context
    R = N // 2 if is_real else N
    F = 4
    raw, halves = _stream(N, is_real, F, seed=4000 + N.bit_length() + (100 if is_real else 0))
    levels = levels_for(R)
    ctx = Context(N, is_real, levels, input_format="s16", max_batch=3)
    try:
        spec, _ = _process(ctx, raw, (3, 1))
    finally:
        ctx.close()
    w, wsrc = _ref_window(N)
    fo = O.FFT(N, is_real, levels, 0, 0)
    nb = N // 2 if is_real else N
    worst = dict(spec_max_gpu=0.0, spec_max_orc=0.0, spec_l2_gpu=0.0, spec_l2_orc=0.0, l2_ratio=0.0)
    for f in range(F):
        tag = f"{_tag(N, is_real)} frame {f}"
        Xt = _truth_spectrum(halves[f], halves[f + 1], w, N, is_real)
        fo.load(halves[f], halves[f + 1])
        fo.execute()
        Xo = fo.output()[: len(Xt)].copy()
        Xg = spec[f]
        peak, nrm = np.abs(Xt[:nb]).max(), np.linalg.norm(Xt[:nb])
        eg, eo = np.abs(Xg[:nb] - Xt[:nb]).max() / peak, np.abs(Xo[:nb] - Xt[:nb]).max() / peak
        lg, lo = np.linalg.norm(Xg[:nb] - Xt[:nb]) / nrm, np.linalg.norm(Xo[:nb] - Xt[:nb]) / nrm
        assert eo <= SPEC_TOL and lo <= SPEC_L2, f"{tag}: oracle spectrum against float64: max {eo:.2e} of the peak, L2 {lo:.2e}"
        assert eg <= SPEC_TOL and lg <= SPEC_L2, f"{tag}: GPU spectrum against float64: max {eg:.2e} of the peak, L2 {lg:.2e}"
        assert lg <= GPU_L2, f"{tag}: GPU relative L2 {lg:.2e} against float64 (oracle {lo:.2e})"
        assert lg <= GPU_OVER_ORACLE * lo, f"{tag}: GPU relative L2 {lg:.2e} is {lg / lo:.2f} x the oracle's {lo:.2e}"
        if is_real:  # the un-normalised bin N/2 (src/fft_impl.cpp:156-160 never visits it)
            assert abs(Xg[N // 2] - Xt[N // 2]) <= 1e-4 * np.abs(Xt[N // 2:]).max() + 1e-4 * peak * N, tag
            assert abs(Xo[N // 2] - Xt[N // 2]) <= 1e-4 * np.abs(Xt[N // 2:]).max() + 1e-4 * peak * N, tag
        worst["spec_max_gpu"], worst["spec_max_orc"] = max(worst["spec_max_gpu"], eg), max(worst["spec_max_orc"], eo)
        worst["spec_l2_gpu"], worst["spec_l2_orc"] = max(worst["spec_l2_gpu"], lg), max(worst["spec_l2_orc"], lo)
        worst["l2_ratio"] = max(worst["l2_ratio"], lg / lo)
    row = dict(test="truth", shape=_tag(N, is_real), fft_size=N, is_real=is_real, frames=F, window=wsrc,
               **{k: float(v) for k, v in worst.items()})
    _record(row)
    print(json.dumps(row))


def _run_engine(sps, N, is_real, clients, waterfalls, splits, fmt="s16", audio_sps=12000, waterfall_size=1024, seed=77):
    """SpectrumEngine over a raw ring for sum(splits) frames, everything against the oracle as
    test_gpu_fullsize.run_workload does - with the oracle's clients at audio_sps.
    clients: (mode, l, m, r); waterfalls: (level, l, r) or callables of the engine's params giving them."""
    from phantomsdr_amd import SpectrumEngine
    nframes, F = sum(splits), max(splits)
    eng = SpectrumEngine(sps, N, is_real, input_format=fmt, audio_sps=audio_sps, waterfall_size=waterfall_size,
                         max_batch=F, max_clients=max(len(clients), 1), max_waterfall_clients=max(len(waterfalls), 1))
    try:
        p = eng.params
        R, n, levels, skip = p["fft_result_size"], p["audio_fft_size"], p["downsample_levels"], p["skip_num"]
        clients = [c(p) if callable(c) else c for c in clients]
        waterfalls = [w(p) if callable(w) else w for w in waterfalls]
        raw, halves = _stream(N, is_real, nframes, seed, fmt)
        eng.upload_ring(raw)
        gcl = [eng.add_audio_client(l, m, r, mode) for mode, l, m, r in clients]
        gwf = [eng.add_waterfall_client(lv, l, r) for lv, l, r in waterfalls]
        ocl = []
        for mode, l, m, r in clients:
            o = O.AudioClient(is_real, n, audio_sps, R)
            o.set_audio_demodulation(mode)
            o.set_audio_range(l, m, r)
            ocl.append(o)
        fo = O.FFT(N, is_real, levels, 0, n)
        nb = N // 2 if is_real else N
        frame = 0
        for nf in splits:
            first = eng.frame_num
            eng.step(frame, nf)
            got = [g.read_audio(nf) for g in gcl]
            wrows = [w.read_waterfall()[0] for w in gwf]
            si = 0
            for f in range(nf):
                fo.load(halves[frame], halves[frame + 1])
                fo.execute()
                spec_o = fo.output().copy()
                tag = f"N=2^{N.bit_length() - 1} real={is_real} n={n} frame {frame}"
                Xg = eng.ctx.read_spectrum(f)
                assert rel_err(Xg[:nb], spec_o[:nb]) < SPEC_TOL, tag
                assert rel_l2(Xg[:nb], spec_o[:nb]) < SPEC_L2, tag
                qg = eng.ctx.read_quantized(f)
                _check_pyramid(qg, Xg, fo.quantized().copy(), N, is_real, levels, tag)
                if (first + f) % skip == 0:
                    for wi, (lv, l, r) in enumerate(waterfalls):
                        row_g = wrows[wi][si]
                        assert np.array_equal(row_g, eng.ctx.quantized_level(qg, lv)[l:r]), f"{tag} waterfall {wi}"
                        d = np.abs(row_g.astype(np.int16) - fo.quantized_level(lv)[l:r].astype(np.int16))
                        assert d.max() <= 1 and (d != 0).mean() <= 5e-3, f"{tag} waterfall {wi} vs oracle"
                    si += 1
                for ci, o in enumerate(ocl):
                    a_o, p_o, _, dropped = o.send_audio(spec_o, first + f, fft=fo)
                    _check_audio(f"{tag} client {ci} {clients[ci]}", o.mode, got[ci][0][f], got[ci][1][f],
                                 got[ci][2][f], a_o, p_o, dropped, o)
                frame += 1
            for wi in range(len(waterfalls)):
                assert wrows[wi].shape[0] == si, "number of sent waterfall rows"
        return p
    finally:
        eng.close()


# (N, is_real, sps): n = 1008 (16 9 7), 1536 (16 16 6), 1260 (12 15 7), 1008
NEW_SHAPES = [(1 << 22, False, 50_000_000), (1 << 18, True, 2_048_000), (1 << 20, True, 10_000_000),
              (1 << 23, True, 100_000_000)]


@pytest.mark.parametrize("N,is_real,sps", NEW_SHAPES, ids=[_tag(N, r) for N, r, _ in NEW_SHAPES])
def test_clients_on_shapes_no_other_test_runs(N, is_real, sps):
    """USB at the upper spectrum edge, LSB, AM on synth_stream's AM carrier, FM on its FM carrier; one waterfall at
    level 0 and one over the whole span at the deepest level; batches of 3 + 2 frames, all against the oracle."""
    b3, b5 = int(3000 * N / sps), int(5000 * N / sps)
    to_c = (lambda k: k) if is_real else (lambda k: (k - (N // 2 + 1)) % N)
    k_am, k_fm = to_c(int(0.11 * N)), to_c(int(0.31 * N) if is_real else int(-0.21 * N) % N)
    R = N // 2 if is_real else N
    clients = [("USB", R - 1 - b3, float(R - 1 - b3), R - 1), ("LSB", k_am - 700 - b3, float(k_am - 700), k_am - 700),
               ("AM", k_am - b5, float(k_am), k_am + b5), ("FM", k_fm - b5, k_fm + 0.5, k_fm + b5)]
    waterfalls = [(0, R // 3, R // 3 + 1024), lambda p: (p["downsample_levels"] - 1, 0, R >> (p["downsample_levels"] - 1))]
    _run_engine(sps, N, is_real, clients, waterfalls, (3, 2), seed=N.bit_length())


# ---- 2. every pyramid depth on every epilogue family -----------------------------------------------------------------
# (N, is_real, LT, ng): the levels the second pass (IQ, fused real) or k_untangle_real (three-pass real) finishes are
# 0..LT; ng > 0: k_col_tail takes log2(ng) more levels inside a row before k_pyramid_tail's launches of 7 levels
FAMILIES = [
    (1 << 12, False, 4, 0),    # (64, 64)
    (1 << 16, False, 4, 0),    # (256, 64)
    (1 << 18, False, 4, 0),    # (512, 32)
    (1 << 20, False, 4, 64),   # (1024, 16), tile-major lines
    (1 << 21, False, 4, 128),  # (1024, 16), pass-1 tiles of 8
    (1 << 22, False, 3, 0),    # (2048, 8), records of 8 bins
    (1 << 13, True, 8, 0),     # three-pass + untangle, (64, 64)
    (1 << 17, True, 8, 0),     # (256, 64)
    (1 << 20, True, 8, 0),     # (512, 32)
    (1 << 23, True, 8, 0),     # (2048, 8), non-fused
    (1 << 21, True, 3, 128),   # fused, octet records
    (1 << 22, True, 2, 256),   # fused, quartet records side by side
]


def depths(N, is_real, LT, ng):
    R = N // 2 if is_real else N
    mx = R.bit_length()  # log2(R) + 1: the last level is one bin
    d = levels_for(R)
    want = [1, 2, LT, LT + 1, LT + 2, d - 1, d, d + 1, LT + 7, LT + 8, mx - 1, mx]
    if ng:
        c = LT + ng.bit_length() - 1  # the first level k_pyramid_tail takes after the column tail
        want += [c, c + 1, c + 7, c + 8]
    return sorted({min(max(v, 1), mx) for v in want})


def _fam_id(fam):
    return _tag(fam[0], fam[1])


@pytest.mark.parametrize("N,is_real,LT,ng", FAMILIES, ids=[_fam_id(f) for f in FAMILIES])
def test_every_pyramid_depth(N, is_real, LT, ng):
    from phantomsdr_amd import Context, WaterfallClient
    R = N // 2 if is_real else N
    F = 2
    raw, _ = _stream(N, is_real, F, seed=900 + N.bit_length() + (50 if is_real else 0))
    ds = depths(N, is_real, LT, ng)
    mx = ds[-1]
    assert mx == R.bit_length()
    spec0, level_bytes = None, {}   # level -> per frame bytes, from the first depth that has the level
    rng = np.random.default_rng(N.bit_length())
    for depth in ds:
        shallow, deepest = depth == ds[1], depth == mx
        nw = 2 * depth + 2 if deepest else 2
        ctx = Context(N, is_real, depth, input_format="s16", max_batch=F, max_waterfall_clients=nw)
        try:
            wfs = []
            if shallow or deepest:
                # the default client: set_waterfall_range(levels - 1, 0, min_waterfall_fft) (src/websocket.cpp:198), the
                # whole span at the coarsest level - on_window_message's own choice for [0, R)
                wd = WaterfallClient(ctx)
                lv_d, l_d, r_d = O.waterfall_pick_level(depth, R >> (depth - 1), 0, R)
                assert (lv_d, l_d, min(r_d, R >> lv_d)) == (depth - 1, 0, R >> (depth - 1))
                wfs.append((wd, depth - 1, 0, R >> (depth - 1)))
                wz = WaterfallClient(ctx)
                for _ in range(20):
                    l = int(rng.integers(0, R - 1))
                    r = int(rng.integers(l + 1, R + 1))
                    lv, ol, orr = O.waterfall_pick_level(depth, R >> (depth - 1), l, r)
                    assert wz.on_window_message(l, r), (depth, l, r)
                    assert (wz.level, wz.l, wz.r) == (lv, ol, min(orr, R >> lv)), (depth, l, r)
                wfs.append((wz, wz.level, wz.l, wz.r))
            if deepest:  # one client per level over its whole range, one over a seeded sub-range (the 2- and 1-bin levels too)
                for lv in range(depth):
                    ln = R >> lv
                    w = WaterfallClient(ctx)
                    w.set_waterfall_range(lv, 0, ln)
                    wfs.append((w, lv, 0, ln))
                    l = int(rng.integers(0, ln))
                    r = int(rng.integers(l + 1, ln + 1))
                    w = WaterfallClient(ctx)
                    w.set_waterfall_range(lv, l, r)
                    wfs.append((w, lv, l, r))
            spec, q = _process(ctx, raw, (F,))
            if wfs:
                ctx.waterfall_batch(0)  # (skip_num 1: every frame is sent)
                for w, lv, l, r in wfs:
                    rows, labels = w.read_waterfall()
                    assert labels == (l << lv, r << lv), (depth, lv, l, r, labels)
                    assert rows.shape == (F, r - l), (depth, lv, l, r, rows.shape)
                    for f in range(F):
                        assert np.array_equal(rows[f], ctx.quantized_level(q[f], lv)[l:r]), \
                            f"depth {depth}: waterfall rows of level {lv} [{l}, {r}) frame {f}"
        finally:
            ctx.close()
        assert ctx.q_len == sum(R >> i for i in range(depth))
        for f in range(F):
            tag = f"{_tag(N, is_real)} depth {depth} frame {f}"
            q_self = O.pyramid_from_spectrum(spec[f], N, is_real, depth)
            bad = q[f] != q_self
            assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} pyramid entries differ from the reference quantiser on the GPU's own spectrum"
        if spec0 is None:
            spec0 = spec
        for f in range(F):
            assert np.array_equal(spec[f].view(np.uint32), spec0[f].view(np.uint32)), f"depth {depth} changes frame {f}'s spectrum"
        off = 0
        for lv in range(depth):
            ln = R >> lv
            cur = [q[f][off:off + ln].copy() for f in range(F)]
            if lv in level_bytes:
                for f in range(F):
                    assert np.array_equal(cur[f], level_bytes[lv][f]), f"level {lv} of frame {f} differs at depth {depth}"
            else:
                level_bytes[lv] = cur
            off += ln
    row = dict(test="depths", shape=_tag(N, is_real), fft_size=N, is_real=is_real, LT=LT, ng=ng, depths=ds, cases=len(ds))
    _record(row)
    print(json.dumps(row))


# ---- 3. the reference's shipped configuration files --------------------------------------------------------------------
# file, input format, sps, FFT size, audio_sps, waterfall_size (all IQ)
REF_CONFIGS = [
    ("config.toml", "s16", 20_000_000, 1 << 20, 192_000, 2048),
    ("config.430.toml", "s16", 20_000_000, 1 << 20, 48_000, 1024),
    ("config.example.hackrf.toml", "s16", 20_000_000, 1 << 20, 192_000, 1024),
    ("config.example.rtlsdr.toml", "u8", 2_880_000, 1 << 17, 12_000, 1024),
    ("config.example.file.toml", "s16", 192_000, 1 << 15, 12_000, 2048),
]


@pytest.mark.parametrize("cfg", REF_CONFIGS, ids=[c[0] for c in REF_CONFIGS])
def test_reference_configurations(cfg):
    """Each shipped configuration for 3 + 2 frames: two clients per mode, a zoomed waterfall and the full span."""
    name, fmt, sps, N, audio_sps, wsize = cfg
    expect_n = {"config.toml": 10068, "config.430.toml": 2520, "config.example.hackrf.toml": 10068,
                "config.example.rtlsdr.toml": 548, "config.example.file.toml": 2048}[name]
    from phantomsdr_amd import derived_params
    p = derived_params(sps, N, False, audio_sps, wsize)
    assert p["audio_fft_size"] == expect_n
    rng = np.random.default_rng(len(name))
    b3 = max(2, int(3000 * N / sps))
    b5 = max(2, int(5000 * N / sps))
    wide = max(b5, int(min(0.45 * audio_sps, 100_000) * N / sps))   # WBFM-width windows where the audio rate allows it
    clients = []
    for i, mode in enumerate(["USB", "LSB", "AM", "FM"] * 2):
        m = int(rng.uniform(0.05 * N, 0.95 * N))
        h = min(wide if (mode == "FM" and i >= 4) else b5, expect_n // 2 - 1)
        clients.append({"USB": (mode, m, float(m), m + b3), "LSB": (mode, m - b3, float(m), m)}.get(mode, (mode, m - h, float(m), m + h)))
    lv = p["downsample_levels"]
    waterfalls = [(lv - 1, 0, N >> (lv - 1)), (max(lv - 3, 0), 100, 100 + min(wsize, N >> max(lv - 3, 0)) - 200)]
    _run_engine(sps, N, False, clients, waterfalls, (3, 2), fmt=fmt, audio_sps=audio_sps, waterfall_size=wsize, seed=len(name) + 3)

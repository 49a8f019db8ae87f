"""The noise reduction's host side (phantomsdr_amd/csrc/nrplan.h) without a GPU: tests/nr_plan_table.cpp is compiled with the host
C++ compiler - the header is plain C++17, and its windows, butterflies and gain rule are the text k_audio_nr runs - and driven by
the scripts below.  The measured figures go to build/records/nr_host.jsonl."""
import ctypes
import functools
import json
import math
import os
import subprocess

import numpy as np
import pytest

import nr_model as M
from conftest import ROOT
from helpers import CLIENT_KINDS
from test_demod_plan import client, kind

RATE = 12000
NAMES = list(CLIENT_KINDS)
AUDIO_KINDS = [k for k in NAMES if CLIENT_KINDS[k][0] != "IQ"]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("nr_host")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


def run(exe, text, timeout=120):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def fields(ln):
    return dict(kv.split("=", 1) for kv in ln.split()[1:])


def record(name, **figures):
    d = os.path.join(ROOT, "build", "records")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "nr_host.jsonl"), "a") as f:
        f.write(json.dumps(dict(test=name, **figures)) + "\n")


def batches_of(split, F):
    out, left, k = [], F, 0
    while left > 0:
        out.append(min(split[k % len(split)], left))
        left -= out[-1]
        k += 1
    return out


@functools.lru_cache(maxsize=None)
def noise(n, seed=20261020):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def bits(v):
    return int(np.float32(v).view(np.uint32))


# ---- the tables and the transform pair ----------------------------------------------------------------------------------------
def test_tables_are_rounded_once_from_double(exe, tmp):
    win, tw = M.tables(exe, tmp)
    n = np.arange(M.M)
    # sin(pi n / 256) IS the periodic square-root Hann window; another libm may differ in the last place of the double
    want = np.sin(np.pi * n / M.M)
    assert np.all(np.abs(win.astype(np.float64) - want) <= np.spacing(want.astype(np.float32)).astype(np.float64) * 0.5000001)
    assert np.all(np.abs(win.astype(np.float64) ** 2 - (0.5 - 0.5 * np.cos(2 * np.pi * n / M.M))) < 1.3e-7)
    assert np.all(np.abs(tw[:, 0] - np.cos(2 * np.pi * n / M.M)) <= 3.0e-8) and np.all(np.abs(tw[:, 1] + np.sin(2 * np.pi * n / M.M)) <= 3.0e-8)
    assert win[0] == 0.0 and win[128] == 1.0 and tuple(tw[0]) == (1.0, 0.0) and tw[64][1] == -1.0 and tw[128][0] == -1.0


def test_unit_gain_is_the_input_delayed_by_256(exe, tmp):
    """depth_db = 0: g_min = 1, every gain is 1 and the output is the input 256 samples late.  The bound: 4 x the largest difference
    the float64 restatement over the same f32 tables shows against the delayed input, on each input"""
    win, tw = M.tables(exe, tmp)
    t = np.arange(180 * 40)
    inputs = {"noise": noise(180 * 40), "tone": np.cos(2 * np.pi * 1000.0 * t / RATE + 0.3).astype(np.float32)}
    for name, x in inputs.items():
        want = np.zeros(len(x))
        want[M.M:] = x[:-M.M]
        full = slice(M.M + M.R, None)  # (the stream's first hop lies under one block only: its window squared, not 1)
        own = float(np.abs(M.restated_unit_gain(x, win, tw) - want)[full].max())
        (got, states, gains), = M.run_streams(exe, tmp, [(0.0, 1.0, x, np.zeros(40, np.int32), 180, [40])], "unit")
        err = float(np.abs(got.astype(np.float64) - want)[full].max())
        print(f"{name}: restatement {own:.3e} nr_stream {err:.3e} ratio {err / own:.2f}")
        record("unit_gain", input=name, restatement_max_abs=own, nr_stream_max_abs=err, bound=4 * own)
        assert np.all(gains == 1.0) and not got[:M.M].any() and not np.signbit(got[:M.M]).any()
        assert err <= 4 * own, (name, err, own)


# ---- batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", (4, 6, 180))
def test_any_split_into_batches_gives_the_same_bits(exe, tmp, h):
    F = 147 if h < 180 else 75
    x = noise(h * F)
    x = (x + 4 * np.cos(2 * np.pi * 0.11 * np.arange(h * F))).astype(np.float32)
    flags = np.zeros(F, np.int32)
    splits = [(F,), (1,), (2,), (3,), (70,), (71,), (1, 2, 3, 70, 71), (71, 3, 1)]
    res = M.run_streams(exe, tmp, [(14.0, 1.5, x, flags, h, batches_of(s, F)) for s in splits], "split%d_" % h)
    rows0, st0, g0 = res[0]
    assert len(g0) == ((h * F - M.M) // M.R + 1 if h * F >= M.M else 0) and int(st0[-1]["pos"]) == h * F
    for s, (rows, st, g) in zip(splits[1:], res[1:]):
        assert rows.tobytes() == rows0.tobytes(), s
        assert g.tobytes() == g0.tobytes() and st[-1].tobytes() == st0[-1].tobytes(), s
    if len(g0):
        assert g0.min() >= 10 ** (-14 / 20) * (1 - 1e-7) and g0.max() <= 1.0 and g0.min() < 0.9


def test_contraction_cannot_change_a_bit(exe, tmp):
    """the table program built to fuse whatever may be fused (-mfma -ffp-contract=fast, -O2) against one that may fuse nothing"""
    if " fma " not in open("/proc/cpuinfo").read():
        pytest.skip("this CPU has no FMA instruction to contract into")
    fast = M.build_table(tmp, ROOT, ("-O2", "-mfma", "-ffp-contract=fast"), "nr_plan_table_fast")
    off = M.build_table(tmp, ROOT, ("-O2", "-ffp-contract=off"), "nr_plan_table_off")
    jobs = [(14.0, 1.5, (noise(180 * 30) + np.cos(0.7 * np.arange(180 * 30))).astype(np.float32), np.zeros(30, np.int32), 180, [30])]
    (ra, sa, ga), (rb, sb, gb) = M.run_streams(fast, tmp, jobs, "fast")[0], M.run_streams(off, tmp, jobs, "off")[0]
    assert ra.tobytes() == rb.tobytes() and sa.tobytes() == sb.tobytes() and ga.tobytes() == gb.tobytes()
    assert ra.tobytes() == M.run_streams(exe, tmp, jobs, "o1")[0][0].tobytes()


def test_a_flagged_frame_enters_as_zeros_and_keeps_its_row(exe, tmp):
    for h in (4, 6, 180):
        F = 150 if h < 180 else 12
        x = noise(h * F).copy()
        flags = np.zeros(F, np.int32)
        bad = [F // 3, F // 3 + 1, F - 2]
        flags[bad] = 1
        for f in bad:
            x[f * h] = np.nan
            x[f * h + 1:(f + 1) * h].view(np.uint32)[:] = 0x7FC01234
        clean = np.where(np.repeat(flags, h) != 0, np.float32(0), x)
        jobs = [(14.0, 1.5, x, flags, h, batches_of(s, F)) for s in ((F,), (1,), (3, 70))] + [(14.0, 1.5, clean, np.zeros(F, np.int32), h, [F])]
        res = M.run_streams(exe, tmp, jobs, "flag")
        keep = np.repeat(flags, h) == 0
        for rows, st, g in res[:3]:
            assert rows[~keep].tobytes() == x[~keep].tobytes()  # NaN bits included
            assert rows[keep].tobytes() == res[3][0][keep].tobytes() and np.isfinite(rows[keep]).all()
            assert st[-1].tobytes() == res[3][1][-1].tobytes()  # the state went on as over zeros


def test_a_bin_of_non_finite_power_keeps_its_records_and_gets_g_min(exe, tmp):
    """a tone of 1e19 on bin 32: the powers of bins 31..33 overflow to +Inf, the others stay finite"""
    h, F1, F2 = 128, 8, 2
    x = noise(h * (F1 + F2)).copy()
    x[h * F1:] += (1e19 * np.cos(2 * np.pi * 32 * np.arange(h * F2) / M.M)).astype(np.float32)
    (rows, st, g), = M.run_streams(exe, tmp, [(14.0, 1.5, x, np.zeros(F1 + F2, np.int32), h, [F1, F2])], "inf")
    g_min = np.float32(10 ** (-14 / 20))
    nb1 = (h * F1 - M.M) // M.R + 1
    hit = g[nb1 + 1:]  # (the first block of the second batch is half tone)
    assert len(hit) >= 1 and np.all(hit[:, 31:34] == g_min)
    for name in ("Ps", "N", "G"):
        assert st[1][name][32] == st[0][name][32] and np.isfinite(st[1][name][:M.BINS]).all()
        assert not np.array_equal(st[1][name][:20], st[0][name][:20])  # the other bins went on
    assert np.all((g >= g_min) & (g <= 1))


def test_the_gain_never_leaves_its_range(exe, tmp):
    x = np.concatenate([noise(6000), np.zeros(3000, np.float32), 100 * noise(3000, 7), 1e-30 * noise(3000, 8), noise(3000, 9)]).astype(np.float32)
    jobs = [(d, b, x, np.zeros(len(x) // 6, np.int32), 6, [len(x) // 6]) for d, b in ((0.0, 0.5), (3.0, 4.0), (8.0, 1.0), (22.0, 2.0), (40.0, 4.0), (40.0, 0.5))]
    for (d, b, *_), (rows, st, g) in zip(jobs, M.run_streams(exe, tmp, jobs, "range")):
        g_min = np.float32(10 ** (-d / 20))
        assert g.min() >= g_min and g.max() <= 1.0 and np.isfinite(rows).all(), (d, b)
        for name in ("G",):
            assert np.all((st[-1][name][:M.BINS] >= g_min) & (st[-1][name][:M.BINS] <= 1))


# ---- refusals, presets ----------------------------------------------------------------------------------------------------------
REFUSALS = [
    ("id below 0", "nr -1 1 14 1.5", "BAD_ID"), ("id past the slots", "nr 8 1 14 1.5", "BAD_ID"), ("id past the slots, off", "nr 9 0 0 0", "BAD_ID"),
    ("no client", "nr 4 1 14 1.5", "INACTIVE"), ("no client, off", "nr 4 0 0 0", "INACTIVE"),
    ("IQ client", "nr 2 1 14 1.5", "IQ"),
    ("NaN depth", "nr 0 1 nan 1.5", "NONFINITE"), ("Inf beta", "nr 0 1 14 inf", "NONFINITE"), ("-Inf depth", "nr 0 1 -inf 1.5", "NONFINITE"),
    ("depth below 0", "nr 0 1 -0.5 1.5", "BAD_DEPTH"), ("depth above 40", "nr 0 1 40.5 1.5", "BAD_DEPTH"),
    ("beta below 0.5", "nr 0 1 14 0.25", "BAD_BETA"), ("beta above 4", "nr 0 1 14 4.5", "BAD_BETA"),
    # the precedence: id, client, IQ, non-finite, depth, beta, rate
    ("id before everything", "nr 8 1 nan 9", "BAD_ID"), ("client before IQ and numbers", "nr 4 1 nan 9", "INACTIVE"), ("IQ before the numbers", "nr 2 1 nan 9", "IQ"),
    ("non-finite beta before depth", "nr 0 1 99 nan", "NONFINITE"), ("depth before beta", "nr 0 1 99 9", "BAD_DEPTH"),
]
ACCEPTED = ["nr 0 1 0 0.5", "nr 0 1 40 4", "nr 2 0 nan nan", "nr 0 0 99 99"]


def test_refusals_in_order_and_nothing_changes(exe):
    lines = ["case validation", *client(0, "USB"), *client(1, "AM"), *client(2, "IQ"), "nr 1 1 14 1.5", "dump"]
    for _, line, _ in REFUSALS:
        lines += [line, "dump"]
    lines += ["rate 0", "nr 0 1 14 1.5", "dump", "nr 0 1 99 9", "rate 12000"]
    for line in ACCEPTED:
        lines += [line, "dump"]
    out = run(exe, "\n".join(lines) + "\n").splitlines()
    sets = [i for i, ln in enumerate(out) if ln.startswith("set ")]
    verdicts = [fields(out[i])["verdict"] for i in sets]
    dumps = [out[i + 1:i + 9] for i in sets]
    base = dumps[0]
    f1 = fields(base[1])
    assert verdicts[0] == "OK" and (f1["on"], f1["fresh"]) == ("1", "1") and int(f1["g_min"]) == bits(10 ** (-14 / 20)) and int(f1["beta"]) == bits(1.5)
    assert {v for _, _, v in REFUSALS} == {"BAD_ID", "INACTIVE", "IQ", "NONFINITE", "BAD_DEPTH", "BAD_BETA"}
    for k, (what, _, verdict) in enumerate(REFUSALS, 1):
        assert verdicts[k] == verdict, what
        assert dumps[k] == base, what
    a = len(REFUSALS) + 1
    assert verdicts[a] == "NO_RATE" and dumps[a] == base and verdicts[a + 1] == "BAD_DEPTH"  # the rate is looked at last
    assert verdicts[a + 2:] == ["OK"] * len(ACCEPTED)
    d = [fields(x[0]) for x in dumps[a + 2:]]
    assert (d[0]["on"], int(d[0]["g_min"]), int(d[0]["beta"])) == ("1", bits(1.0), bits(0.5))  # the limits themselves pass
    assert (d[1]["on"], int(d[1]["g_min"]), int(d[1]["beta"])) == ("1", bits(0.01), bits(4.0))
    assert d[3]["on"] == "0" and int(d[3]["g_min"]) == bits(0.01)  # off ignores the numbers


def test_presets(exe):
    out = [fields(ln) for ln in run(exe, "".join("preset %d\n" % k for k in (0, 1, 2, 3, 4, -1))).splitlines()]
    assert [(o["ok"], float(o["depth"]), float(o["beta"])) for o in out[1:4]] == [("1", 8.0, 1.0), ("1", 14.0, 1.5), ("1", 22.0, 2.0)]
    assert [o["ok"] for o in out] == ["0", "1", "1", "1", "0", "0"]


# ---- plausibility ---------------------------------------------------------------------------------------------------------------
def test_noise_goes_down_and_a_tone_loses_less(exe, tmp):
    """One stream of 4 s: white noise alone, then a steady tone 20 dB over the noise in its bin on top of it.  The noise is alone
    for 3 s - one time constant of the rising noise track, what a fresh track needs to settle when the stream's first block was a
    low one - and the tone holds the fourth second.  The noise attenuation is that of the last second of noise alone, [2 s, 3 s);
    the tone's loss is taken at the end of the stream, over its last quarter second (the loss only grows while the tone is on, so
    this is its largest).  Asserted, per preset: 0 < attenuation <= depth_db, and the tone loses less than the noise.

    Recorded beside it and NOT asserted (a limit of the rule): a tone that is there for all of a 4 s stream.  The track
    rises to a steady power with its 3 s time constant, so such a tone is taken for noise - it loses 7.7 / 13.4 / 20.7 dB where
    noise alone loses 3.9 / 6.3 / 9.0 dB (light / normal / strong)."""
    n = 4 * RATE
    n -= n % 180
    on = 3 * RATE
    w = noise(n)
    # the noise in one bin of the windowed transform: sigma^2 * sum(win^2) = 128; the tone's power there: (A / 2)^2 * (sum win)^2
    swin = float(np.sin(np.pi * np.arange(M.M) / M.M).sum())
    A = 2 * math.sqrt(100 * 128) / swin
    steady = (A * np.cos(2 * np.pi * 40 * np.arange(n) / M.M)).astype(np.float32)
    tone = steady.copy()
    tone[:on] = 0
    ref = np.exp(-2j * np.pi * 40 * np.arange(n) / M.M)

    def delayed(x):
        return np.concatenate([np.zeros(M.M, np.float32), x[:-M.M]]).astype(np.float64)

    def power_db(x, y, s):
        return 10 * math.log10(float(np.mean(delayed(x)[s] ** 2)) / float(np.mean(y[s].astype(np.float64) ** 2)))

    def tone_db(x, y, s):
        return 20 * math.log10(abs(np.vdot(ref[s], delayed(x)[s])) / abs(np.vdot(ref[s], y[s])))
    figures = []
    for depth, beta in ((8.0, 1.0), (14.0, 1.5), (22.0, 2.0)):
        streams = ((w + tone).astype(np.float32), w, (w + steady).astype(np.float32))
        (r, _, _), (rn, _, _), (rs, _, _) = M.run_streams(exe, tmp, [(depth, beta, x, np.zeros(n // 180, np.int32), 180, [n // 180]) for x in streams], "plaus")
        att = power_db(streams[0], r, slice(2 * RATE + M.M, on + M.M))
        loss = tone_db(streams[0], r, slice(n - RATE // 4, n))
        att4, loss4 = power_db(w, rn, slice(n - RATE, n)), tone_db(streams[2], rs, slice(n - RATE, n))
        print(f"depth {depth} beta {beta}: noise attenuation {att:.2f} dB, tone loss {loss:.2f} dB; a tone of 4 s: {att4:.2f} / {loss4:.2f} dB")
        record("plausibility", depth_db=depth, beta=beta, noise_attenuation_db=att, tone_loss_db=loss, noise_alone_4s_db=att4, steady_tone_4s_loss_db=loss4)
        figures.append((depth, att, loss))
    for depth, att, loss in figures:
        assert 0 < att <= depth, (depth, att)
    for depth, att, loss in figures:
        assert loss < att, figures


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def entries(p):
    return [tuple(int(v) for v in e.split(":")) for e in p["list"].split(",")] if p["list"] else []


def zero(p):
    return [int(v) for v in p["zero"].split(",")] if p["zero"] else []


def test_plan_who_is_listed_and_whose_state_is_fresh(exe):
    P = len(NAMES)  # the paused client's slot
    iq = NAMES.index("IQ")
    lines = ["case plan", "size 16 360 5"]
    for i, k in enumerate(NAMES):
        lines += client(i, k) + (["nr %d 1 14 1.5" % i] if CLIENT_KINDS[k][0] != "IQ" else [])
    lines += client(P, "USB") + ["nr %d 1 8 1" % P, "pause %d" % P, "batch",  # 0
                                 "batch",  # 1: nobody fresh
                                 "nr 0 1 22 2", "resume %d" % P, "batch",  # 2: new numbers: fresh; switched on while paused: fresh now
                                 kind(NAMES.index("AM"), "FM"), "window 1 30 35.5 40", "window 3 10 15.75 20", "window 4 10 16.25 20", "batch",  # 3: mode; retune; mid inside its bin; floor(mid)
                                 kind(0, "IQ"), "batch", kind(0, "USB"), "batch",  # 4, 5: USB -> IQ -> USB: not listed, then the state stood still
                                 "nr 6 0 0 0", "remove 3", "add 3", kind(3, "FM"), "window 3 10 15.25 20", "batch",  # 6: off; a fresh slot comes without
                                 "nr 6 1 14 1.5", "batch",  # 7: off and on again: fresh
                                 ]
    for i in range(P + 1):
        lines.append("nr %d 0 0 0" % i)
    lines += ["batch"]  # 8: nobody
    b = [fields(ln) for ln in run(exe, "\n".join(lines) + "\n").splitlines() if ln.startswith("nrp ")]
    audio = [NAMES.index(k) for k in AUDIO_KINDS]
    am = NAMES.index("AM")
    assert len(audio) == 9 and [e[0] for e in entries(b[0])] == audio and zero(b[0]) == audio  # IQ, TIQ and the paused one are not listed
    a_up = bits(1 - math.exp(-128 / (3.0 * 12000)))
    assert all(e[1:] == (bits(10 ** (-14 / 20)), bits(1.5), a_up) for e in entries(b[0]))
    assert [e[0] for e in entries(b[1])] == audio and zero(b[1]) == []
    assert [e[0] for e in entries(b[2])] == audio + [P] and zero(b[2]) == [0, P] and entries(b[2])[0][1:3] == (bits(10 ** (-22 / 20)), bits(2.0))
    assert zero(b[3]) == sorted([am, 1, 4]) and 3 not in zero(b[3])
    assert 0 not in [e[0] for e in entries(b[4])] and zero(b[4]) == []
    assert 0 in [e[0] for e in entries(b[5])] and zero(b[5]) == []
    assert [e[0] for e in entries(b[6])] == [i for i in audio + [P] if i not in (3, 6)] and zero(b[6]) == []
    assert zero(b[7]) == [6]
    assert b[8]["any"] == "0" and entries(b[8]) == [] and zero(b[8]) == []


def test_plan_of_a_context_without_such_clients(exe):
    lines = ["case none", *client(0, "USB"), *client(1, "AM"), "batch", "batch"]
    b = [fields(ln) for ln in run(exe, "\n".join(lines) + "\n").splitlines() if ln.startswith("nrp ")]
    assert len(b) == 2 and all(x["have"] == "0" and x["any"] == "0" and x["list"] == "" for x in b)


def test_the_demodulation_plan_does_not_know_the_noise_reduction(exe):
    def script(with_nr):
        out = ["case ring", "size 12 360 5", "post on"]
        for i, k in ((0, "USB"), (1, "IQ"), (2, "TUSB"), (3, "SAMU"), (7, "FM"), (8, "TIQ")):
            out += client(i, k) + (["nr %d 1 14 1.5" % i] if with_nr else [])
        return out + ["batch", "pause 2", "batch", "post off", "resume 2", "batch"]
    plan = lambda text: [ln for ln in text.splitlines() if not ln.startswith(("nrp ", "set "))]  # noqa: E731
    assert plan(run(exe, "\n".join(script(True)) + "\n")) == plan(run(exe, "\n".join(script(False)) + "\n"))


def test_sanitizers(tmp, exe):
    """the table program as a stand-alone program under AddressSanitizer and UBSan: ragged batches at every h, a flagged frame,
    the validation script"""
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    probe = tmp / "sanitizer_probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17", *flags, str(probe), "-o", str(tmp / "sanitizer_probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime to link against")
    san = M.build_table(tmp, ROOT, flags, "nr_plan_table_san")
    jobs = []
    for h, F in ((4, 1), (4, 63), (4, 64), (4, 200), (6, 43), (6, 150), (180, 1), (180, 2), (180, 9)):
        fl = np.zeros(F, np.int32)
        fl[F // 2] = F > 4
        for s in ((F,), (1,), (3, 70, 1)):
            jobs.append((14.0, 1.5, noise(h * F), fl, h, batches_of(s, F)))
    for (ra, sa, ga), (rb, sb, gb) in zip(M.run_streams(san, tmp, jobs, "san"), M.run_streams(exe, tmp, jobs, "ref")):
        assert ra.tobytes() == rb.tobytes() and sa.tobytes() == sb.tobytes() and ga.tobytes() == gb.tobytes()
    text = "\n".join(["case v", *client(0, "USB"), *client(2, "IQ")] + [line for _, line, _ in REFUSALS] + ["batch", "nr 0 1 14 1.5", "batch", "dump"]) + "\n"
    r = subprocess.run([san], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == run(exe, text)


def test_abi_symbols_and_constants():
    lib = ctypes.CDLL(os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so"))
    for name in ("psdr_client_set_noise_reduction", "psdr_noise_reduction_preset"):
        assert hasattr(lib, name), name
    import re

    import phantomsdr_amd as p
    from phantomsdr_amd import _lib
    assert {"psdr_client_set_noise_reduction", "psdr_noise_reduction_preset"} <= {s[0] for s in _lib.SYMBOLS}
    hdr = open(os.path.join(ROOT, "include", "psdr.h")).read()
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(PSDR_NR_[A-Z]+|PSDR_OPT_NOISE_REDUCTION)\s+(\d+)", hdr))
    assert defs == {"PSDR_NR_LIGHT": p.NR_LIGHT, "PSDR_NR_NORMAL": p.NR_NORMAL, "PSDR_NR_STRONG": p.NR_STRONG, "PSDR_OPT_NOISE_REDUCTION": p.Context.OPT_NOISE_REDUCTION}
    assert "#define PSDR_ABI_VERSION 3" in hdr
    # the preset helper needs no context (and no device)
    assert [p.noise_reduction_preset(k) for k in ("light", "normal", "strong")] == [(8.0, 1.0), (14.0, 1.5), (22.0, 2.0)]
    with pytest.raises(p.PsdrError) as e:
        p.noise_reduction_preset(0)
    assert e.value.code == -1 and "unknown kind 0" in str(e.value)

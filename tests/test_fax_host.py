"""The radiofax decoder's host side (phantomsdr_amd/csrc/faxplan.h; include/psdr.h: psdr_client_set_fax_decoder), without a device:
tests/fax_plan_table.cpp runs the text k_audio_fax runs, tests/fax_model.py restates the rule in numpy and holds the sender.
The sent picture is the yardstick of the truth tests, not the code."""
import os
import re

import numpy as np
import pytest

import fax_model as M
from conftest import ROOT

NOISE_SEED = 20261021
# Measured with the host program with NOISE_SEED:
#   the largest rho of 120 s of unit noise alone at 12000, 16000 and 48000 Hz: 0.0184 (NOISE_RHO bounds it);
#   the lowest signal-to-noise ratio in 3 kHz (SNR = a^2 / (2 sigma^2) * rate / 6000), in 3 dB steps, at which the 240 lpm sequence
#   still locks: LOWEST_SNR_DB; 3 dB below it no line is kept; the smallest rho of its start tone there: 0.425 (LOWEST_RHO bounds it);
#   the default tone_ratio, half-way between the two: M.TONE_RATIO_DEFAULT;
#   fax_angle's worst error against float64 atan2: 1.85e-7 rad (ANGLE_ERR bounds it);
#   the worst |pix - sent| away from the squares' edges, noise-free, FREE, 12000 Hz, 120 lpm, 256 pixels: FIDELITY levels.
NOISE_RHO, LOWEST_SNR_DB, LOWEST_RHO, ANGLE_ERR, FIDELITY = 0.019, 6.0, 0.42, 2.0e-7, 19
AMP, H180 = 0.5, 180
SEQ = dict(mode=M.AUTO, width=256, start_blocks=4, phase_lines=3)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("fax_host")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


@pytest.fixture(scope="module")
def builds(tmp, exe):
    """the table program as built by default, with contraction on and with contraction off"""
    return [exe, M.build_table(tmp, ROOT, ("-mfma", "-ffp-contract=fast"), "fax_fast"), M.build_table(tmp, ROOT, ("-ffp-contract=off",), "fax_off")]


def sequence(rate, lpm, snr_db=None, h=H180, **tx):
    f, on = M.tx_freq(rate, M.test_image(12, 256), lpm=lpm, **tx)
    x = M.audio(f, on, rate, AMP)
    if snr_db is not None:
        x = x + AMP * np.sqrt(rate / (4 * 3000.0 * 10 ** (snr_db / 10))) * np.random.default_rng(NOISE_SEED).standard_normal(len(x))
    return M.framed(x, h)


def order_of(state):
    return [int(s) for i, s in enumerate(state) if i == 0 or s != state[i - 1]]


def pulse_column(line, wp):
    """the middle of the window of wp circular columns that differs most from the line's median"""
    dev = np.abs(line.astype(int) - int(np.median(line)))
    win = np.convolve(np.r_[dev, dev[:wp]], np.ones(wp), "valid")[:len(line)]
    return (int(np.argmax(win)) + wp // 2) % len(line)


# ---- 1. bit parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,lpm,tones", ((7900, 90.0, (900.0, 1700.0)), (12000, 240.0, (1500.0, 2300.0)), (16000, 240.0, (2300.0, 1500.0)), (48000, 240.0, (1500.0, 2300.0))))
def test_contraction_on_and_off_give_the_models_bits(tmp, builds, rate, lpm, tones):
    rng = np.random.default_rng(rate)
    jobs = []
    for h, mode in ((180, M.AUTO), (256, M.FREE)):
        x, flags = sequence(rate, lpm, h=h, black_hz=tones[0], white_hz=tones[1], phasing=6)
        x = (x + 0.01 * rng.standard_normal(len(x))).astype(np.float32)
        flags[len(flags) // 2] = 1  # a flagged frame enters as zeros
        F = len(flags)
        cfg = dict(SEQ, mode=mode, lpm=lpm, black_hz=tones[0], white_hz=tones[1], phase_col=0 if mode == M.AUTO else 100)
        for frames in ([F], [1] * F, [5, 6] * (F // 11) + ([F % 11] if F % 11 else [])):
            jobs.append((cfg, x, flags, h, frames))
    outs = [M.run_streams(e, tmp, jobs, rate=rate) for e in builds]
    for j, (cfg, x, flags, h, _) in enumerate(jobs):
        rec, lines, meta = M.records(x.reshape(len(flags), h), flags, h, rate, **cfg)
        for o in outs:
            got = o[j]
            wl, wm = M.ring_tail(lines, meta, got[5])
            assert got[0].tobytes() == rec.tobytes() and got[2].tobytes() == wl.tobytes() and got[3].tobytes() == wm.tobytes() and got[4] == len(lines), (rate, h, j)
            assert got[1] == outs[0][j - j % 3][1], "the state behind a split is the state behind the whole"
        assert len(lines) >= 10
        if cfg["mode"] == M.AUTO:
            assert order_of(rec["state"]) == [M.IDLE, M.PHASING, M.IMAGE, M.IDLE]


# ---- 2. truth -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lpm", (240.0, 120.0))
def test_the_sequence_is_found_phased_and_ended(tmp, exe, lpm):
    rate = 12000
    cases = [dict(), dict(dark_pulse=True), dict(start_hz=675.0), dict(offset=0.37 * 60.0 / lpm)]
    jobs = [(dict(SEQ, lpm=lpm), *sequence(rate, lpm, **c), H180, None) for c in cases]
    jobs = [(c, x, f, h, [len(f)]) for c, x, f, h, _ in jobs]
    for c, (rec, _, lines, meta, total, _) in zip(cases, M.run_streams(exe, tmp, jobs, rate=rate)):
        cols = [pulse_column(ln, 12) for ln in lines[:3]]
        print(f"lpm {lpm} {c}: states {order_of(rec['state'])} lines {total} ioc {rec['ioc'][-1]} pulse at {cols} offset {rec['offset_hz'][-1]:.1f} Hz")
        assert order_of(rec["state"]) == [M.IDLE, M.PHASING, M.IMAGE, M.IDLE] and rec["image"][-1] == 1
        assert rec["ioc"][-1] == (288 if c.get("start_hz") == 675.0 else 576)
        assert 12 <= total <= 18 and (meta == (1 << 8 | M.IMAGE)).all()
        # the phasing lines kept behind the lock hold the pulse within width / 64 columns of column 0
        assert all(min(k, 256 - k) <= 256 // 64 for k in cols), cols


def test_fidelity_of_a_ramp_with_a_checkerboard(tmp, exe):
    rate, lpm, width = 12000, 120.0, 256
    img = M.test_image(24, width)
    f, on = M.tx_freq(rate, img, lpm=lpm, lead=0.0, start_s=0.0, phasing=0, stop_s=0.0, tail=0.1)
    rows, flags = M.framed(M.audio(f, on, rate), H180)
    (rec, _, lines, meta, total, _), = M.run_streams(exe, tmp, [(dict(mode=M.FREE, lpm=lpm, width=width), rows, flags, H180, [len(flags)])], rate=rate)
    sent = np.floor(255 * img + 0.5)
    cols = np.flatnonzero((np.arange(width) % 8 >= 2) & (np.arange(width) % 8 <= 5))  # two pixels away from the squares' edges
    err = np.abs(lines[1:24].astype(int) - sent[1:24])[:, cols]
    print(f"fidelity: worst |pix - sent| {err.max()}, mean {err.mean():.2f} levels")
    assert total == 24 and (rec["state"] == M.IMAGE).all() and err.max() <= FIDELITY + 2


def test_fax_angle_against_atan2(tmp, exe):
    rng = np.random.default_rng(5)
    th = np.concatenate([np.linspace(-np.pi / 2, np.pi / 2, 200001)[1:-1], rng.uniform(-np.pi / 2, np.pi / 2, 200000)])
    r = np.exp(rng.uniform(-20, 20, len(th)))
    re, im = (r * np.cos(th)).astype(np.float32), (r * np.sin(th)).astype(np.float32)
    a = M.angles(exe, tmp, re, im)
    assert a.tobytes() == M.angle(re, im).tobytes()
    ok = re > 0
    worst = np.abs(a[ok] - np.arctan2(im[ok].astype(np.float64), re[ok].astype(np.float64))).max()
    # the largest s the call can make: audio_rate 6399 (D = 1) at the narrowest shift
    s_max = 6399.0 / (2 * np.pi * 200.0)
    print(f"fax_angle: worst error {worst:.3g} rad, {worst * s_max * 255:.2g} of a u8 step of v at the largest s")
    assert worst <= ANGLE_ERR and worst * s_max < 0.25 / 255
    sat = M.angles(exe, tmp, [0, -1, -1, 0, np.nan, np.inf, 1], [0, 2, -2, 3, 1, -1, np.inf])
    assert sat.tolist() == [0, float(M.HALF_PI), -float(M.HALF_PI), float(M.HALF_PI), float(M.HALF_PI), -float(M.HALF_PI), float(M.HALF_PI)]


# ---- 3. the default tone_ratio --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", (12000, 16000, 48000))
def test_noise_alone_never_leaves_idle(tmp, exe, rate):
    F = 120 * rate // H180
    x = np.random.default_rng(NOISE_SEED).standard_normal(F * H180).astype(np.float32)
    (rec, _, lines, _, total, _), = M.run_streams(exe, tmp, [(dict(), x, np.zeros(F, np.int32), H180, [F])], rate=rate)
    q = rec["tone_quality"].max()
    print(f"rate {rate}: 120 s of noise alone, the largest rho {q:.4f}")
    assert (rec["state"] == M.IDLE).all() and total == 0 and rec["image"][-1] == 0
    assert q <= NOISE_RHO < M.TONE_RATIO_DEFAULT


def test_the_sequence_at_the_lowest_ratio_that_locks(tmp, exe):
    rate, lpm = 12000, 240.0
    jobs = [(dict(SEQ, lpm=lpm, tone_ratio=0.04), *sequence(rate, lpm, snr_db=s), H180, None) for s in (LOWEST_SNR_DB, LOWEST_SNR_DB - 3)]
    jobs = [(c, x, f, h, [len(f)]) for c, x, f, h, _ in jobs]
    (at, _, _, _, tat, _), (below, _, _, _, tbelow, _) = M.run_streams(exe, tmp, jobs, rate=rate)
    first = int((0.3 + 0.25) * rate / H180)
    last = min(int((0.3 + 1.4) * rate / H180), int(np.flatnonzero(at["state"] == M.PHASING)[0]))
    qmin = at["tone_quality"][first:last].min()
    print(f"{LOWEST_SNR_DB} dB: states {order_of(at['state'])} lines {tat} smallest rho of the start tone {qmin:.4f}; {LOWEST_SNR_DB - 3} dB: lines {tbelow}")
    assert order_of(at["state"]) == [M.IDLE, M.PHASING, M.IMAGE, M.IDLE] and tat >= 12
    assert tbelow == 0  # the measurement, again: 3 dB below nothing is kept
    assert qmin >= LOWEST_RHO and abs(M.TONE_RATIO_DEFAULT - (NOISE_RHO + LOWEST_RHO) / 2) <= 0.0051


# ---- 4. validation, defaults, plan --------------------------------------------------------------------------------------------
OK_TAIL = "1500 2300 120 1024 0 0 0.22 8 4 0"
VERDICTS = [  # in the order they are looked for: each call holds every later fault too
    ("fax 9 1 2 nan 2300 100 255 nan -1 1 1 1 -1", "BAD_ID", "fax decoder: id %d outside 0..%d"),
    ("fax 1 1 2 nan 2300 100 255 nan -1 1 1 1 -1", "INACTIVE", "no audio client with id %d"),
    ("fax 2 1 2 nan 2300 100 255 nan -1 1 1 1 -1", "IQ", "fax decoder: client %d is a PSDR_IQ client, which has no audio rows"),
    ("fax 0 1 2 nan 2300 100 255 nan -1 1 1 1 -1", "BAD_MODE", "fax decoder: mode %d is neither PSDR_FAX_AUTO nor PSDR_FAX_FREE"),
    ("fax 0 1 1 nan 2300 100 255 nan -1 1 1 1 -1", "BAD_TONES", "fax decoder: black_hz %g and white_hz %g are not finite numbers inside [%g, %g] that lie %g to %g apart"),
    ("fax 0 1 1 299 2300 100 255 nan -1 1 1 1 -1", "BAD_TONES", None),
    ("fax 0 1 1 1500 3401 100 255 nan -1 1 1 1 -1", "BAD_TONES", None),
    ("fax 0 1 1 1500 1699 100 255 nan -1 1 1 1 -1", "BAD_TONES", None),
    ("fax 0 1 1 1500 3101 100 255 nan -1 1 1 1 -1", "BAD_TONES", None),
    ("fax 0 1 1 3100 1500 100 255 nan -1 1 1 1 -1", "BAD_LPM", "fax decoder: lpm %g is none of 60, 90, 120 and 240"),
    ("fax 0 1 1 3100 1500 nan 255 nan -1 1 1 1 -1", "BAD_LPM", None),
    ("fax 0 1 1 3100 1500 60 255 nan -1 1 1 1 -1", "BAD_WIDTH", "fax decoder: width %d outside [%d, %d]"),
    ("fax 0 1 1 3100 1500 60 2049 nan -1 1 1 1 -1", "BAD_WIDTH", None),
    ("fax 0 1 1 3100 1500 60 2048 nan -1 1 1 1 -1", "BAD_SLANT", "fax decoder: slant_ppm %g is not a finite number inside [%g, %g]"),
    ("fax 0 1 1 3100 1500 60 2048 2000.1 -1 1 1 1 -1", "BAD_SLANT", None),
    ("fax 0 1 1 3100 1500 60 2048 -2000 -1 1 1 1 -1", "BAD_PHASE_COL", "fax decoder: phase_col %d outside [0, width %d)"),
    ("fax 0 1 1 3100 1500 60 2048 -2000 2048 1 1 1 -1", "BAD_PHASE_COL", None),
    ("fax 0 1 1 3100 1500 60 2048 -2000 2047 1 1 1 -1", "BAD_RATIO", "fax decoder: tone_ratio %g is not a finite number inside (0, 1)"),
    ("fax 0 1 1 3100 1500 60 2048 -2000 2047 0 1 1 -1", "BAD_RATIO", None),
    ("fax 0 1 1 3100 1500 60 2048 -2000 2047 nan 1 1 -1", "BAD_RATIO", None),
    ("fax 0 1 1 3100 1500 60 2048 -2000 2047 0.5 1 1 -1", "BAD_START", "fax decoder: start_blocks %d outside [2, 64]"),
    ("fax 0 1 1 3100 1500 60 2048 -2000 2047 0.5 65 1 -1", "BAD_START", None),
    ("fax 0 1 1 3100 1500 60 2048 -2000 2047 0.5 64 1 -1", "BAD_PHASE_LINES", "fax decoder: phase_lines %d outside [2, 32]"),
    ("fax 0 1 1 3100 1500 60 2048 -2000 2047 0.5 64 33 -1", "BAD_PHASE_LINES", None),
    ("fax 0 1 1 3100 1500 60 2048 -2000 2047 0.5 64 32 -1", "BAD_MAX_LINES", "fax decoder: max_lines %d is negative"),
    ("fax 0 1 1 3100 1500 60 2048 -2000 2047 0.5 64 32 0", "BAD_RATE", "fax decoder: the context's audio_rate %d is outside [%d, %d]"),
]
BAND = "fax decoder: the higher tone %g Hz plus %g does not lie under %g of the audio_rate %d"
PIXEL = "fax decoder: at lpm %g and audio_rate %d a pixel of width %d would not hold 1 to %d samples"


def test_every_refusal_in_order_with_a_text_of_its_own(exe):
    script = "case v\nrate 3999\nadd 0\nadd 2\nkind 2 4 0 0\n" + "".join(v[0] + "\n" for v in VERDICTS)
    last = VERDICTS[-1][0]
    script += ("fax 2 0 0 0 0 0 0 0 0 0 0 0 0\nfax 1 0 0 0 0 0 0 0 0 0 0 0 0\nrate 48001\n" + last + "\nrate 4000\n" + last + "\n"  # 3100 + 300 > 1800: the band, before the pixel
               "rate 5778\nfax 0 1 0 " + OK_TAIL + "\nrate 5777\nfax 0 1 0 " + OK_TAIL + "\n"  # 2300 + 300 Hz = 0.45 x 5777.8
               # 1 to 64 samples per pixel: 48000 Hz at 60 lpm is 48000 samples a line, 750 pixels of 64; 8000 Hz at 240 lpm is 2000 samples
               "rate 48000\nfax 0 1 0 1500 2300 60 750 0 0 0.22 8 4 0\nfax 0 1 0 1500 2300 60 749 0 0 0.22 8 4 0\nfax 0 1 0 1500 2300 60 750 0.1 0 0.22 8 4 0\n"
               "rate 8000\nfax 0 1 0 900 1700 240 2000 0 0 0.22 8 4 0\nfax 0 1 0 900 1700 240 2001 0 0 0.22 8 4 0\nfax 0 1 0 900 1700 240 2000 -0.1 0 0.22 8 4 0\n"
               "rate 12000\nfax 0 1 1 1500 2300 120 1024 100 512 0.22 8 4 7\ndump\n")
    out = M.run_script(exe, script).splitlines()
    got = [ln.split("verdict=")[1] for ln in out if ln.startswith("set ")]
    assert got == [v[1] for v in VERDICTS] + ["OK", "INACTIVE", "BAD_RATE", "BAD_BAND", "OK", "BAD_BAND", "OK", "BAD_PIXEL", "BAD_PIXEL", "OK", "BAD_PIXEL", "BAD_PIXEL", "OK"]
    slot0 = [ln for ln in out if ln.startswith("fxs slot=0 ")][0]
    d = dict(kv.split("=", 1) for kv in slot0.split()[1:])
    Lq = M.lq_of(120.0, 100.0, 12000)
    assert (d["on"], d["fresh"], d["mode"], d["width"]) == ("1", "1", "1", "1024") and int(d["Lq"]) == Lq == round(65536 * 6000 * 1.0001)
    assert (int(d["K"]), int(d["D"]), int(d["NB"]), int(d["wp"])) == (M.k_of(1900.0, 12000), M.d_of(12000), M.nb_of(12000), 51) == (3, 3, 94, 51)
    assert int(d["origin0"]) == 512 * Lq // 1024 and int(d["R"]) == M.ring_of(Lq, 900) == 64 and int(d["inc"]) == M.increment(1900.0, 12000) and int(d["tinc0"]) == M.increment(300.0, 12000)
    assert M.ring_of(M.lq_of(240.0, 0.0, 12000), 100 * 3000) == 2 + 100 + 1 and M.k_of(400.0, 48000) == 60 and M.d_of(48000) == 15 and M.d_of(4000) == 1 and M.k_of(3000.0, 4000) == 2
    src = open(os.path.join(ROOT, "phantomsdr_amd", "csrc", "demod.hip")).read()
    texts = {v[1]: v[2] for v in VERDICTS if v[2]}
    texts.update(BAD_BAND=BAND, BAD_PIXEL=PIXEL)
    assert len(set(texts.values())) == len(texts) == 16
    state = ("BAD_RATE", "BAD_BAND", "BAD_PIXEL")
    for verdict, text in texts.items():
        m = re.search(r"case FAX_%s: return fail\((PSDR_ERR_\w+), \"([^\"]*)\"" % verdict, src)
        assert m and m.group(2) == text and m.group(1) == ("PSDR_ERR_STATE" if verdict in state else "PSDR_ERR_INVALID"), verdict
    order = [src.index("case FAX_%s:" % v) for v in texts]
    assert order == sorted(order)


def test_defaults(exe):
    rates = (4000, 7999, 8000, 16000, 48000)
    out = M.run_script(exe, "".join(f"defaults {r}\n" for r in rates) + "defaults 3999.9\ndefaults 48000.1\ndefaults nan\n").splitlines()
    for line, rate in zip(out, rates):
        assert line == (f"defaults rate={rate} ok=1 mode=0 black_hz=1500 white_hz=2300 lpm=120 width=1024 slant_ppm=0 phase_col=0 tone_ratio={M.TONE_RATIO_DEFAULT!r} "
                        "start_blocks=8 phase_lines=4 max_lines=0"), line
    assert all(" ok=0 " in ln for ln in out[5:8])
    assert [M.hop_of(r) for r in rates] == [8, 8, 16, 32, 64] and [M.nb_of(r) for r in rates] == [63, 125, 63, 63, 94]


def test_plan_lists_and_zeroes(exe):
    """fax_plan behind demod_plan: who is listed and whose state starts from zero"""
    on = "0 " + OK_TAIL
    script = ("case plan\nadd 0\nadd 1\nadd 2\nadd 3\nwindow 0 100 100.3 200\nwindow 1 100 100.3 200\nwindow 2 100 100.3 200\nwindow 3 100 100.3 200\n"
              "batch\n"                                      # no fax client yet: nothing
              f"fax 1 1 {on}\nfax 3 1 1 1500 2300 240 256 0 0 0.3 4 3 0\nbatch\n"   # both from zero
              "batch\n"                                      # carried
              f"fax 1 1 {on}\nbatch\n"                       # again on: from zero
              "window 3 101 101.3 201\nkind 1 1 0 0\npause 0\nbatch\n"   # a retune and a mode change start over
              "kind 3 4 0 0\nbatch\n"                        # an IQ client keeps its setting and is not listed
              "kind 3 0 0 0\nfax 1 0 " + on + "\nbatch\ndump\n")
    lines = M.run_script(exe, script).splitlines()
    p = [dict(kv.split("=", 1) for kv in ln.split()[1:]) for ln in lines if ln.startswith("fxp")]
    assert p[0]["have"] == "0" and p[0]["any"] == "0"
    assert (p[1]["n"], p[1]["zero"]) == ("2", "1,3") and (p[2]["n"], p[2]["zero"]) == ("2", "") and (p[3]["n"], p[3]["zero"]) == ("2", "1")
    assert p[1]["list"].split(",")[1].split(":") == ["3", "1", "256", str(M.lq_of(240.0, 0.0, 12000)), str(M.increment(1900.0, 12000))]
    assert (p[4]["n"], p[4]["zero"]) == ("2", "1,3")
    assert (p[5]["n"], p[5]["zero"]) == ("1", "") and p[5]["list"].startswith("1:")
    assert (p[6]["n"], p[6]["zero"]) == ("1", "") and p[6]["list"].startswith("3:")  # back from IQ: the state stood still, as a paused one
    s = [dict(kv.split("=", 1) for kv in ln.split()[1:]) for ln in lines if ln.startswith("fxs")]
    assert [d["on"] for d in s[:4]] == ["0", "0", "0", "1"] and [d["b_on"] for d in s[:4]] == ["0", "0", "0", "1"]


def test_header_and_python_mirror():
    import ctypes

    import phantomsdr_amd as P
    from phantomsdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "psdr.h")).read()
    assert "#define PSDR_ABI_VERSION 3" in hdr and "#define PSDR_FAX_AUTO 0" in hdr and "#define PSDR_FAX_FREE 1" in hdr  # additions only
    assert f"#define PSDR_FAX_TONE_RATIO_DEFAULT {M.TONE_RATIO_DEFAULT!r}" in hdr
    names = [s[0] for s in _lib.SYMBOLS]
    syms = ("psdr_client_set_fax_decoder", "psdr_fax_defaults", "psdr_read_fax", "psdr_read_fax_lines")
    for sym in syms:
        assert sym in names and re.search(r"\bint %s\(" % sym, hdr), sym
    assert ctypes.sizeof(_lib.psdr_fax_config) == 80
    for attr in ("set_fax_decoder", "read_fax", "read_fax_lines"):
        assert hasattr(P.AudioClient, attr), attr
    assert callable(P.fax_defaults) and (P.FAX_AUTO, P.FAX_FREE) == (0, 1) and "fax" in __import__("phantomsdr_amd.build", fromlist=["UNITS"]).UNITS
    for words in ("applying offset_hz (AFC)", "automatic slant correction", "colour fax and SSTV", "Nobody has tried it on off-air radiofax", "psdr_fetch_*"):
        assert words in hdr, words
    lib = os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so")
    if os.path.exists(lib):  # the four symbols in the built library
        dll = ctypes.CDLL(lib)
        for sym in syms:
            assert hasattr(dll, sym), sym

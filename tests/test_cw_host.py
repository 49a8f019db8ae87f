"""The CW decoder's host side (phantomsdr_amd/csrc/cwplan.h; include/psdr.h: psdr_client_set_cw_decoder), without a device:
tests/cw_plan_table.cpp runs the text k_audio_cw runs, tests/cw_model.py restates the rule in numpy.  The sent text is the
yardstick of the truth tests, not the code."""
import os
import re

import numpy as np
import pytest

import cw_model as M
from conftest import ROOT

RATES = (4000, 8000, 12000, 16000, 48000)
TEXT = "PARIS CQ DE K1ABC 599 = ? /"
# the lowest signal-to-noise ratio, in the 2 H window's bandwidth (rate / 2 H: SNR = a^2 H / (2 sigma^2)) and in 3 dB steps, at which
# decode64() still reads TEXT at 20 WPM exactly with the seed below: measured 24 dB (21 dB gives `5OI*` for `599`); DESIGN 3.21
LOWEST_SNR_DB = 24.0
NOISE_SEED = 20261021


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("cw_host")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


@pytest.fixture(scope="module")
def builds(tmp, exe):
    """the table program as built by default, with contraction on and with contraction off"""
    return [exe, M.build_table(tmp, ROOT, ("-mfma", "-ffp-contract=fast"), "cw_fast"), M.build_table(tmp, ROOT, ("-ffp-contract=off",), "cw_off")]


def sent(text, wpm, rate, h=180, pitch=700.0, snr_db=None, seed=NOISE_SEED):
    """(rows f32 [F * h], flags [F]) of `text` keyed at `wpm`: 1.2 s of silence (not a whole number of hops), the keying, 3.5 dots
    behind it - the last character's space and no word space"""
    x = M.keyed_sine(text, wpm, rate, pitch=pitch, tail=3.5 * 1.2 / wpm)
    if snr_db is not None:
        x = x + 0.5 * np.sqrt(M.hop_of(rate) / (2 * 10 ** (snr_db / 10))) * np.random.default_rng(seed).standard_normal(len(x))
    F = -(-len(x) // h)
    x = np.concatenate([x, np.zeros(F * h - len(x))])
    return x.astype(np.float32), np.zeros(F, np.int32)


def decode(exe, tmp, jobs, rate):
    return M.run_streams(exe, tmp, jobs, rate=rate)


# ---- 1. bit parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_contraction_on_and_off_give_the_models_bits(tmp, builds, rate):
    rng = np.random.default_rng(rate)
    jobs, flags_of = [], {}
    for h in (180, 256):
        x, flags = sent("CQ K", 25, rate, h)
        x = (x + 0.01 * rng.standard_normal(len(x))).astype(np.float32)
        flags[len(flags) // 2] = 1  # a flagged frame enters as zeros
        jobs.append((dict(wpm=25.0), x, flags, h, [len(flags)]))
    outs = [decode(e, tmp, jobs, rate) for e in builds]
    for j, (cfg, x, flags, h, _) in enumerate(jobs):
        rec, text = M.records(x.reshape(len(flags), h), flags, h, rate, **cfg)
        for o in outs:
            assert o[j][0].tobytes() == rec.tobytes() and o[j][2] == text and o[j][1][-1].tobytes() == outs[0][j][1][-1].tobytes(), (rate, h)
        assert text == "CQ K" and rec["key"].any()


# ---- 2. truth -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_the_sent_text_is_read_at_12_20_and_30_wpm(tmp, exe, rate):
    speeds = (12, 20, 30)
    jobs = []
    for wpm in speeds:
        x, flags = sent(TEXT, wpm, rate)
        jobs.append((dict(wpm=float(wpm)), x, flags, 180, [len(flags)]))
    for wpm, (rec, _, text) in zip(speeds, decode(exe, tmp, jobs, rate)):
        second = int(np.argmax(rec["nchars"] >= len("PARIS ")))  # from the second word on
        err = np.abs(rec["wpm"][second:] / wpm - 1).max()
        print(f"rate {rate} {wpm} WPM: {text!r}, wpm off by at most {100 * err:.1f} % from frame {second} on")
        assert text == TEXT
        assert second > 0 and err <= 0.10
        assert (rec["pitch_hz"] == 700.0).all() and abs(rec["level"].max() / 0.25 - 1) < 0.05  # amplitude 0.5, squared


# ---- 3. speed tracking --------------------------------------------------------------------------------------------------------
def test_the_dot_length_follows_the_sender_from_20_wpm(tmp, exe):
    rate = 12000
    jobs = []
    for wpm, track in ((12, 1), (26, 1), (26, 0)):
        x, flags = sent(TEXT, wpm, rate)
        jobs.append((dict(track_speed=track), x, flags, 180, [len(flags)]))
    (r12, _, t12), (r26, _, t26), (rfix, _, tfix) = decode(exe, tmp, jobs, rate)
    assert t12 == TEXT and t26 == TEXT and tfix == TEXT
    assert abs(r12["wpm"][-1] / 12 - 1) < 0.1 and abs(r26["wpm"][-1] / 26 - 1) < 0.1
    moving = rfix["wpm"][rfix["wpm"] != 0]
    assert len(moving) and (moving == M.wpm_of(M.u_of(20.0, rate), rate)).all()  # u never moves


# ---- 4. pitch -----------------------------------------------------------------------------------------------------------------
def test_the_follower_finds_a_signal_inside_the_search_width_alone(tmp, exe):
    rate = 12000
    x, flags = sent(TEXT, 20, rate, pitch=580.0)
    (found, _, text), (fixed, _, _) = decode(exe, tmp, [(dict(search_hz=200.0), x, flags, 180, [len(flags)]),
                                                        (dict(search_hz=0.0), x, flags, 180, [len(flags)])], rate)
    assert text == TEXT and found["pitch_hz"][0] == 700.0 and found["pitch_hz"][-1] in (575.0, 600.0)
    assert (fixed["pitch_hz"] == 700.0).all()


# ---- 5. noise -----------------------------------------------------------------------------------------------------------------
def test_text_in_noise_6_db_above_the_lowest_ratio_that_float64_reads(tmp, exe):
    rate = 12000
    at, below = (M.decode64(sent(TEXT, 20, rate, snr_db=s)[0].astype(np.float64), rate)[1] for s in (LOWEST_SNR_DB, LOWEST_SNR_DB - 3))
    print(f"float64: {LOWEST_SNR_DB} dB {at!r}, {LOWEST_SNR_DB - 3} dB {below!r}")
    assert at == TEXT and below != TEXT  # the measurement, again
    x, flags = sent(TEXT, 20, rate, snr_db=LOWEST_SNR_DB + 6)
    (_, _, text), = decode(exe, tmp, [(dict(), x, flags, 180, [len(flags)])], rate)
    assert text == TEXT


def test_noise_alone_gives_no_character(tmp, exe):
    rate, h = 12000, 180
    F = 20 * rate // h
    x = (0.1 * np.random.default_rng(NOISE_SEED + 1).standard_normal(F * h)).astype(np.float32)
    (rec, _, text), = decode(exe, tmp, [(dict(), x, np.zeros(F, np.int32), h, [F])], rate)
    assert text == "" and rec["nchars"][-1] == 0


def test_silence_keys_nothing(tmp, exe):
    (rec, _, text), = decode(exe, tmp, [(dict(), np.zeros(400 * 180, np.float32), np.zeros(400, np.int32), 180, [400])], 12000)
    assert text == "" and not rec["key"].any() and not rec["level"].any()


# ---- 6. splits ----------------------------------------------------------------------------------------------------------------
def test_any_split_gives_the_same_records_text_and_state(tmp, exe):
    rate, h = 12000, 180
    x, flags = sent("CQ DE K", 25, rate, h, snr_db=36.0)
    flags[150] = 1
    F = len(flags)
    splits = ([F], [1] * F, [5, 6] * (F // 11) + ([F % 11] if F % 11 else []))
    outs = decode(exe, tmp, [(dict(wpm=25.0), x, flags, h, fr) for fr in splits], rate)
    for rec, st, text in outs:
        assert rec.tobytes() == outs[0][0].tobytes() and text == outs[0][2] == "CQ DE K" and st[-1].tobytes() == outs[0][1][-1].tobytes()
    last = outs[0][1][-1]
    assert last["pos"] == F * h and np.array_equal(last["part"][:F * h % 64], x[F * h - F * h % 64:]) and not last["part"][F * h % 64:].any()


# ---- 7. validation, defaults, table -------------------------------------------------------------------------------------------
VERDICTS = [  # in the order they are looked for: each call holds every later fault too
    ("cw 9 1 nan -1 9 2 5", "BAD_ID", "CW decoder: id %d outside 0..%d"),
    ("cw 1 1 nan -1 9 2 5", "INACTIVE", "no audio client with id %d"),
    ("cw 2 1 nan -1 9 2 5", "IQ", "CW decoder: client %d is a PSDR_IQ client, which has no audio rows"),
    ("cw 0 1 nan -1 9 2 5", "BAD_PITCH", "CW decoder: pitch_hz %g is not a finite number inside [%g, %g]"),
    ("cw 0 1 299.9 -1 9 2 5", "BAD_PITCH", None),
    ("cw 0 1 1800.1 -1 9 2 5", "BAD_PITCH", None),
    ("cw 0 1 300 -1 9 2 5", "BAD_SEARCH", "CW decoder: search_hz %g is not a finite number inside [%g, %g]"),
    ("cw 0 1 1800 800.1 9 2 5", "BAD_SEARCH", None),
    ("cw 0 1 700 0 9.9 2 5", "BAD_WPM", "CW decoder: wpm %g is not a finite number inside [%g, %g]"),
    ("cw 0 1 700 800 inf 2 5", "BAD_WPM", None),
    ("cw 0 1 700 100 10 2 5", "BAD_TRACK", "CW decoder: track_speed %d outside 0..1"),
    ("cw 0 1 700 100 40 -1 5", "BAD_TRACK", None),
    ("cw 0 1 700 100 40 0 5.9", "BAD_SNR", "CW decoder: snr_db %g is not a finite number inside [%g, %g]"),
    ("cw 0 1 700 100 40 1 40.1", "BAD_SNR", None),
    ("cw 0 1 700 100 40 1 nan", "BAD_SNR", None),
    ("cw 0 1 700 100 40 1 40", "BAD_RATE", "CW decoder: the context's audio_rate %d is outside [%d, %d]"),
]


def test_every_refusal_in_order_with_a_text_of_its_own(exe):
    script = "case v\nrate 3999\nadd 0\nadd 2\nkind 2 4 0 0\n" + "".join(v[0] + "\n" for v in VERDICTS)
    script += "cw 2 0 0 0 0 0 0\ncw 1 0 0 0 0 0 0\nrate 48001\n" + VERDICTS[-1][0] + "\nrate 48000\n" + VERDICTS[-1][0] + "\nrate 4000\n" + VERDICTS[-1][0] + "\ndump\n"
    out = M.run_script(exe, script).splitlines()
    got = [ln.split("verdict=")[1] for ln in out if ln.startswith("set ")]
    assert got == [v[1] for v in VERDICTS] + ["OK", "INACTIVE", "BAD_RATE", "OK", "OK"]  # (off: an IQ client may; the rate's ends are inside)
    slot0 = [ln for ln in out if ln.startswith("cws slot=0 ")][0]
    assert " on=1 fresh=1 " in slot0 and " p0=18 " in slot0 and " track=1 " in slot0  # a refusal changed nothing, the last call is in
    src = open(os.path.join(ROOT, "phantomsdr_amd", "csrc", "demod.hip")).read()
    texts = [v[2] for v in VERDICTS if v[2]]
    assert len(set(texts)) == len(texts) == 9
    for verdict, text in {v[1]: v[2] for v in VERDICTS if v[2]}.items():
        m = re.search(r"case CW_%s: return fail\((PSDR_ERR_\w+), \"([^\"]*)\"" % verdict, src)
        assert m and m.group(2) == text and m.group(1) == ("PSDR_ERR_STATE" if verdict == "BAD_RATE" else "PSDR_ERR_INVALID"), verdict


def test_defaults_and_tables(exe):
    out = M.run_script(exe, "defaults 4000\ndefaults 48000\ndefaults 3999.9\ndefaults 48000.1\ndefaults nan\n" + "".join(f"tables {r}\n" for r in RATES)).splitlines()
    for line, rate in zip(out, (4000, 48000)):
        assert line == f"defaults rate={rate} ok=1 pitch_hz=700 search_hz=100 wpm=20 track_speed=1 snr_db=22", line
    assert all(" ok=0 " in ln for ln in out[2:5])
    for line, rate in zip(out[5:], RATES):
        d = dict(kv.split("=", 1) for kv in line.split()[1:])
        H = M.hop_of(rate)
        assert int(d["H"]) == H and 0.004 <= H / rate <= 0.008
        assert (int(d["umin"]), int(d["umax"]), int(d["u20"])) == (M.u_of(40.0, rate), M.u_of(10.0, rate), M.u_of(20.0, rate))
        assert int(d["lscale"]) == int(np.float32(1.0 / (H * H)).view(np.uint32)) and int(d["wpm20"]) == int(M.wpm_of(M.u_of(20.0, rate), rate).view(np.uint32))
        assert [int(v) for v in d["inc"].split(",")] == M.increments(rate).tolist()
        morse = bytes.fromhex(d["morse"])
        assert {c: chr(b) for c, b in enumerate(morse) if b != ord("*")} == M.BY_CODE and len(M.BY_CODE) == 49
    assert M.lane_hz(63) == 1825.0 < 4000 / 2
    # the hop length's class boundaries, on both sides
    edges = {15999: 64, 16000: 128, 31999: 128, 32000: 256}
    out = M.run_script(exe, "".join(f"tables {r}\n" for r in edges)).splitlines()
    assert len(out) == len(edges)
    for line, (rate, H) in zip(out, edges.items()):
        d = dict(kv.split("=", 1) for kv in line.split()[1:])
        assert float(d["rate"]) == rate and int(d["H"]) == H == M.hop_of(rate), line
    assert M.hop_of(15999) == 64 and M.hop_of(16000) == 128 and M.hop_of(31999) == 128 and M.hop_of(32000) == 256


def test_every_listed_character_round_trips_through_a_synthetic_keying(exe):
    """dits of 11 hops at 12 kHz and 20 WPM (u = 180: 11.25 hops), standard gaps; too long and unknown codes give `*`"""
    def raw(chars, dot=11):
        s = "0" * 40
        for ch in chars:
            key = M.MORSE.get(ch, ch)
            s += ("0" * dot).join("1" * (dot * (3 if el == "-" else 1)) for el in key) + "0" * (3 * dot)
        return s + "0" * (4 * dot)

    chars = list(M.MORSE)
    script = "".join(f"keying 12000 20 1 {raw([ch])}\n" for ch in chars)
    script += f"keying 12000 20 1 {raw(['........', '......', 'E'])}\n" + f"keying 12000 20 0 {raw(chars)}\n"
    out = M.run_script(exe, script).splitlines()
    for ch, line in zip(chars, out):
        assert line.endswith(f"text=[{ch} ]"), (ch, line)
    assert out[len(chars)].endswith("text=[**E ]"), out[len(chars)]  # (character gaps between them, a word gap behind)
    assert out[-1].endswith("text=[%s ]" % "".join(chars)) and out[-1].startswith("keying u=180 ")


def test_plan_lists_and_zeroes(exe):
    """cw_plan behind demod_plan: who is listed and whose state starts from zero"""
    script = ("case plan\nadd 0\nadd 1\nadd 2\nadd 3\nwindow 0 100 100.3 200\nwindow 1 100 100.3 200\nwindow 2 100 100.3 200\nwindow 3 100 100.3 200\n"
              "batch\n"                                      # no CW client yet: nothing
              "cw 1 1 700 100 20 1 22\ncw 3 1 580 200 25 0 22\nbatch\n"   # both from zero
              "batch\n"                                      # carried
              "cw 1 1 700 100 20 1 22\nbatch\n"              # again on: from zero
              "window 3 101 101.3 201\nkind 1 1 0 0\npause 0\nbatch\n"   # a retune and a mode change start over
              "kind 3 4 0 0\nbatch\n"                        # an IQ client keeps its setting and is not listed
              "kind 3 0 0 0\ncw 1 0 0 0 0 0 0\nbatch\ndump\n")
    lines = M.run_script(exe, script).splitlines()
    p = [dict(kv.split("=", 1) for kv in ln.split()[1:]) for ln in lines if ln.startswith("cwp")]
    assert p[0]["have"] == "0" and p[0]["any"] == "0"
    assert (p[1]["n"], p[1]["zero"]) == ("2", "1,3") and (p[2]["n"], p[2]["zero"]) == ("2", "") and (p[3]["n"], p[3]["zero"]) == ("2", "1")
    e = p[1]["list"].split(",")[1].split(":")
    assert e[:4] == ["3", str(M.nearest(580.0)), str(M.u_of(25.0, 12000)), "0"]
    assert int(e[5], 16) == sum(1 << k for k in np.flatnonzero(M.candidates(580.0, 200.0)))
    assert (p[4]["n"], p[4]["zero"]) == ("2", "1,3")
    assert (p[5]["n"], p[5]["zero"]) == ("1", "") and p[5]["list"].startswith("1:")
    assert (p[6]["n"], p[6]["zero"]) == ("1", "") and p[6]["list"].startswith("3:")  # back from IQ: the state stood still, as a paused one
    s = [dict(kv.split("=", 1) for kv in ln.split()[1:]) for ln in lines if ln.startswith("cws")]
    assert [d["on"] for d in s[:4]] == ["0", "0", "0", "1"] and [d["b_on"] for d in s[:4]] == ["0", "0", "0", "1"]


def test_header_and_python_mirror():
    import ctypes

    import phantomsdr_amd as P
    from phantomsdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "psdr.h")).read()
    assert "#define PSDR_ABI_VERSION 3" in hdr and "#define PSDR_CW_LANES 64" in hdr  # additions only
    names = [s[0] for s in _lib.SYMBOLS]
    for sym in ("psdr_client_set_cw_decoder", "psdr_cw_defaults", "psdr_read_cw", "psdr_read_cw_text"):
        assert sym in names and re.search(r"\bint %s\(" % sym, hdr), sym
    assert ctypes.sizeof(_lib.psdr_cw_config) == 40
    for attr in ("set_cw_decoder", "read_cw", "read_cw_text"):
        assert hasattr(P.AudioClient, attr), attr
    assert callable(P.cw_defaults) and "cw" in __import__("phantomsdr_amd.build", fromlist=["UNITS"]).UNITS
    assert "Nobody has tried it on off-air CW" in hdr and "no psdr_group_* call: a group's clients have no CW decoder" in hdr

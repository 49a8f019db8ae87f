"""The RTTY decoder's host side (phantomsdr_amd/csrc/rttyplan.h; include/psdr.h: psdr_client_set_rtty_decoder), without a device:
tests/rtty_plan_table.cpp runs the text k_audio_rtty runs, tests/rtty_model.py restates the rule in numpy and holds the sender.
The sent text is the yardstick of the truth tests, not the code."""
import os
import re

import numpy as np
import pytest

import rtty_model as M
from conftest import ROOT

RATES = (4000, 8000, 12000, 16000, 48000)
TEXT = "RYRYRY CQ DE K1ABC 599 K\r\n"
NOISE_SEED = 20261021
# Measured with the host program, all at 12 kHz and 45.45 baud with NOISE_SEED:
#   the largest `quality` of 60 s of noise alone, over every rate of RATES at 45 and 75 baud: 6.4 dB (NOISE_QUALITY_DB bounds it);
#   the lowest signal-to-noise ratio, in the bit window's bandwidth (baud: SNR = a^2 / (2 sigma^2) * rate / (2 baud)) and in 3 dB
#   steps, at which TEXT is still read exactly with errors == 0: LOWEST_SNR_DB; 3 dB below it the text is not read;
#   the smallest `quality` while that text is read: LOWEST_QUALITY_DB;
#   the default snr_db, half-way between the two in dB: M.SNR_DEFAULT.
NOISE_QUALITY_DB = 6.5
LOWEST_SNR_DB = 15.0
LOWEST_QUALITY_DB = 8.5
AMP = 0.5


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("rtty_host")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


@pytest.fixture(scope="module")
def builds(tmp, exe):
    """the table program as built by default, with contraction on and with contraction off"""
    return [exe, M.build_table(tmp, ROOT, ("-mfma", "-ffp-contract=fast"), "rtty_fast"), M.build_table(tmp, ROOT, ("-ffp-contract=off",), "rtty_off")]


def framed(x, h=180):
    F = -(-len(x) // h)
    return np.concatenate([x, np.zeros(F * h - len(x))]).astype(np.float32), np.zeros(F, np.int32)


def sent(text, baud, rate, h=180, snr_db=None, seed=NOISE_SEED, **kw):
    """(rows f32 [F * h], flags [F]) of `text` at `baud`: 0.8 s of mark, the characters, 0.3 s of mark; kw: M.fsk's"""
    kw.setdefault("mark", M.default_mark(rate))
    x = M.fsk(text, baud, rate, amp=AMP, **kw)
    if snr_db is not None:  # sigma from the ratio in the bit window's bandwidth
        x = x + AMP * np.sqrt(rate / (4 * baud * 10 ** (snr_db / 10))) * np.random.default_rng(seed).standard_normal(len(x))
    return framed(x, h)


def decode(exe, tmp, jobs, rate):
    return M.run_streams(exe, tmp, jobs, rate=rate)


def db(v):
    return 10 * np.log10(max(float(v), 1e-30))


# ---- 1. bit parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_contraction_on_and_off_give_the_models_bits(tmp, builds, rate):
    rng = np.random.default_rng(rate)
    jobs = []
    for h in (180, 256):
        x, flags = sent("RY 5", 50.0, rate, h, lead=0.6, tail=0.1)
        x = (x + 0.01 * rng.standard_normal(len(x))).astype(np.float32)
        flags[2] = 1  # a flagged frame enters as zeros: here while the presence fills (inside a transmission it costs the characters up to the next idle)
        F = len(flags)
        for frames in ([F], [1] * F, [5, 6] * (F // 11) + ([F % 11] if F % 11 else [])):
            jobs.append((dict(baud=50.0), x, flags, h, frames))
    outs = [decode(e, tmp, jobs, rate) for e in builds]
    for j, (cfg, x, flags, h, _) in enumerate(jobs):
        rec, text = M.records(x.reshape(len(flags), h), flags, h, rate, **cfg)
        for o in outs:
            assert o[j][0].tobytes() == rec.tobytes() and o[j][2] == text and o[j][1][-1].tobytes() == outs[0][j - j % 3][1][-1].tobytes(), (rate, h, j)
        assert text == "RY 5" and rec["present"].any() and rec["errors"][-1] == 0


# ---- 2. truth -----------------------------------------------------------------------------------------------------------------
def check_truth(rec, text, rate, h=180, lead=0.8):
    assert text == TEXT and rec["errors"][-1] == 0
    first = int(lead * rate / h)  # the frame the first character starts in
    assert rec["present"][first:].all()
    assert abs(rec["level"][first:].max() / AMP ** 2 - 1) < 0.05


@pytest.mark.parametrize("rate", RATES)
def test_the_sent_text_is_read_at_every_speed_shift_and_stop_length(tmp, exe, rate):
    rng = np.random.default_rng(rate)
    nidle = len(M.baudot(TEXT))
    cases = [dict(baud=b) for b in (45.45, 50.0, 75.0)]
    cases += [dict(baud=50.0, shift=s) for s in (425.0, 850.0, -170.0) if rate >= 8000 or abs(s) < 800]
    cases += [dict(baud=45.45, stop_bits=s) for s in (1.0, 2.0)]
    cases += [dict(baud=45.45, idle=rng.uniform(0.0, 0.1, nidle)), dict(baud=45.45, fast=1.02), dict(baud=45.45, fast=0.98), dict(baud=45.45, usos=0)]
    jobs = []
    for c in cases:
        c = dict(c)
        cfg = dict(baud=c.pop("baud"), usos=c.pop("usos", 1))
        mark = M.default_mark(rate) if c.get("shift", 170.0) > 0 else M.default_mark(rate) + 170.0
        if "shift" in c:
            cfg.update(shift_hz=c["shift"], mark_hz=mark)
        x, flags = sent(TEXT, cfg["baud"] * c.pop("fast", 1.0), rate, mark=mark, **c)
        jobs.append((cfg, x, flags, 180, [len(flags)]))
    for c, (rec, _, text) in zip(cases, decode(exe, tmp, jobs, rate)):
        print(f"rate {rate} {c}: {text!r} errors {rec['errors'][-1]} level {rec['level'].max():.4f} quality {db(rec['quality'][-1]):.1f} dB")
        check_truth(rec, text, rate)
        assert (rec["offset_hz"] == 0).all()


# ---- 3. follower --------------------------------------------------------------------------------------------------------------
def test_the_follower_finds_a_signal_50_hz_off_inside_the_search_width_alone(tmp, exe):
    rate = 12000
    x, flags = sent(TEXT, 45.45, rate, mark=2175.0)
    (found, _, text), (fixed, _, _) = decode(exe, tmp, [(dict(), x, flags, 180, [len(flags)]), (dict(search_hz=0.0), x, flags, 180, [len(flags)])], rate)
    assert text == TEXT and found["errors"][-1] == 0 and abs(found["offset_hz"][-1] - 50.0) <= M.DF
    assert (fixed["offset_hz"] == 0).all()


# ---- 4. fading ----------------------------------------------------------------------------------------------------------------
def test_a_space_tone_at_a_quarter_of_the_marks_amplitude_is_read(tmp, exe):
    rate = 12000
    x, flags = sent(TEXT, 45.45, rate, amp_space=AMP / 4)
    (rec, _, text), = decode(exe, tmp, [(dict(), x, flags, 180, [len(flags)])], rate)
    assert text == TEXT and rec["errors"][-1] == 0


# ---- 5. presence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,baud", [(4000, 45.0), (12000, 45.45), (12000, 75.0), (48000, 45.0)])
def test_noise_alone_prints_nothing(tmp, exe, rate, baud):
    h = 180
    F = 60 * rate // h
    x = (0.1 * np.random.default_rng(NOISE_SEED).standard_normal(F * h)).astype(np.float32)
    (rec, _, text), = decode(exe, tmp, [(dict(baud=baud), x, np.zeros(F, np.int32), h, [F])], rate)
    q = db(rec["quality"][M.FILL * M.hop_of(rate) // h + 1:].max())
    print(f"rate {rate} baud {baud}: 60 s of noise alone, the largest quality {q:.2f} dB")
    assert text == "" and rec["nchars"][-1] == 0 and rec["errors"][-1] == 0 and not rec["present"].any()
    assert q <= NOISE_QUALITY_DB < M.SNR_DEFAULT


def test_text_in_noise_at_the_lowest_ratio_that_is_read(tmp, exe):
    rate = 12000
    jobs = [(dict(), *sent(TEXT, 45.45, rate, snr_db=s), 180, None) for s in (LOWEST_SNR_DB, LOWEST_SNR_DB - 3)]
    jobs = [(c, x, f, h, [len(f)]) for c, x, f, h, _ in jobs]
    (at, _, tat), (below, _, tbelow) = decode(exe, tmp, jobs, rate)
    first = int(0.8 * rate / 180)
    qmin = db(at["quality"][first:].min())
    print(f"{LOWEST_SNR_DB} dB: {tat!r} errors {at['errors'][-1]} smallest quality {qmin:.2f} dB; {LOWEST_SNR_DB - 3} dB: {tbelow!r} errors {below['errors'][-1]}")
    assert tat == TEXT and at["errors"][-1] == 0 and at["present"][first:].all()
    assert tbelow != TEXT  # the measurement, again: 3 dB below the text is not read
    assert qmin >= LOWEST_QUALITY_DB and abs(M.SNR_DEFAULT - (NOISE_QUALITY_DB + LOWEST_QUALITY_DB) / 2) <= 0.051


def test_silence_prints_nothing(tmp, exe):
    (rec, _, text), = decode(exe, tmp, [(dict(), np.zeros(400 * 180, np.float32), np.zeros(400, np.int32), 180, [400])], 12000)
    assert text == "" and not rec["present"].any() and not rec["level"].any() and not rec["quality"].any()


# ---- 6. validation, defaults, table, plan -------------------------------------------------------------------------------------
VERDICTS = [  # in the order they are looked for: each call holds every later fault too
    ("rtty 9 1 nan 50 9 2 -1 1", "BAD_ID", "RTTY decoder: id %d outside 0..%d"),
    ("rtty 1 1 nan 50 9 2 -1 1", "INACTIVE", "no audio client with id %d"),
    ("rtty 2 1 nan 50 9 2 -1 1", "IQ", "RTTY decoder: client %d is a PSDR_IQ client, which has no audio rows"),
    ("rtty 0 1 nan 50 9 2 -1 1", "BAD_MARK", "RTTY decoder: mark_hz %g is not a finite number inside [%g, %g]"),
    ("rtty 0 1 299.9 50 9 2 -1 1", "BAD_MARK", None),
    ("rtty 0 1 3000.1 50 9 2 -1 1", "BAD_MARK", None),
    ("rtty 0 1 300 84.9 9 2 -1 1", "BAD_SHIFT", "RTTY decoder: shift_hz %g is not a finite number of magnitude inside [%g, %g]"),
    ("rtty 0 1 3000 -1000.1 9 2 -1 1", "BAD_SHIFT", None),
    ("rtty 0 1 3000 nan 9 2 -1 1", "BAD_SHIFT", None),
    ("rtty 0 1 1000 170 44.9 2 -1 1", "BAD_BAUD", "RTTY decoder: baud %g is not a finite number inside [%g, %g]"),
    ("rtty 0 1 1000 -170 75.1 2 -1 1", "BAD_BAUD", None),
    ("rtty 0 1 1000 170 45 2 -1 1", "BAD_USOS", "RTTY decoder: usos %d outside 0..1"),
    ("rtty 0 1 1000 170 75 -1 -1 1", "BAD_USOS", None),
    ("rtty 0 1 1000 170 75 0 -0.1 1", "BAD_SEARCH", "RTTY decoder: search_hz %g is not a finite number inside [%g, %g]"),
    ("rtty 0 1 1000 170 75 1 160.1 1", "BAD_SEARCH", None),
    ("rtty 0 1 1000 170 75 1 0 2.9", "BAD_SNR", "RTTY decoder: snr_db %g is not a finite number inside [%g, %g]"),
    ("rtty 0 1 1000 170 75 1 160 30.1", "BAD_SNR", None),
    ("rtty 0 1 1000 170 75 1 160 inf", "BAD_SNR", None),
    ("rtty 0 1 3000 1000 75 1 160 30", "BAD_RATE", "RTTY decoder: the context's audio_rate %d is outside [%d, %d]"),
]
BAND = "RTTY decoder: the tones %g and %g Hz with %g Hz to either side do not lie inside [%g Hz, %g of the audio_rate %d]"


def test_every_refusal_in_order_with_a_text_of_its_own(exe):
    script = "case v\nrate 3999\nadd 0\nadd 2\nkind 2 4 0 0\n" + "".join(v[0] + "\n" for v in VERDICTS)
    last = VERDICTS[-1][0]
    script += ("rtty 2 0 0 0 0 0 0 0\nrtty 1 0 0 0 0 0 0 0\nrate 48001\n" + last + "\nrate 48000\n" + last + "\nrate 4000\n" + last + "\n"  # 4160 Hz: over 0.45 x 4000
               "rtty 0 1 1640 0 45 1 0 3\nrtty 0 1 1470 170 45 1 0 3\nrtty 0 1 1471 170 45 1 0 3\nrtty 0 1 430 -170 45 1 0 3\nrtty 0 1 429 -170 45 1 0 3\n"
               "rtty 0 1 915 170 45.45 1 60 9\ndump\n")
    out = M.run_script(exe, script).splitlines()
    got = [ln.split("verdict=")[1] for ln in out if ln.startswith("set ")]
    assert got == [v[1] for v in VERDICTS] + ["OK", "INACTIVE", "BAD_RATE", "OK", "BAD_BAND", "BAD_SHIFT", "OK", "BAD_BAND", "OK", "BAD_BAND", "OK"]
    slot0 = [ln for ln in out if ln.startswith("rts slot=0 ")][0]
    assert " on=1 fresh=1 " in slot0 and f" wn={M.wn_of(45.45, 4000)} " in slot0 and f" u={M.u_of(45.45, 4000)} " in slot0 and " cand=0fe0 " in slot0
    inc = M.increments(4000, 915.0, 170.0)
    assert f" inc16={inc[16]} inc17={inc[17]}" in slot0
    src = open(os.path.join(ROOT, "phantomsdr_amd", "csrc", "demod.hip")).read()
    texts = [v[2] for v in VERDICTS if v[2]] + [BAND]
    assert len(set(texts)) == len(texts) == 11
    for verdict, text in list({v[1]: v[2] for v in VERDICTS if v[2]}.items()) + [("BAD_BAND", BAND)]:
        m = re.search(r"case RTTY_%s: return fail\((PSDR_ERR_\w+), \"([^\"]*)\"" % verdict, src)
        assert m and m.group(2) == text and m.group(1) == ("PSDR_ERR_STATE" if verdict in ("BAD_RATE", "BAD_BAND") else "PSDR_ERR_INVALID"), verdict
    order = [src.index("case RTTY_%s:" % v) for v in ("BAD_ID", "INACTIVE", "IQ", "BAD_MARK", "BAD_SHIFT", "BAD_BAUD", "BAD_USOS", "BAD_SEARCH", "BAD_SNR", "BAD_RATE", "BAD_BAND")]
    assert order == sorted(order)


def test_defaults_and_tables(exe):
    rates = (4000, 5455, 5456, 8000, 48000)
    out = M.run_script(exe, "".join(f"defaults {r}\n" for r in rates) + "defaults 3999.9\ndefaults 48000.1\ndefaults nan\n" + "".join(f"tables {r}\n" for r in RATES)).splitlines()
    for line, rate in zip(out, rates):
        assert line == f"defaults rate={rate} ok=1 mark_hz={M.default_mark(rate):g} shift_hz=170 baud=45.450000000000003 usos=1 search_hz=60 snr_db={M.SNR_DEFAULT!r}", line
    assert M.default_mark(5455) == 915.0 and M.default_mark(5456) == 2125.0
    assert all(" ok=0 " in ln for ln in out[5:8])
    for line, rate in zip(out[8:], RATES):
        d = dict(kv.split("=", 1) for kv in line.split()[1:])
        H = M.hop_of(rate)
        assert int(d["H"]) == H and 0.001 <= H / rate <= 0.002
        assert (int(d["wn45"]), int(d["wn75"]), int(d["u4545"])) == (M.wn_of(45.0, rate), M.wn_of(75.0, rate), M.u_of(45.45, rate))
        assert 7 <= int(d["wn75"]) <= int(d["wn45"]) <= M.WMAX - 2
        table = bytes.fromhex(d["baudot"])
        assert [chr(b) if b else "" for b in table[:32]] == M.LTRS and [chr(b) if b else "" for b in table[32:]] == M.FIGS
    # the sender's table and the decoder's are two: every character of the one is where the other has it
    for send, have in ((M.SEND_LTRS, M.LTRS), (M.SEND_FIGS, M.FIGS)):
        for ch, bits in list(send.items()) + list(M.SEND_BOTH.items()):
            assert have[int(bits[::-1], 2)] == ch, ch
    assert len(M.SEND_LTRS) == 26 and len(M.SEND_FIGS) == 26 and int(M.SEND_LTRS_SHIFT[::-1], 2) == M.CODE_LTRS and int(M.SEND_FIGS_SHIFT[::-1], 2) == M.CODE_FIGS
    assert M.wn_of(45.0, 7999) == 22 and M.hop_of(7999) == 8 and M.hop_of(8000) == 16 and M.hop_of(15999) == 16 and M.hop_of(16000) == 32 and M.hop_of(32000) == 64


def test_every_character_of_either_shift_is_read(tmp, exe):
    rate = 12000
    text = "THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG 1234567890 -$',!:(\")#?&./;\x07\r\n"
    x, flags = sent(text, 75.0, rate)
    (rec, _, got), (_, _, got0) = decode(exe, tmp, [(dict(baud=75.0), x, flags, 180, [len(flags)]), (dict(baud=75.0, usos=0), x, flags, 180, [len(flags)])], rate)
    assert got == text and got0 == text and rec["errors"][-1] == 0 and rec["nchars"][-1] == len(text)


def test_plan_lists_and_zeroes(exe):
    """rtty_plan behind demod_plan: who is listed and whose state starts from zero"""
    on = "2125 170 45.45 1 60 9"
    script = ("case plan\nadd 0\nadd 1\nadd 2\nadd 3\nwindow 0 100 100.3 200\nwindow 1 100 100.3 200\nwindow 2 100 100.3 200\nwindow 3 100 100.3 200\n"
              "batch\n"                                      # no RTTY client yet: nothing
              f"rtty 1 1 {on}\nrtty 3 1 2125 -850 75 0 0 9\nbatch\n"   # both from zero
              "batch\n"                                      # carried
              f"rtty 1 1 {on}\nbatch\n"                      # again on: from zero
              "window 3 101 101.3 201\nkind 1 1 0 0\npause 0\nbatch\n"   # a retune and a mode change start over
              "kind 3 4 0 0\nbatch\n"                        # an IQ client keeps its setting and is not listed
              "kind 3 0 0 0\nrtty 1 0 0 0 0 0 0 0\nbatch\ndump\n")
    lines = M.run_script(exe, script).splitlines()
    p = [dict(kv.split("=", 1) for kv in ln.split()[1:]) for ln in lines if ln.startswith("rtp")]
    assert p[0]["have"] == "0" and p[0]["any"] == "0"
    assert (p[1]["n"], p[1]["zero"]) == ("2", "1,3") and (p[2]["n"], p[2]["zero"]) == ("2", "") and (p[3]["n"], p[3]["zero"]) == ("2", "1")
    e = p[1]["list"].split(",")[1].split(":")
    assert e[:4] == ["3", str(M.wn_of(75.0, 12000)), str(M.u_of(75.0, 12000)), "0"] and e[5] == "0100" and int(e[6]) == M.increments(12000, 2125.0, -850.0)[16]
    assert (p[4]["n"], p[4]["zero"]) == ("2", "1,3")
    assert (p[5]["n"], p[5]["zero"]) == ("1", "") and p[5]["list"].startswith("1:")
    assert (p[6]["n"], p[6]["zero"]) == ("1", "") and p[6]["list"].startswith("3:")  # back from IQ: the state stood still, as a paused one
    s = [dict(kv.split("=", 1) for kv in ln.split()[1:]) for ln in lines if ln.startswith("rts")]
    assert [d["on"] for d in s[:4]] == ["0", "0", "0", "1"] and [d["b_on"] for d in s[:4]] == ["0", "0", "0", "1"]


def test_header_and_python_mirror():
    import ctypes

    import phantomsdr_amd as P
    from phantomsdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "psdr.h")).read()
    assert "#define PSDR_ABI_VERSION 3" in hdr and "#define PSDR_RTTY_LANES 32" in hdr  # additions only
    assert f"#define PSDR_RTTY_SNR_DEFAULT {M.SNR_DEFAULT!r}" in hdr
    names = [s[0] for s in _lib.SYMBOLS]
    for sym in ("psdr_client_set_rtty_decoder", "psdr_rtty_defaults", "psdr_read_rtty", "psdr_read_rtty_text"):
        assert sym in names and re.search(r"\bint %s\(" % sym, hdr), sym
    assert ctypes.sizeof(_lib.psdr_rtty_config) == 48
    for attr in ("set_rtty_decoder", "read_rtty", "read_rtty_text"):
        assert hasattr(P.AudioClient, attr), attr
    assert callable(P.rtty_defaults) and "rtty" in __import__("phantomsdr_amd.build", fromlist=["UNITS"]).UNITS
    assert "Nobody has tried it on off-air RTTY" in hdr and "no psdr_group_* call: a group's clients have no RTTY decoder" in hdr
    lib = os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so")
    if os.path.exists(lib):  # the four symbols in the built library
        dll = ctypes.CDLL(lib)
        for sym in ("psdr_client_set_rtty_decoder", "psdr_rtty_defaults", "psdr_read_rtty", "psdr_read_rtty_text"):
            assert hasattr(dll, sym), sym

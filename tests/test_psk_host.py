"""The PSK31 decoder's host side (phantomsdr_amd/csrc/pskplan.h; include/psdr.h: psdr_client_set_psk_decoder), without a device:
tests/psk_plan_table.cpp runs the text k_audio_psk runs, tests/psk_model.py restates the rule in numpy and holds the sender.
The sent text is the yardstick of the truth tests, not the code."""
import os
import re

import numpy as np
import pytest

import psk_model as M
from conftest import ROOT

RATES = (4000, 8000, 12000, 16000, 48000)
BAUDS = (31.25, 62.5)
TEXT = "CQ CQ de K1ABC K1ABC pse k\r\n"
NOISE_SEED = 20261021
# Measured with the host program with NOISE_SEED:
#   the largest coherence of 60 s of unit noise alone, over every rate of RATES at both speeds: 0.405 (NOISE_COHERENCE bounds it);
#   the lowest signal-to-noise ratio, in a bandwidth equal to the baud rate (SNR = a^2 / (2 sigma^2) * rate / (2 baud)) and in
#   3 dB steps, at which TEXT is still read exactly with errors == 0, at 12 kHz and 31.25 baud: LOWEST_SNR_DB; 3 dB below it the
#   text is not read;
#   the smallest coherence while that text is read: 0.616 (LOWEST_COHERENCE bounds it);
#   the default quality, half-way between the two: M.QUALITY_DEFAULT.
NOISE_COHERENCE = 0.41
LOWEST_SNR_DB = 12.0
LOWEST_COHERENCE = 0.61
AMP = 0.5
PREAMBLE = 64


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("psk_host")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


@pytest.fixture(scope="module")
def builds(tmp, exe):
    """the table program as built by default, with contraction on and with contraction off"""
    return [exe, M.build_table(tmp, ROOT, ("-mfma", "-ffp-contract=fast"), "psk_fast"), M.build_table(tmp, ROOT, ("-ffp-contract=off",), "psk_off")]


def framed(x, h=180):
    F = -(-len(x) // h)
    return np.concatenate([x, np.zeros(F * h - len(x))]).astype(np.float32), np.zeros(F, np.int32)


def sent(text, baud, rate, h=180, snr_db=None, seed=NOISE_SEED, carrier=1000.0, fast=1.0, preamble=PREAMBLE, lead=0.2):
    """(rows f32 [F * h], flags [F]) of `text` at `baud`: 0.2 s of nothing, the idle preamble, the characters, 32 symbols of carrier"""
    x = M.bpsk(M.varicode(text, preamble=preamble), baud * fast, rate, carrier=carrier, amp=AMP, lead=lead)
    if snr_db is not None:  # sigma from the ratio in a bandwidth equal to the baud rate
        x = x + AMP * np.sqrt(rate / (4 * baud * 10 ** (snr_db / 10))) * np.random.default_rng(seed).standard_normal(len(x))
    return framed(x, h)


def decode(exe, tmp, jobs, rate):
    return M.run_streams(exe, tmp, jobs, rate=rate)


def text_frames(text, baud, rate, h=180, lead=0.2):
    """the frames in which the characters are sent: behind the preamble, in front of the carrier"""
    n = len(M.varicode(text, preamble=PREAMBLE, postamble=0))
    return int((lead + PREAMBLE / baud) * rate / h), int((lead + n / baud) * rate / h)


# ---- 1. bit parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_contraction_on_and_off_give_the_models_bits(tmp, builds, rate):
    rng = np.random.default_rng(rate)
    jobs = []
    for h, baud in ((180, 62.5), (256, 31.25)):
        x, flags = sent("ab c", baud, rate, h, preamble=40, lead=0.1)
        x = (x + 0.01 * rng.standard_normal(len(x))).astype(np.float32)
        flags[2] = 1  # a flagged frame enters as zeros: here in front of the presence
        F = len(flags)
        for frames in ([F], [1] * F, [5, 6] * (F // 11) + ([F % 11] if F % 11 else [])):
            jobs.append((dict(baud=baud), x, flags, h, frames))
    outs = [decode(e, tmp, jobs, rate) for e in builds]
    for j, (cfg, x, flags, h, _) in enumerate(jobs):
        rec, text = M.records(x.reshape(len(flags), h), flags, h, rate, **cfg)
        for o in outs:
            assert o[j][0].tobytes() == rec.tobytes() and o[j][2] == text and o[j][1][-1].tobytes() == outs[0][j - j % 3][1][-1].tobytes(), (rate, h, j)
        assert text == "ab c" and rec["present"].any() and not rec["present"].all() and rec["errors"][-1] == 0


# ---- 2. truth -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_the_sent_text_is_read_at_both_speeds_off_tune_and_off_speed(tmp, exe, rate):
    cases = [dict(baud=b, off=o) for b in BAUDS for o in (0.0, 2.0, -2.0, 6.0, -6.0, 10.0, -10.0)]
    cases += [dict(baud=b, off=0.0, fast=f) for b in BAUDS for f in (1.001, 0.999)]
    jobs = []
    for c in cases:
        x, flags = sent(TEXT, c["baud"], rate, carrier=1000.0 + c["off"] * c["baud"] / 31.25, fast=c.get("fast", 1.0))
        jobs.append((dict(baud=c["baud"]), x, flags, 180, [len(flags)]))
    for c, (rec, _, text) in zip(cases, decode(exe, tmp, jobs, rate)):
        print(f"rate {rate} {c}: {text!r} errors {rec['errors'][-1]} offset {rec['offset_hz'][-1]} level {rec['level'].max():.4f} quality {rec['quality'][-1]:.3f}")
        assert text == TEXT and rec["errors"][-1] == 0
        first, last = text_frames(TEXT, c["baud"], rate)
        assert rec["present"][first:].all()
        # offsets are in Hz at 31.25 baud and twice that at 62.5: within one lane of the truth
        assert abs(rec["offset_hz"][-1] - c["off"] * c["baud"] / 31.25) <= c["baud"] / 8
        # the carrier behind the text reads its squared amplitude (the follower has had 32 symbols: within 1 - exp(-1) of it)
        assert 0.2 * AMP ** 2 < rec["level"][-1] <= 1.02 * AMP ** 2


def test_the_configured_carrier_alone_is_followed_without_a_search(tmp, exe):
    rate = 12000
    x, flags = sent(TEXT, 31.25, rate, carrier=1006.0)
    (found, _, text), (fixed, _, _) = decode(exe, tmp, [(dict(), x, flags, 180, [len(flags)]), (dict(search_hz=0.0), x, flags, 180, [len(flags)])], rate)
    assert text == TEXT and abs(found["offset_hz"][-1] - 6.0) <= 31.25 / 8
    assert (fixed["offset_hz"] == 0).all()


# ---- 3. presence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("baud", BAUDS)
def test_noise_alone_prints_nothing(tmp, exe, rate, baud):
    h = 180
    F = 60 * rate // h
    x = np.random.default_rng(NOISE_SEED).standard_normal(F * h).astype(np.float32)
    (rec, _, text), = decode(exe, tmp, [(dict(baud=baud), x, np.zeros(F, np.int32), h, [F])], rate)
    q = rec["quality"].max()
    print(f"rate {rate} baud {baud}: 60 s of noise alone, the largest coherence {q:.4f}")
    assert text == "" and rec["nchars"][-1] == 0 and rec["errors"][-1] == 0 and not rec["present"].any()
    assert q <= NOISE_COHERENCE < M.QUALITY_DEFAULT


def test_text_in_noise_at_the_lowest_ratio_that_is_read(tmp, exe):
    rate, baud = 12000, 31.25
    jobs = [(dict(), *sent(TEXT, baud, rate, snr_db=s), 180, None) for s in (LOWEST_SNR_DB, LOWEST_SNR_DB - 3)]
    jobs = [(c, x, f, h, [len(f)]) for c, x, f, h, _ in jobs]
    (at, _, tat), (below, _, tbelow) = decode(exe, tmp, jobs, rate)
    first, last = text_frames(TEXT, baud, rate)
    qmin = at["quality"][first:last].min()
    print(f"{LOWEST_SNR_DB} dB: {tat!r} errors {at['errors'][-1]} smallest coherence {qmin:.4f}; {LOWEST_SNR_DB - 3} dB: {tbelow!r} errors {below['errors'][-1]}")
    assert tat == TEXT and at["errors"][-1] == 0 and at["present"][first:last].all()
    assert tbelow != TEXT  # the measurement, again: 3 dB below the text is not read
    assert qmin >= LOWEST_COHERENCE and abs(M.QUALITY_DEFAULT - (NOISE_COHERENCE + LOWEST_COHERENCE) / 2) <= 0.0051


def test_a_steady_carrier_and_silence_print_nothing(tmp, exe):
    rate, h, F = 12000, 180, 400
    t = np.arange(F * h) / rate
    carrier = (AMP * np.cos(2 * np.pi * 1000.0 * t + 0.3)).astype(np.float32)  # on lane 8: every symbol turns by nothing
    (rc, _, tc), (rs, _, ts) = decode(exe, tmp, [(dict(), carrier, np.zeros(F, np.int32), h, [F]), (dict(), np.zeros(F * h, np.float32), np.zeros(F, np.int32), h, [F])], rate)
    assert tc == "" and rc["errors"][-1] == 0 and rc["present"][-1] == 1 and rc["quality"][-1] > 0.99 and abs(rc["level"][-1] / AMP ** 2 - 1) < 0.02
    assert ts == "" and not rs["present"].any() and not rs["level"].any() and not rs["quality"].any()


# ---- 4. the table -------------------------------------------------------------------------------------------------------------
ANCHORS = {" ": "1", "e": "11", "t": "101", "o": "111", "a": "1011", "i": "1101", "n": "1111", "r": "10101", "s": "10111", "l": "11011", "\n": "11101",
           "\r": "11111", "\0": "1010101011"}


def test_the_varicode_tables_structure_and_anchors(exe):
    line = M.run_script(exe, "tables 12000\n").splitlines()[0]
    d = M.parse_tables(line)
    codes = [bin(c)[2:] for c in d["varicode"]]
    assert tuple(d["varicode"]) == M.table() and len(codes) == 128 and len(set(codes)) == 128
    for c in codes:
        assert len(c) <= 10 and c[0] == "1" and c[-1] == "1" and "00" not in c, c
    # every string of up to 9 bits that begins and ends in 1 and holds no 00 is used: there are 88
    legal = [bin(v)[2:] for v in range(1, 512) if v & 1 and "00" not in bin(v)[2:]]
    assert len(legal) == 88 and set(legal) <= set(codes) and sum(len(c) == 10 for c in codes) == 40
    for ch, code in ANCHORS.items():
        assert codes[ord(ch)] == code, ch
    assert d["known"] == "128" and d["wrong"] == "0"  # the table by code is the table by character


def test_all_128_characters_round_trip(tmp, exe):
    rate = 12000
    text = "".join(chr(c) for c in range(128))
    x, flags = sent(text, 62.5, rate)
    (rec, _, got), = decode(exe, tmp, [(dict(baud=62.5), x, flags, 180, [len(flags)])], rate)
    assert got == text[1:] and rec["errors"][-1] == 0 and rec["nchars"][-1] == 127  # NUL is sent, read and dropped


# ---- 5. validation, defaults, plan --------------------------------------------------------------------------------------------
VERDICTS = [  # in the order they are looked for: each call holds every later fault too
    ("psk 9 1 nan 45 -1 1", "BAD_ID", "PSK decoder: id %d outside 0..%d"),
    ("psk 1 1 nan 45 -1 1", "INACTIVE", "no audio client with id %d"),
    ("psk 2 1 nan 45 -1 1", "IQ", "PSK decoder: client %d is a PSDR_IQ client, which has no audio rows"),
    ("psk 0 1 nan 45 -1 1", "BAD_CARRIER", "PSK decoder: carrier_hz %g is not a finite number inside [%g, %g]"),
    ("psk 0 1 299.9 45 -1 1", "BAD_CARRIER", None),
    ("psk 0 1 3000.1 45 -1 1", "BAD_CARRIER", None),
    ("psk 0 1 3000 45 -1 1", "BAD_BAUD", "PSK decoder: baud %g is neither %g nor %g"),
    ("psk 0 1 3000 125 -1 1", "BAD_BAUD", None),
    ("psk 0 1 3000 nan -1 1", "BAD_BAUD", None),
    ("psk 0 1 3000 31.25 -0.1 1", "BAD_SEARCH", "PSK decoder: search_hz %g is not a finite number inside [0, %g), half the baud rate"),
    ("psk 0 1 3000 31.25 15.625 1", "BAD_SEARCH", None),
    ("psk 0 1 3000 62.5 nan 1", "BAD_SEARCH", None),
    ("psk 0 1 3000 62.5 31 1", "BAD_QUALITY", "PSK decoder: quality %g is not a finite number inside (0, 1)"),
    ("psk 0 1 3000 62.5 0 0", "BAD_QUALITY", None),
    ("psk 0 1 3000 62.5 0 nan", "BAD_QUALITY", None),
    ("psk 0 1 3000 62.5 0 0.5", "BAD_RATE", "PSK decoder: the context's audio_rate %d is outside [%d, %d]"),
]
BAND = "PSK decoder: the lanes from %g to %g Hz do not lie inside [%g Hz, %g of the audio_rate %d]"


def test_every_refusal_in_order_with_a_text_of_its_own(exe):
    script = "case v\nrate 3999\nadd 0\nadd 2\nkind 2 4 0 0\n" + "".join(v[0] + "\n" for v in VERDICTS)
    last = VERDICTS[-1][0]
    script += ("psk 2 0 0 0 0 0\npsk 1 0 0 0 0 0\nrate 48001\n" + last + "\nrate 48000\n" + last + "\nrate 4000\n" + last + "\n"  # 3054.7 Hz: over 0.45 x 4000
               "psk 0 1 1772.65625 31.25 0 0.5\npsk 0 1 1772.7 31.25 0 0.5\npsk 0 1 1745.3125 62.5 0 0.5\npsk 0 1 1745.4 62.5 0 0.5\n"
               "psk 0 1 1000 31.25 11.71875 0.51\ndump\n")
    out = M.run_script(exe, script).splitlines()
    got = [ln.split("verdict=")[1] for ln in out if ln.startswith("set ")]
    assert got == [v[1] for v in VERDICTS] + ["OK", "INACTIVE", "BAD_RATE", "OK", "BAD_BAND", "OK", "BAD_BAND", "OK", "BAD_BAND", "OK"]
    slot0 = [ln for ln in out if ln.startswith("pks slot=0 ")][0]
    assert " on=1 fresh=1 " in slot0 and f" wn={M.wn_of(31.25, 4000)} " in slot0 and f" u={M.u_of(31.25, 4000)} " in slot0 and " cand=0fe0 " in slot0
    inc = M.increments(4000, 1000.0, 31.25)
    assert f" inc0={inc[0]} inc8={inc[8]} inc15={inc[15]}" in slot0
    src = open(os.path.join(ROOT, "phantomsdr_amd", "csrc", "demod.hip")).read()
    texts = [v[2] for v in VERDICTS if v[2]] + [BAND]
    assert len(set(texts)) == len(texts) == 9
    for verdict, text in list({v[1]: v[2] for v in VERDICTS if v[2]}.items()) + [("BAD_BAND", BAND)]:
        m = re.search(r"case PSK_%s: return fail\((PSDR_ERR_\w+), \"([^\"]*)\"" % verdict, src)
        assert m and m.group(2) == text and m.group(1) == ("PSDR_ERR_STATE" if verdict in ("BAD_RATE", "BAD_BAND") else "PSDR_ERR_INVALID"), verdict
    order = [src.index("case PSK_%s:" % v) for v in ("BAD_ID", "INACTIVE", "IQ", "BAD_CARRIER", "BAD_BAUD", "BAD_SEARCH", "BAD_QUALITY", "BAD_RATE", "BAD_BAND")]
    assert order == sorted(order)


def test_defaults_and_tables(exe):
    rates = (4000, 7999, 8000, 16000, 48000)
    out = M.run_script(exe, "".join(f"defaults {r}\n" for r in rates) + "defaults 3999.9\ndefaults 48000.1\ndefaults nan\n" + "".join(f"tables {r}\n" for r in RATES + (7900,))).splitlines()
    for line, rate in zip(out, rates):
        assert line.startswith(f"defaults rate={rate} ok=1 carrier_hz=1000 baud=31.25 search_hz=11.71875 quality=") and float(line.split("quality=")[1]) == M.QUALITY_DEFAULT, line
    assert all(" ok=0 " in ln for ln in out[5:8])
    for line, rate in zip(out[8:], RATES + (7900,)):
        d = M.parse_tables(line)
        H = M.hop_of(rate)
        assert int(d["H"]) == H and 0.001 <= H / rate <= 0.002 and int(d["fill"]) == M.FILL
        assert (int(d["wn31"]), int(d["wn63"]), int(d["u31"]), int(d["u63"])) == (M.wn_of(31.25, rate), M.wn_of(62.5, rate), M.u_of(31.25, rate), M.u_of(62.5, rate))
        assert 8 <= int(d["wn63"]) <= int(d["wn31"]) <= M.WMAX and 128 <= int(d["u63"])
    assert M.wn_of(62.5, 4000) == 8 and M.wn_of(31.25, 7900) == 32 and M.wn_of(31.25, 7999) == 32


def test_plan_lists_and_zeroes(exe):
    """psk_plan behind demod_plan: who is listed and whose state starts from zero"""
    on = "1000 31.25 11.71875 0.51"
    script = ("case plan\nadd 0\nadd 1\nadd 2\nadd 3\nwindow 0 100 100.3 200\nwindow 1 100 100.3 200\nwindow 2 100 100.3 200\nwindow 3 100 100.3 200\n"
              "batch\n"                                      # no PSK client yet: nothing
              f"psk 1 1 {on}\npsk 3 1 1500 62.5 0 0.4\nbatch\n"   # both from zero
              "batch\n"                                      # carried
              f"psk 1 1 {on}\nbatch\n"                       # again on: from zero
              "window 3 101 101.3 201\nkind 1 1 0 0\npause 0\nbatch\n"   # a retune and a mode change start over
              "kind 3 4 0 0\nbatch\n"                        # an IQ client keeps its setting and is not listed
              "kind 3 0 0 0\npsk 1 0 0 0 0 0\nbatch\ndump\n")
    lines = M.run_script(exe, script).splitlines()
    p = [dict(kv.split("=", 1) for kv in ln.split()[1:]) for ln in lines if ln.startswith("pkp")]
    assert p[0]["have"] == "0" and p[0]["any"] == "0"
    assert (p[1]["n"], p[1]["zero"]) == ("2", "1,3") and (p[2]["n"], p[2]["zero"]) == ("2", "") and (p[3]["n"], p[3]["zero"]) == ("2", "1")
    e = p[1]["list"].split(",")[1].split(":")
    assert e[:3] == ["3", str(M.wn_of(62.5, 12000)), str(M.u_of(62.5, 12000))] and e[4] == "0100" and int(e[5]) == M.increments(12000, 1500.0, 62.5)[8]
    assert (p[4]["n"], p[4]["zero"]) == ("2", "1,3")
    assert (p[5]["n"], p[5]["zero"]) == ("1", "") and p[5]["list"].startswith("1:")
    assert (p[6]["n"], p[6]["zero"]) == ("1", "") and p[6]["list"].startswith("3:")  # back from IQ: the state stood still, as a paused one
    s = [dict(kv.split("=", 1) for kv in ln.split()[1:]) for ln in lines if ln.startswith("pks")]
    assert [d["on"] for d in s[:4]] == ["0", "0", "0", "1"] and [d["b_on"] for d in s[:4]] == ["0", "0", "0", "1"]


def test_header_and_python_mirror():
    import ctypes

    import phantomsdr_amd as P
    from phantomsdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "psdr.h")).read()
    assert "#define PSDR_ABI_VERSION 3" in hdr and "#define PSDR_PSK_LANES 16" in hdr  # additions only
    assert f"#define PSDR_PSK_QUALITY_DEFAULT {M.QUALITY_DEFAULT!r}" in hdr
    names = [s[0] for s in _lib.SYMBOLS]
    for sym in ("psdr_client_set_psk_decoder", "psdr_psk_defaults", "psdr_read_psk", "psdr_read_psk_text"):
        assert sym in names and re.search(r"\bint %s\(" % sym, hdr), sym
    assert ctypes.sizeof(_lib.psdr_psk_config) == 32
    for attr in ("set_psk_decoder", "read_psk", "read_psk_text"):
        assert hasattr(P.AudioClient, attr), attr
    assert callable(P.psk_defaults) and "psk" in __import__("phantomsdr_amd.build", fromlist=["UNITS"]).UNITS
    for words in ("QPSK31 (it needs a Viterbi decoder)", "PSK125", "the false lock every PSK31\n *     program knows", "Nobody has tried it on off-air PSK31"):
        assert words in hdr, words
    lib = os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so")
    if os.path.exists(lib):  # the four symbols in the built library
        dll = ctypes.CDLL(lib)
        for sym in ("psdr_client_set_psk_decoder", "psdr_psk_defaults", "psdr_read_psk", "psdr_read_psk_text"):
            assert hasattr(dll, sym), sym

"""The tone decoder's host side (phantomsdr_amd/csrc/toneplan.h; include/psdr.h: psdr_client_set_tone_decoder), without a device:
tests/tone_plan_table.cpp runs the text k_audio_tone runs, tests/tone_model.py restates the rule in numpy."""
import os
import re

import numpy as np
import pytest

import squelch_model
import tone_model as M
from conftest import ROOT

RATES = (2000, 8000, 12000, 48000)
SNR_DB = 22.0
# the level against a float64 evaluation with exact phases, measured once on tone_inputs() at 8000, 12000 and 48000: worst relative
# error 7.82e-6 (the f32 sum over up to 19 200 samples); the bound is four times that, for other seeds.  Rate 2000, added to RATES
# later, shows 9.04e-6 - the worst of the four now - under the same bound
LEVEL_ERR_MEASURED = 7.82e-6
LEVEL_ERR_BOUND = 4 * LEVEL_ERR_MEASURED


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("tone_host")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


def stream_180(F=120, h=180, rate=12000):
    """a stream that opens the gate, holds a flagged frame, and closes again: noise, then tone 12 in noise, then noise"""
    rng = np.random.default_rng(1)
    t = np.arange(F * h)
    x = 0.05 * rng.standard_normal(F * h)
    x[10 * h:70 * h] += 0.1 * np.cos(2 * np.pi * 100.0 * t[10 * h:70 * h] / rate + 0.3)
    flags = np.zeros(F, np.int32)
    flags[50] = 1
    prev = np.zeros(F, np.int32)
    prev[[3, 60]] = 1
    return x.astype(np.float32), flags, prev


# (the issue's "5 x 6": batches of 5 and 6 frames in turn, then the last 10 frames - tests/test_gpu_tone_decoder.py reads it the same way)
SPLITS = ([120], [1] * 120, [3] * 40, [5, 6] * 10 + [10], [40] * 3)


def test_one_definition_and_split_invariance(tmp, exe):
    """contraction on and off print the same bits; every split of the stream gives the uncut stream's records, drop flags and
    final state; and they are the numpy model's records exactly"""
    x, flags, prev = stream_180()
    cfg = dict(hang=2)
    jobs = [(cfg, x, flags, prev, 180, fr) for fr in SPLITS]
    builds = [exe, M.build_table(tmp, ROOT, ("-mfma", "-ffp-contract=fast"), "tone_fast"), M.build_table(tmp, ROOT, ("-ffp-contract=off",), "tone_off")]
    outs = [M.run_streams(e, tmp, jobs) for e in builds]
    ref = outs[0][0]
    for o in outs:
        for rec, drop, st in o:
            assert rec.tobytes() == ref[0].tobytes() and drop.tobytes() == ref[1].tobytes() and st[-1].tobytes() == ref[2][-1].tobytes()
    rec, drop = M.records(x.reshape(120, 180), flags, 180, 12000, hang=2, prev_drop=prev)
    assert rec.tobytes() == ref[0].tobytes() and np.array_equal(drop, ref[1])
    # the stream holds what it is meant to: an opening, the tone named, a closing, drop = prev | !open
    assert ref[0]["open"][0] == 0 and ref[0]["open"][60] == 1 and ref[0]["open"][-1] == 0 and (ref[0]["tone"][40:70] == 12).all()
    assert np.array_equal(ref[1], ((prev != 0) | (ref[0]["open"] == 0)).astype(np.int32))
    assert ref[2][-1]["pos"] == 120 * 180 and np.array_equal(ref[2][-1]["part"][:96], x[-96:]) and not ref[2][-1]["part"][96:].any()


@pytest.mark.parametrize("rate", RATES)
def test_identification_and_truth(tmp, exe, rate):
    x, k = M.tone_inputs(rate)
    best, q, _ = M.windows64(x, rate)
    print(f"rate {rate}: named {int((best == k).sum())} of {len(k)}, worst P_best / ref {10 * np.log10(q.min()):.1f} dB")
    assert np.array_equal(best, k) and set(k.tolist()) == set(range(50))
    assert (10 * np.log10(q) >= SNR_DB).all()
    _, nq, _ = M.windows64(M.noise_inputs(rate), rate)
    print(f"rate {rate}: largest noise-only ratio in {len(nq)} windows {10 * np.log10(nq.max()):.1f} dB")
    assert len(nq) == 300 and (10 * np.log10(nq) < SNR_DB).all()  # no hit
    # the plan program on the same windows (f32): it names the tones too, and its level is the truth's
    nb = M.nb_of(rate)
    x32 = x.astype(np.float32)
    outs = M.run_streams(exe, tmp, [(dict(gate=0, attack=1), xi, np.zeros(nb, np.int32), None, 256, [nb]) for xi in x32], rate=rate)
    tone = np.array([o[0]["tone"][-1] for o in outs])
    level = np.array([o[0]["level"][-1] for o in outs], np.float64)
    assert np.array_equal(tone, k) and all((o[0]["tone"][:-1] == -1).all() and o[0]["open"][-1] == 1 for o in outs)
    _, _, truth = M.windows64(x32.astype(np.float64), rate)
    err = np.abs(level - truth) / truth
    print(f"rate {rate}: level against float64 truth, worst relative error {err.max():.3g} (bound {LEVEL_ERR_BOUND:.3g}); level {level.mean():.4g}")
    assert err.max() <= LEVEL_ERR_BOUND
    assert abs(level.mean() / 0.01 - 1) < 0.1  # amplitude 0.1: the squared amplitude, in the units of the rows


def test_the_model_in_f32_names_the_tones_too():
    """records() - the rule's own arithmetic - on one window per tone at 12 kHz"""
    x, k = M.tone_inputs(12000, phases=1)
    nb = M.nb_of(12000)
    for xi, ki in zip(x.astype(np.float32), k):
        rec = M.records(xi.reshape(nb, 256), np.zeros(nb, np.int32), 256, 12000, attack=1)
        assert rec["tone"][-1] == ki and rec["open"][-1] == 1 and (rec["tone"][:-1] == -1).all()


@pytest.mark.parametrize("attack,hang", [(1, 0), (2, 2), (3, 1), (1, 5)])
def test_gate_is_the_squelch_models_state_machine(exe, attack, hang):
    rng = np.random.default_rng(attack * 10 + hang)
    scripts = ["0110111000011110100000001", "1" * 8 + "0" * 8, "".join("01"[int(b)] for b in rng.integers(0, 2, 200)),
               "".join("01"[int(b)] for b in (rng.random(200) < 0.8))]
    out = M.run_script(exe, "".join(f"gate {attack} {hang} {s}\n" for s in scripts)).splitlines()
    for s, line in zip(scripts, out):
        m = re.fullmatch(r"gate attack=(\d+) hang=(\d+) open=([01]+) tone=([7-]+) cnt=(\d+)", line)
        hits = np.array([int(c) for c in s], np.float32)
        want, (_, cnt) = squelch_model.run(hits, 0.5, 0.5, attack, hang)
        assert m and m.group(3) == "".join(str(v) for v in want) and int(m.group(5)) == cnt
        assert m.group(4) == "".join("7" if c == "1" else "-" for c in s)  # the tone is the last decision's, whatever the gate


def test_frames_in_which_no_block_or_several_complete(exe):
    out = M.run_script(exe, "frames 0 180 6\nframes 0 2 300\nframes 0 1024 3\nframes 100 600 4\nframes 255 2 2\nframes 256 256 2\n").splitlines()

    def done(pos0, h, nf):
        return ",".join(str((pos0 + (f + 1) * h) // 256) for f in range(nf))

    cases = [(0, 180, 6), (0, 2, 300), (0, 1024, 3), (100, 600, 4), (255, 2, 2), (256, 256, 2)]
    for (pos0, h, nf), line in zip(cases, out):
        assert line == f"frames pos0={pos0} h={h} done={done(pos0, h, nf)}", line
    # h = 2: 127 frames in a row complete no block; h = 1024: every frame completes four
    assert done(0, 1024, 3) == "4,8,12" and done(0, 2, 300).startswith("0," * 127 + "1,")


def test_records_at_a_frame_of_several_blocks(tmp, exe):
    """h = 1024 at 8 kHz: four blocks per frame, the record is the last one's; against the model"""
    rate, h, F = 8000, 1024, 8
    rng = np.random.default_rng(5)
    t = np.arange(F * h)
    x = (0.1 * np.cos(2 * np.pi * 67.0 * t / rate) + 0.05 * rng.standard_normal(F * h)).astype(np.float32)
    flags = np.zeros(F, np.int32)
    (rec, _, _), = M.run_streams(exe, tmp, [(dict(attack=1), x, flags, None, h, [3, 5])], rate=rate)
    assert rec.tobytes() == M.records(x.reshape(F, h), flags, h, rate, attack=1).tobytes()
    assert (rec["tone"][:3] == -1).all() and (rec["tone"][3:] == 0).all()  # NB = 13: the first decision falls into frame 3


VERDICTS = [  # in the order they are looked for: each call holds every later fault too
    ("tone 9 1 99 5 nan -1 0 -1", "BAD_ID", "tone decoder: id %d outside 0..%d"),
    ("tone 1 1 99 5 nan -1 0 -1", "INACTIVE", "no audio client with id %d"),
    ("tone 2 1 99 5 nan -1 0 -1", "IQ", "tone decoder: client %d is a PSDR_IQ client, which has no audio rows"),
    ("tone 0 1 99 5 nan -1 0 -1", "BAD_WANT", "tone decoder: want %d outside %d..%d"),
    ("tone 0 1 -2 5 nan -1 0 -1", "BAD_WANT", None),
    ("tone 0 1 49 5 nan -1 0 -1", "BAD_GATE", "tone decoder: gate %d outside 0..1"),
    ("tone 0 1 -1 1 nan -1 0 -1", "BAD_SNR", "tone decoder: snr_db %g is not a finite number inside [%g, %g]"),
    ("tone 0 1 -1 1 5.9 -1 0 -1", "BAD_SNR", None),
    ("tone 0 1 -1 1 60.1 -1 0 -1", "BAD_SNR", None),
    ("tone 0 1 -1 0 6 -1 0 -1", "BAD_LEVEL", "tone decoder: min_level %g is not a finite number at or above 0"),
    ("tone 0 1 -1 0 60 inf 0 -1", "BAD_LEVEL", None),
    ("tone 0 1 -1 0 22 0 0 -1", "BAD_ATTACK", "tone decoder: attack_blocks %d outside 1..%d"),
    ("tone 0 1 -1 0 22 0 1025 -1", "BAD_ATTACK", None),
    ("tone 0 1 -1 0 22 0 1 -1", "BAD_HANG", "tone decoder: hang_blocks %d outside 0..%d"),
    ("tone 0 1 -1 0 22 0 1024 1025", "BAD_HANG", None),
    ("tone 0 1 -1 0 22 0 1024 1024", "BAD_RATE", "tone decoder: the context's audio_rate %d is outside [%d, %d]"),
]


def test_every_refusal_in_order_with_a_text_of_its_own(exe):
    script = "case v\nrate 1999\nadd 0\nadd 2\nkind 2 4 0 0\n" + "".join(v[0] + "\n" for v in VERDICTS)
    script += "tone 2 0 0 0 0 0 0 0\ntone 1 0 0 0 0 0 0 0\nrate 48001\n" + VERDICTS[-1][0] + "\nrate 48000\n" + VERDICTS[-1][0] + "\nrate 2000\n" + VERDICTS[-1][0] + "\n"
    got = [ln.split("verdict=")[1] for ln in M.run_script(exe, script).splitlines() if ln.startswith("set ")]
    assert got == [v[1] for v in VERDICTS] + ["OK", "INACTIVE", "BAD_RATE", "OK", "OK"]  # (off: an IQ client may; the rate's ends are inside)
    src = open(os.path.join(ROOT, "phantomsdr_amd", "csrc", "demod.hip")).read()
    texts = [v[2] for v in VERDICTS if v[2]]
    assert len(set(texts)) == len(texts) == 10
    for verdict, text in {v[1]: v[2] for v in VERDICTS if v[2]}.items():
        m = re.search(r"case TONE_%s: return fail\((PSDR_ERR_\w+), \"([^\"]*)\"" % verdict, src)
        assert m and m.group(2) == text and m.group(1) == ("PSDR_ERR_STATE" if verdict == "BAD_RATE" else "PSDR_ERR_INVALID"), verdict


def test_defaults(exe):
    out = M.run_script(exe, "defaults 8000\ndefaults 12000\ndefaults 48000\ndefaults 2000\ndefaults 1999.9\ndefaults 48000.1\ndefaults nan\n").splitlines()
    for line, (rate, nb) in zip(out, ((8000, 13), (12000, 19), (48000, 75), (2000, 4))):
        assert line == f"defaults rate={rate} ok=1 want=-1 gate=1 snr_db=22 min_level=0 attack=2 hang={nb}", line
        assert M.nb_of(rate) == nb
    assert all(" ok=0 " in ln for ln in out[4:]) and len(out) == 7


def test_tables_are_the_models(tmp, exe):
    path = str(tmp / "tables.bin")
    M.run_script(exe, f"tables 12000 {path}\n")
    raw = open(path, "rb").read()
    assert len(raw) == 66616
    inc = np.frombuffer(raw, np.uint32, 64, 65536)
    h = np.frombuffer(raw, np.float32, 76, 65536 + 256 + 512)
    nb, = np.frombuffer(raw, np.int32, 1, 66608)
    lscale, = np.frombuffer(raw, np.float32, 1, 66612)
    wh, wl = M.window(12000)
    assert nb == 19 and np.array_equal(inc[:50], M.increments(12000).astype(np.uint32)) and not inc[50:].any()
    assert h[:19].tobytes() == wh.tobytes() and not h[19:].any() and lscale == wl
    assert inc[12] == round(100.0 / 12000 * 2 ** 32)


def test_plan_lists_zeroes_and_copies(exe):
    """tone_plan behind demod_plan: who is listed, whose state starts from zero, the chain's copy entries"""
    script = ("case plan\nadd 0\nadd 1\nadd 2\nadd 3\nwindow 0 100 100.3 200\nwindow 1 100 100.3 200\nwindow 2 100 100.3 200\nwindow 3 100 100.3 200\n"
              "batch\n"                                   # no tone client yet: nothing
              "tone 1 1 12 1 22 0 2 19\ntone 3 1 -1 0 22 0 2 19\nbatch\n"   # both from zero; no chain: no copies
              "post on\nbatch\n"                          # the chain: slot 1 is gated, slots 0 and 2 are copied
              "tone 1 1 12 0 22 0 2 19\nbatch\n"          # again on: from zero; nobody gated: no copies
              "window 3 101 101.3 201\nkind 1 1 0 0\npause 0\nbatch\n"  # a retune and a mode change start over
              "kind 3 4 0 0\nbatch\n"                     # an IQ client keeps its setting and is not listed
              "kind 3 0 0 0\ntone 1 0 0 0 0 0 0 0\nbatch\ndump\n")
    lines = [ln for ln in M.run_script(exe, script).splitlines() if ln.startswith("tonep") or ln.startswith("tones")]
    p = [dict(kv.split("=", 1) for kv in ln.split()[1:]) for ln in lines if ln.startswith("tonep")]
    assert p[0]["have"] == "0" and p[0]["any"] == "0"
    assert (p[1]["n"], p[1]["ncopy"], p[1]["gated"], p[1]["zero"]) == ("2", "0", "0", "1,3")
    assert (p[2]["n"], p[2]["ncopy"], p[2]["gated"], p[2]["zero"]) == ("2", "2", "1", "")
    assert [e.split(":")[0] for e in p[2]["list"].split(",")] == ["1", "3", "0", "2"] and p[2]["list"].split(",")[2].split(":")[3] == "0"
    assert (p[3]["n"], p[3]["ncopy"], p[3]["gated"], p[3]["zero"]) == ("2", "0", "0", "1")
    assert (p[4]["n"], p[4]["zero"]) == ("2", "1,3")
    assert (p[5]["n"], p[5]["zero"]) == ("1", "") and p[5]["list"].startswith("1:")
    assert (p[6]["n"], p[6]["zero"]) == ("1", "") and p[6]["list"].startswith("3:")  # back from IQ: the state stood still, as a paused one
    s = [dict(kv.split("=", 1) for kv in ln.split()[1:]) for ln in lines if ln.startswith("tones")]
    assert [d["on"] for d in s[:4]] == ["0", "0", "0", "1"] and [d["b_on"] for d in s[:4]] == ["0", "0", "0", "1"]


def test_header_and_python_mirror():
    import ctypes

    import phantomsdr_amd as P
    from phantomsdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "psdr.h")).read()
    assert "#define PSDR_ABI_VERSION 3" in hdr and "#define PSDR_TONE_COUNT 50" in hdr and "#define PSDR_TONE_ANY (-1)" in hdr  # additions only
    names = [s[0] for s in _lib.SYMBOLS]
    for sym in ("psdr_client_set_tone_decoder", "psdr_tone_defaults", "psdr_tone_table", "psdr_read_tone"):
        assert sym in names and re.search(r"\bint %s\(" % sym, hdr), sym
    assert ctypes.sizeof(_lib.psdr_tone_config) == 32 and P.TONE_ANY == -1
    assert hasattr(P.AudioClient, "set_tone_decoder") and hasattr(P.AudioClient, "read_tone") and callable(P.tone_defaults) and callable(P.tone_table)
    src = open(os.path.join(ROOT, "phantomsdr_amd", "csrc", "toneplan.h")).read()
    tab = [float(v) for v in re.search(r"TONE_HZ\[TONE_N\] = \{([^}]*)\}", src).group(1).split(",")]
    assert tab == M.HZ and tab == sorted(tab) and len(tab) == 50
    assert "tone" in __import__("phantomsdr_amd.build", fromlist=["UNITS"]).UNITS

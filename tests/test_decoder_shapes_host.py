"""The decoders' host table programs and numpy models at the cases of tests/decoder_shapes.py, without a GPU.

tests/tone_plan_table.cpp and tests/cw_plan_table.cpp run the text the kernels run (toneplan.h, cwplan.h); tests/tone_model.py's and
tests/cw_model.py's records() restate the rule in numpy and are what tests/test_gpu_tone_shapes.py and tests/test_gpu_cw_shapes.py hold
the GPU to.  Here the two are held to each other, to the bit, at every case's rate, frame length and batches - whole and split - on
synthetic rows (cw_model.keyed_sine in noise; tone_model.tone_inputs and noise_inputs) with one flagged frame: a GPU mismatch at a
new shape then points at the kernel and not at the model.  The same runs evaluate the table's conditions - cw_rules, tone_rules - on
the model's records: none may be broken."""
import os
import re

import numpy as np
import pytest

import create_plan_table
import cw_model as CW
import decoder_shapes as S
import tone_model as TM
from conftest import ROOT


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("decoder_shapes")


@pytest.fixture(scope="module")
def cw_exe(tmp):
    return CW.build_table(tmp, ROOT)


@pytest.fixture(scope="module")
def tone_exe(tmp):
    return TM.build_table(tmp, ROOT)


@pytest.mark.parametrize("rate,n", S.CW_CASES)
def test_cw_program_and_model_agree_and_the_conditions_hold(tmp, cw_exe, rate, n):
    h = n // 2
    nf = S.cw_timing(rate, n)[0]
    x, flags = S.cw_synthetic(rate, n)
    split = S.split_of(nf, h)
    want, wtext = CW.records(x.reshape(nf, h), flags, h, rate, **S.CW_CFG)
    outs = CW.run_streams(cw_exe, tmp, [(S.CW_CFG, x, flags, h, list(b)) for b in ((nf,), split)], tag=f"cw{rate}_{n}_", rate=rate)
    for (rec, states, text), b in zip(outs, ("whole", "split")):
        bad = [f for f in range(nf) if rec[f].tobytes() != want[f].tobytes()]
        assert not bad, (b, bad[:8], rec[bad[:4]], want[bad[:4]])
        assert text == wtext and int(states[-1]["nchars"]) == len(wtext) and int(states[-1]["pos"]) == nf * h, b
    assert outs[0][1][-1].tobytes() == outs[1][1][-1].tobytes(), "the final state of the two runs"
    broken = S.cw_rules(rate, h, split, want, wtext, flags)
    print(f"cw rate {rate} n {n}: frames {nf} batches {split} text {wtext!r} {broken}")
    assert not broken, broken
    assert wtext == S.TEXT and abs(want["pitch_hz"][-1] - S.PITCH) <= CW.DF  # (the synthetic rows are clean at every h)


@pytest.mark.parametrize("rate,n", S.TONE_CASES)
def test_tone_program_and_model_agree_and_the_conditions_hold(tmp, tone_exe, rate, n):
    h = n // 2
    nf, off, nan_frame = S.tone_timing(rate, n)
    x, flags = S.tone_synthetic(rate, n)
    split = S.split_of(nf, h)
    prev = flags.copy()
    for gate in (0, 1):
        cfg = dict(gate=gate, hang=2)
        want, wdrop = TM.records(x.reshape(nf, h), flags, h, rate, prev_drop=prev, **cfg)
        outs = TM.run_streams(tone_exe, tmp, [(cfg, x, flags, prev, h, list(b)) for b in ((nf,), split)], tag=f"tone{rate}_{n}_", rate=rate)
        for (rec, drop, states), b in zip(outs, ("whole", "split")):
            bad = [f for f in range(nf) if rec[f].tobytes() != want[f].tobytes()]
            assert not bad, (b, gate, bad[:8], rec[bad[:4]], want[bad[:4]])
            assert np.array_equal(drop, wdrop) and int(states[-1]["pos"]) == nf * h, (b, gate)
        assert outs[0][2][-1].tobytes() == outs[1][2][-1].tobytes(), "the final state of the two runs"
    assert wdrop[nan_frame] and (wdrop == 0).any() and np.array_equal(wdrop, ((prev != 0) | (want["open"] == 0)).astype(np.int32))
    broken = S.tone_rules(rate, h, split, want, flags)
    print(f"tone rate {rate} n {n}: frames {nf} (tone off at {off}) batches {split} open {int(want['open'].sum())} frames {broken}")
    assert not broken, broken
    named = want["tone"][want["open"] == 1]  # (the windows' phases jump: at nb = 4 a neighbour is named now and then)
    assert 2 * np.count_nonzero(named == S.TONE) > len(named)


def test_the_case_tables():
    src = {nm: open(os.path.join(ROOT, "phantomsdr_amd", "csrc", nm)).read() for nm in ("cwplan.h", "toneplan.h")}
    assert re.search(r"constexpr int CW_GROUP = (\d+);", src["cwplan.h"]).group(1) == str(S.CW_GROUP)
    assert re.search(r"constexpr int CW_HMAX = (\d+);", src["cwplan.h"]).group(1) == str(S.CW_HMAX)
    assert re.search(r"constexpr int TONE_GROUP = (\d+);", src["toneplan.h"]).group(1) == str(S.TONE_GROUP)
    assert "inline int tone_ring(int nb) { return nb - 1 + TONE_GROUP; }" in src["toneplan.h"]
    # what each case is there for
    assert [(CW.hop_of(r), n // 2) for r, n in S.CW_CASES] == [(32, 180), (128, 180), (256, 180), (256, 256), (64, 360), (64, 518), (64, 1200), (64, 6), (64, 2)]
    assert [(TM.nb_of(r), n // 2) for r, n in S.TONE_CASES] == [(4, 180), (4, 1200), (75, 256), (13, 518), (19, 360), (19, 1200), (19, 6), (19, 2)]
    assert {CW.hop_of(r) for r, _ in S.CW_TRUTH} == {32, 64, 128, 256} and set(S.CW_CASES) - set(S.CW_TRUTH) == {(12000, 12)}
    assert {r for r, _ in S.TONE_GATED} == {r for r, _ in S.TONE_CASES} and set(S.TONE_GATED) <= set(S.TONE_CASES) and S.TWIN in S.TONE_CASES
    for rate, n in set(S.CW_CASES + S.TONE_CASES):
        create_plan_table.idft(n)  # (asserts that the plan is accepted)
        l, _, r = S.window(n)
        assert 1 <= r - l <= n
    # n = 4: the whole configuration plans, with the longest batch of both tables
    longest = max(S.cw_timing(12000, 4)[0], S.tone_timing(12000, 4)[0])
    p = create_plan_table.plan(S.N, 0, levels=S.LEVELS, additional=4, audio=4, rate=12000, batch=longest, clients=3)
    assert p["shape"]["n"] == "4" and longest > 200
    for rate, n in S.CW_CASES:
        nf, lead, runs, nan_t = S.cw_timing(rate, n)
        H, h = CW.hop_of(rate), n // 2
        assert lead * rate >= 1.1 * CW.RING * H and nf * h / rate < 3.0
        split = S.split_of(nf, h)
        assert max(split) >= 7 and 1 in split and (h > 6 or (max(split) > 200 and 20 in split and 41 in split))
        if (rate, n) == (32000, 360):  # the carried partial hop passes 192 samples: all four waves store it
            assert any(int(p) % H > 192 for p in S.bounds(split, h))
        if (rate, n) == (12000, 2400):  # five groups in a one-frame batch
            assert max(S.single_frame_units(split, h, H)) > 4 * S.CW_GROUP
    for rate, n in S.TONE_CASES:
        nf, off, _ = S.tone_timing(rate, n)
        h, win = n // 2, TM.nb_of(rate) * TM.B
        assert off * h >= 3 * win and (nf - off) * h >= 2 * win - h
    # the rules notice what they are there for
    rec = np.zeros(40, CW.REC_DTYPE)
    assert S.cw_rules(12000, 180, (40,), rec, "", np.zeros(40)) == ["key does not take both values", "the text is shorter than 3 characters or holds no space",
                                                                     "no batch boundary inside a hop", "no batch of one frame", "no flagged frame"]
    assert "no one-frame batch completes more than CW_GROUP hops" in S.cw_rules(12000, 1200, (5,), rec, "", np.zeros(5))
    assert "no batch completes no hop" in S.cw_rules(12000, 6, (11, 11), rec, "", np.zeros(22))
    rec = np.zeros(8, TM.REC_DTYPE)
    assert S.tone_rules(2000, 256, (3,), rec[:3], np.zeros(3)) == ["the gate does not open and later close", "fewer than 2 ring + TONE_GROUP blocks", "no batch of one frame",
                                                               "no flagged frame", "no group wraps the ring inside the group"]
    rec["open"][2:] = 1
    assert "the gate does not open and later close" in S.tone_rules(12000, 256, (8,), rec, np.zeros(8))
    assert "no batch boundary inside a block" in S.tone_rules(12000, 128, (2, 2), rec, np.zeros(4))
    assert "no batch completes no block" in S.tone_rules(12000, 6, (43, 43), rec, np.zeros(86))
    assert "no one-frame batch completes more than TONE_GROUP blocks" in S.tone_rules(12000, 1200, (16, 1), rec, np.zeros(17))

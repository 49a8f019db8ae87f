"""What tests/test_gpu_post_chain_ragged.py covers, checked on the host (cases: tests/post_chain_ragged.py).

1. Every case resolves - through the library's own pc_resolve, as tests/test_post_chain_forms_cover.py does - to the plan
   literal of the forms case it takes its geometry from.
2. rules() holds for every case: the drop script has every edge the module text lists, the features sit where they should.
3. The kernels the cases launch - derived from each case's plan and from whether a batch travels with a profile table -
   against a written-out set: a change that moves a case onto another kernel fails here.
4. Each case's expected PCM with the oracle's demodulator in the GPU's place: every client with at least 1000 non-zero samples
   and one in the last batch, no NaN in an unflagged row, the squelch model's flags with an opening and a closing.
5. agc_profile_model.model_runs equals the oracle's AGC bit for bit at every rate the cases use."""
import numpy as np
import pytest

import agc_profile_model as M
import post_chain_forms as PF
import post_chain_ragged as R
from conftest import ROOT
from oracle import oracle as O


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return PF.build_plan_table(tmp_path_factory.mktemp("post_chain_ragged"))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("post_chain_ragged_agc")


@pytest.fixture(scope="module")
def exe(tmp):
    return M.build_table(tmp, ROOT)


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_resolves_to_its_plan(table, name):
    case = R.CASES[name]
    assert case._replace(batches=()) == PF.CASES[name]._replace(batches=()), "the geometry is the forms case's"
    (got,) = PF.resolve(table, PF.case_points(case))
    want = dict(case.plan, verdict="OK")
    assert {k: got[k] for k in want} == {k: str(v) for k, v in want.items()}, got


@pytest.mark.parametrize("name", list(R.CASES))
def test_rules_hold(name):
    assert not R.rules(name)


# what "Why" of the cases names, as post_chain_ragged.kernels() spells it: the moving averages, the recurrences with 32 and 64
# lanes, own and not, with and without the profile table, the scalar gather / output, k_pc_agc at h = 16, DIRECT
LAUNCHED = {
    "k_pc_index", "k_pc_history", "k_pc_gather", "k_pc_gather4", "k_pc_out", "k_pc_out4", "k_pc_submax", "k_pc_prefix", "k_pc_want", "k_pc_want_prof",
    "k_pc_cm", "k_pc_cscan", "k_pc_zero",
    "k_pc_ma<false, true> lanes=32", "k_pc_ma<true, true> lanes=32", "k_pc_ma<false, false> lanes=32", "k_pc_ma<true, false> lanes=32",
    "k_pc_ma<false, false> lanes=64", "k_pc_ma<true, false> lanes=64",
    "k_pc_ma2<true, true> lanes=32", "k_pc_ma2<true> DIRECT lanes=32", "k_pc_ma2<true> DIRECT lanes=64", "k_pc_ma2<false> DIRECT lanes=64",
    "k_pc_mad<true> lanes=64", "k_pc_mad<false> lanes=64",
    "k_pc_gain<true, true> lanes=32", "k_pc_gain<true, true, PcWithProfiles> lanes=32",
    "k_pc_gain<true, true> lanes=64", "k_pc_gain<true, true, PcWithProfiles> lanes=64",
    "k_pc_gain<true, false> lanes=64", "k_pc_gain<true, false, PcWithProfiles> lanes=64",
    "k_pc_agc<true, false> h=124 lanes=32", "k_pc_agc<true, false, PcWithProfiles> h=124 lanes=32",
    "k_pc_agc<true, true> h=124 lanes=32", "k_pc_agc<true, true, PcWithProfiles> h=124 lanes=32",
    "k_pc_agc<true, false> h=16 lanes=32", "k_pc_agc<true, false, PcWithProfiles> h=16 lanes=32",
}


def test_the_cases_launch_every_instantiation(table):
    names = list(R.CASES)
    plans = PF.resolve(table, [PF.case_points(R.CASES[nm])[0] for nm in names])
    got, by_case = set(), {}
    for nm, plan in zip(names, plans):
        case = R.CASES[nm]
        tables = {R.has_table(case, b) for b in range(len(case.batches))}
        assert tables == {True, False}, f"{nm}: batches with and without the profile table"
        by_case[nm] = set().union(*(R.kernels(plan, t) for t in tables))
        got |= by_case[nm]
        print(nm, sorted(by_case[nm]))
    assert got == LAUNCHED, (sorted(got - LAUNCHED), sorted(LAUNCHED - got))
    # the forms the cases were chosen for
    assert "k_pc_gather" in by_case["1000-n248"] and "k_pc_submax" not in by_case["1000-n248"] and "k_pc_out" in by_case["16000-n248"]
    assert "k_pc_ma<true, true> lanes=32" in by_case["3200-n248"] and "k_pc_agc<true, false, PcWithProfiles> h=124 lanes=32" in by_case["3200-n248"]
    assert "k_pc_out4" in by_case["8000-n248-agc0"] and "k_pc_agc<true, true, PcWithProfiles> h=124 lanes=32" in by_case["8000-n248-pcm16"]
    assert "k_pc_gain<true, true, PcWithProfiles> lanes=32" in by_case["12000-n8"] and R.CASES["12000-n8"].max_batch > 192
    assert "k_pc_gain<true, false, PcWithProfiles> lanes=64" in by_case["12000-n360-2000"] & by_case["48000-n248-1600"]
    assert "k_pc_ma2<false> DIRECT lanes=64" in by_case["12000-n360-2000"] and "k_pc_mad<false> lanes=64" in by_case["48000-n248-1600"]


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_input_drives_the_chain(name, exe, tmp):
    case = R.CASES[name]
    ft, st = R.features(case), R.starts(case)
    run = R.oracle_run(name)
    present, al = R.present(name), R.alive(name)
    for k, (audio, pwr, dropped) in enumerate(run):
        assert np.array_equal(dropped[present[k]], ~al[k][present[k]]), f"client {k}: the oracle's NaN guard does not follow the script"
        assert not np.isnan(audio[~dropped]).any(), f"client {k}: a NaN in an unflagged row"
    sq = present[ft.squelch]
    opened = np.zeros(st[-1], bool)
    opened[sq] = R.squelch_flags(case, run[ft.squelch][1][sq])[0] == 1
    d = np.diff(opened[sq].astype(int))
    assert (d > 0).any() and (d < 0).any(), "the squelch model's flags hold no opening or no closing"
    keep = R.keep_mask(name, opened | ~sq)
    e = R.expected_pcm(name, [r[0] for r in run], keep, exe, tmp, "cover" + name)
    pcm = e.pcm
    assert e.uncapped and not R.cap_binds(e), f"the cap does not act for clients {R.cap_binds(e)} (largest gains {e.peak_gain})"
    nonzero = [int(np.count_nonzero(pcm[k])) for k in range(len(run))]
    in_last = [int(np.count_nonzero(pcm[k][int(keep[k][:st[-2]].sum()):])) for k in range(len(run))]
    print(f"{name}: non-zero expected PCM samples per client {nonzero}, in the last batch {in_last}")
    assert min(nonzero) >= 1000 and min(in_last) >= 1, (nonzero, in_last)
    for k, p in ft.profiles.items():   # the profile acts
        rows = np.ascontiguousarray(run[k][0][keep[k]])
        assert not np.array_equal(pcm[k], O.PostChain(case.rate).process(rows.reshape(-1)).reshape(rows.shape)), k


def noise(rate, seed=3):
    """noise whose level rises by 20 dB in the middle: the gain climbs, then falls; five look-aheads long"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(rate).astype(np.float32) * np.float32(1e-3)
    x[rate // 2:] *= np.float32(10)
    return x


@pytest.mark.parametrize("rate", sorted({c.rate for c in R.CASES.values()}))
def test_the_model_is_the_oracles_agc_at_the_cases_rates(exe, tmp, rate):
    x = noise(rate)
    ((y, g),) = M.model_runs(exe, tmp, [(x, [(x.size, 0, R.EXPRESSIBLE)])], rate=rate, look=rate // 5, tag=f"pin{rate}")
    want = M.oracle_agc(x, R.EXPRESSIBLE, rate=rate)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    assert not y[:rate // 5 - 1].any() and np.count_nonzero(y) > rate // 2
    d = np.diff(g[rate // 5 - 1:])
    assert (d > 0).any() and (d < 0).any(), "the gain did not both rise and fall"

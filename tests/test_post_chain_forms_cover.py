"""What tests/test_gpu_post_chain_forms.py covers, checked on the host (cases: tests/post_chain_forms.py).

1. Every case resolves - through the library's own pc_resolve, tests/post_plan_table.cpp built with the host compiler as
   tests/test_post_plan.py does - to the plan written beside it.
2. A sweep of rates, frame sizes, slot counts and AGC options with no knob set, every plan projected onto what decides which
   code runs (post_chain_forms.projection): every value of every component the sweep produces is produced by a GPU case -
   one of the new ones, or one of the points the older GPU files run (EXISTING).  Rates of 384 kHz and up (D >= 1024, where
   64 lanes fall back to MA_POW2) are outside the sweep: see post_chain_forms.py.
3. Each case's input, with the oracle's demodulator in the GPU's place: no frame flagged, the expected PCM of every client
   with at least 1000 non-zero samples and a non-zero sample in the last batch, streams as long as the rules ask."""
import numpy as np
import pytest

import post_chain_forms as PF
from oracle import oracle as O

# the (rate, n, max_batch, slots, AGC option) the GPU suite ran the chain at before test_gpu_post_chain_forms.py, by test
EXISTING = [
    ("test_gpu_parity.py::test_post_chain_bit_exact", [(12000, 248, 8, 4, 1), (12000, 248, 8, 4, 0), (192000, 248, 128, 4, 1), (12000, 252, 7, 4, 1),
                                                       (48000, 248, 33, 4, 1), (48000, 248, 33, 4, 0), (6000, 360, 9, 4, 1), (6000, 360, 9, 4, 0),
                                                       (44100, 248, 40, 4, 1)]),
    ("test_gpu_parity.py::test_post_chain_many_clients", [(12000, 360, 6, 70, 1), (12000, 360, 6, 600, 1)]),
    ("test_gpu_parity.py::test_post_chain_agc_forms_agree_under_churn", [(12000, 360, 7, 42, 1), (12000, 360, 7, 42, 0), (12000, 248, 5, 92, 1),
                                                                         (12000, 248, 5, 92, 0)]),
    ("test_gpu_post_chain_edges.py::test_post_chain_through_silence_bursts_and_saturation",
     [(12000, 360, 7, 3, 1), (12000, 360, 7, 3, 0), (12000, 252, 7, 3, 1), (44100, 248, 33, 3, 1), (48000, 248, 33, 3, 1), (48000, 248, 33, 3, 0),
      (192000, 248, 128, 3, 1)]),
]
SWEEP = [(rate, n, 16, slots, agc)
         for rate in (1000, 1500, 3200, 6000, 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 96000, 192000)
         for n in (8, 32, 128, 248, 252, 360) for slots in (4, 70, 600, 1600, 2000) for agc in (0, 1)]
# the rows the cases were made for, as (rate, n, slots, AGC option): none of them may leave the table
WANTED = [(1000, 248, 4, 1), (1500, 248, 4, 1), (3200, 248, 4, 1), (3200, 248, 4, 0), (8000, 248, 4, 1), (8000, 248, 4, 0), (8000, 248, 4, 2),
          (8000, 360, 4, 1), (16000, 248, 4, 1), (12000, 8, 4, 1), (12000, 32, 4, 1), (12000, 32, 4, 0), (48000, 248, 600, 1),
          (192000, 248, 600, 1), (12000, 360, 2000, 1), (48000, 248, 1600, 1)]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return PF.build_plan_table(tmp_path_factory.mktemp("post_chain_forms"))


@pytest.mark.parametrize("name", list(PF.CASES))
def test_case_resolves_to_its_plan(table, name):
    case = PF.CASES[name]
    for point, got in zip(PF.case_points(case), PF.resolve(table, PF.case_points(case))):
        want = dict(case.plan, verdict="OK")
        if case.agc == 2:  # both forms in turn: the option decides
            want["agc"] = PF.ONE if point[4] else PF.FIVE
        assert {k: got[k] for k in want} == {k: str(v) for k, v in want.items()}, (point, got)


def covered_by(points_by_name, plans):
    """{component: {value: [names]}}"""
    out, it = {}, iter(plans)
    for name, points in points_by_name:
        for _ in points:
            for comp, v in PF.projection(next(it)).items():
                out.setdefault(comp, {}).setdefault(v, []).append(name)
    return out


def uncovered(table, cases):
    """[(component, value, a sweep point that gives it)] of the sweep that neither `cases` nor EXISTING produce"""
    gpu = [("test_gpu_post_chain_forms.py[%s]" % name, PF.case_points(c)) for name, c in cases.items()]
    gpu += [(name, [(r, n, mb, s, a, 0) for r, n, mb, s, a in pts]) for name, pts in EXISTING]
    have = covered_by(gpu, PF.resolve(table, [p for _, pts in gpu for p in pts]))
    sweep = [(r, n, mb, s, a, 0) for r, n, mb, s, a in SWEEP]
    plans = PF.resolve(table, sweep)
    assert all(p["verdict"] == "OK" for p in plans)
    missing = {}
    for point, plan in zip(sweep, plans):
        for comp, v in PF.projection(plan).items():
            if v not in have.get(comp, {}):
                missing.setdefault((comp, v), point)
    return [(comp, v, point) for (comp, v), point in missing.items()], have


def test_the_gpu_cases_cover_every_form_of_the_sweep(table):
    missing, have = uncovered(table, PF.CASES)
    for comp, values in have.items():
        for v, names in sorted(values.items()):
            print(f"{comp}: {v}: {len(names)} GPU points, the first {names[0]}")
    assert not missing, "no GPU case runs (component, value, a (rate, n, max_batch, slots, AGC option, pcm16) that resolves to it): %s" % missing
    keys = {(c.rate, c.n, c.slots, c.agc) for c in PF.CASES.values()}
    assert not [w for w in WANTED if w not in keys], "cases that left the table"
    assert any(c.pcm16 and c.rate == 8000 for c in PF.CASES.values())


@pytest.mark.parametrize("name,lost", [("3200-n248", "MA_POW2"), ("12000-n360-2000", "MA2"), ("48000-n248-1600", "MAD"), ("1000-n248", "nsub"),
                                       ("12000-n8", "h < 16")])
def test_the_coverage_check_notices_a_missing_case(table, name, lost):
    """the check is not vacuous: without one of these cases, a form of the sweep is left without a GPU test"""
    missing, _ = uncovered(table, {k: c for k, c in PF.CASES.items() if k != name})
    assert any(lost in str(comp) + str(v) for comp, v, _ in missing), missing


@pytest.mark.parametrize("name", list(PF.CASES))
def test_case_input_drives_the_chain(name):
    case = PF.CASES[name]
    assert not PF.rules(case)
    n, h, total = case.n, case.n // 2, sum(case.batches)
    halves = O.convert(PF.raw_stream(case), "s16").view(np.complex64).reshape(total + 1, PF.N // 2)
    fo = O.FFT(PF.N, False, PF.LEVELS, 0, n)
    slots = PF.slots_of(case)
    clients, chains, nonzero, in_last = [], [], [0] * len(slots), [0] * len(slots)
    for k in range(len(slots)):
        mode, l, m, r = PF.client_spec(case, k)
        o = O.AudioClient(False, n, case.rate, PF.N)
        o.set_audio_demodulation(mode)
        o.set_audio_range(l, m, r)
        clients.append(o)
        chains.append(O.PostChain(case.rate))
    last_from = total - case.batches[-1]
    for f in range(total):
        fo.load(halves[f], halves[f + 1])
        fo.execute()
        spec = fo.output().copy()
        for k, slot in enumerate(slots):
            if f < PF.start_frame(case, slot):
                continue
            audio, _, _, dropped = clients[k].send_audio(spec, f, fft=fo, stats=False)
            assert not dropped and not np.isnan(audio).any(), f"client {k} frame {f} is flagged"
            c = int(np.count_nonzero(chains[k].process(audio)))
            nonzero[k] += c
            in_last[k] += c if f >= last_from else 0
    print(f"{name}: non-zero expected PCM samples per client {nonzero}, in the last batch {in_last}")
    assert min(nonzero) >= 1000 and min(in_last) >= 1, (nonzero, in_last)
    assert h * total >= case.rate // 5 + case.rate // 750 * 2 + 4 * h

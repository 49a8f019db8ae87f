"""k_audio_nb, k_audio_nr and k_audio_filter at frames of one block and longer (the cases: tests/audio_rows_shapes.py).

tests/test_gpu_audio_blanker.py's twin scheme: every client has a twin without the feature in the same context and batch, and
the expected rows are the host table programs' - anb_stream, nr_stream and af_stream, the text the kernels run - on the TWIN's
rows and NaN flags with the same batch lengths.  No tolerance anywhere: rows are compared as the bits of their words.  The host
programs are anchored at these frame lengths in tests/test_audio_rows_shapes_host.py.

Per n one 2^12-point IQ context and, per audio kind, five clients: the twin, the blanker alone (threshold 2, width 15), the noise
reduction alone, a two-section audio filter alone, and all three.  Batches of 1, 3, 2 and 4 frames; frames 5 and 6 are NaN."""
import functools

import numpy as np
import pytest

import anb_model as ANB
import audio_filter_model as AF
import audio_rows_shapes as S
import nr_model as NR
from conftest import ROOT
from helpers import assert_same_bits, read_client
from test_gpu_audio_blanker import AUDIO_KINDS, cat, expect, same_words
from test_gpu_squelch import Ctx, oracle_pcm

pytestmark = pytest.mark.gpu

ROLES = ("twin", "nb", "nr", "af", "all")
NAMES = ("pwr", "nan flags", "carrier level", "carrier offset")


def sections():
    from phantomsdr_amd import design_audio_filter as d
    return [d("highpass", S.RATE, 300.0), d("deemphasis", S.RATE, 212.0)]


def features(g, role, sec):
    if role in ("nb", "all"):
        g.set_audio_blanker("normal", *S.PARITY)
    if role in ("nr", "all"):
        g.set_noise_reduction("normal", *S.NRP)
    if role in ("af", "all"):
        g.set_audio_filter(sec)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_audio_rows_long")


@pytest.fixture(scope="module")
def progs(tmp):
    return ANB.build_table(tmp, ROOT), NR.build_table(tmp, ROOT), AF.build_table(tmp, ROOT)


@functools.lru_cache(maxsize=None)
def run(n):
    """-> {kind: {role: (rows [F][h], pwr, flags, ...)}}, {kind: {role: blanker totals}}"""
    sec = sections()
    A = Ctx(S.SHAPE, n, len(ROLES) * len(AUDIO_KINDS), maxb=S.MAX_BATCH, raw=S.raw_of(n))
    try:
        cl = {k: {} for k in AUDIO_KINDS}
        for k in AUDIO_KINDS:
            for role in ROLES:
                cl[k][role] = A.add(k)
                features(cl[k][role], role, sec)
        assert cl[AUDIO_KINDS[-1]]["all"].id == len(ROLES) * len(AUDIO_KINDS) - 1
        parts = {k: {r: [] for r in ROLES} for k in AUDIO_KINDS}
        for F in S.BATCHES:
            A.batch(F)
            for k in AUDIO_KINDS:
                for role in ROLES:
                    parts[k][role].append(read_client(cl[k][role], k, F))
        counts = {k: {r: cl[k][r].audio_blanker_counts() for r in ("nb", "all")} for k in AUDIO_KINDS}
        return {k: {r: cat(v) for r, v in p.items()} for k, p in parts.items()}, counts
    finally:
        A.close()


def hosts(progs, tmp, n, res):
    """per kind what the three host programs give on the twin's rows and flags: (blanked, blanker state, trace), reduced,
    filtered, and the chain blanked -> reduced -> filtered"""
    anb, nr, af = progs
    h, sizes, sec = n // 2, list(S.BATCHES), sections()
    tw = [res[k]["twin"] for k in AUDIO_KINDS]
    blanked = expect(lambda jobs: ANB.run_streams(anb, tmp, jobs), [S.PARITY + (t[0], t[2], sizes) for t in tw])
    reduced = NR.run_streams(nr, tmp, [S.NRP + (t[0].reshape(-1), t[2], h, sizes) for t in tw], rate=S.RATE)
    filtered = AF.run_blocked(af, tmp, [(sec, t[0].reshape(-1), t[2], h, sizes) for t in tw])
    chain_nr = NR.run_streams(nr, tmp, [S.NRP + (b[0].reshape(-1), t[2], h, sizes) for b, t in zip(blanked, tw)], "chain", rate=S.RATE)
    chain_af = AF.run_blocked(af, tmp, [(sec, c[0], t[2], h, sizes) for c, t in zip(chain_nr, tw)], "chain")
    shape = tw[0][0].shape
    return {k: dict(nb=blanked[i], nr=reduced[i][0].reshape(shape), af=filtered[i][0].reshape(shape), all=chain_af[i][0].reshape(shape))
            for i, k in enumerate(AUDIO_KINDS)}


@pytest.mark.parametrize("n", S.LONG_N)
def test_rows_and_totals_are_the_host_programs_at_long_frames(progs, tmp, n):
    res, counts = run(n)
    h, sizes = n // 2, S.BATCHES
    want = hosts(progs, tmp, n, res)
    for k in AUDIO_KINDS:
        twin = res[k]["twin"]
        flagged = twin[2] != 0
        assert flagged[S.NAN_HALF - 1] and flagged[S.NAN_HALF] and not flagged[:S.NAN_HALF - 1].any() and not flagged.all(), (k, flagged)
        blanked, st, tr = want[k]["nb"]
        # the host program's run is worth comparing against (conditions on the input: chosen on the CPU for S.CPU_KINDS)
        broken = S.stream_rules(h, sizes, tr)
        print(f"n {n} {k}: flagged frames {np.flatnonzero(flagged).tolist()} centres {len(tr['centres'])} unusable blocks {S.unusable_blocks(tr)} {broken}")
        S.record("gpu_long", n=n, h=h, kind=k, batches=list(sizes), slots=len(ROLES) * len(AUDIO_KINDS), centres=len(tr["centres"]),
                 unusable_blocks=S.unusable_blocks(tr), rules_broken=broken)
        if k in S.CPU_KINDS:
            assert not broken, (n, k, broken)
        assert len(tr["centres"]) >= 8, (n, k)
        if h == 1200:
            assert S.unusable_blocks(tr) > 4, "the flagged frames blank more than a group of four blocks"
        for role in ROLES[1:]:
            got = res[k][role]
            assert_same_bits(got[1:], twin[1:], f"n {n} {k} {role}: pwr, flags, carrier records", NAMES)
            assert got[0][flagged].tobytes() == twin[0][flagged].tobytes(), (n, k, role, "a flagged frame's row was touched")
        same_words(res[k]["nb"][0], blanked, (n, k, "anb_stream"))
        same_words(res[k]["nr"][0], want[k]["nr"], (n, k, "nr_stream"))
        same_words(res[k]["af"][0], want[k]["af"], (n, k, "af_stream"))
        same_words(res[k]["all"][0], want[k]["all"], (n, k, "anb_stream, nr_stream, then af_stream"))
        assert not np.array_equal(res[k]["nb"][0][~flagged], twin[0][~flagged]) and not np.array_equal(res[k]["nr"][0][~flagged], twin[0][~flagged])
        total = (int(st["impulses"]), int(st["samples"]))
        assert counts[k]["nb"] == total and counts[k]["all"] == total and total[0] == len(tr["centres"]), (n, k, counts[k], total)


def test_the_chain_at_h_1200_in_front_of_the_post_chain(progs, tmp):
    """tests/test_gpu_audio_blanker.py's test_the_chain_blanker_noise_reduction_audio_filter_post_chain at n = 2400"""
    n = 2400
    anb, nr, af = progs
    sizes, sec = list(S.BATCHES), sections()
    A = Ctx(S.SHAPE, n, 2, maxb=S.MAX_BATCH, post=True, raw=S.raw_of(n))
    try:
        allc, tw = A.add("AM"), A.add("AM")
        features(allc, "all", sec)
        parts = ([], [])
        for F in sizes:
            A.batch(F)
            parts[0].append(read_client(allc, "AM", F, pcm=True)), parts[1].append(read_client(tw, "AM", F, pcm=True))
    finally:
        A.close()
    got, twin = cat(parts[0]), cat(parts[1])
    ((blanked, _, tr),) = expect(lambda jobs: ANB.run_streams(anb, tmp, jobs), [S.PARITY + (twin[0], twin[2], sizes)])
    assert len(tr["centres"]) >= 8
    ((reduced, _, _),) = NR.run_streams(nr, tmp, [S.NRP + (blanked.reshape(-1), twin[2], n // 2, sizes)], rate=S.RATE)
    (filtered, _), = AF.run_blocked(af, tmp, [(sec, reduced, twin[2], n // 2, sizes)])
    filtered = filtered.reshape(got[0].shape)
    same_words(got[0], filtered, ("anb_stream, nr_stream, then af_stream", n))
    keep = twin[2] == 0
    assert keep.any() and not keep.all()
    want = oracle_pcm(np.where(keep[:, None], filtered, 0), keep, n // 2)
    assert np.count_nonzero(want) > 1000, "the chain was not exercised"
    assert np.array_equal(got[3], want), "the PCM is the oracle's chain over the processed rows"

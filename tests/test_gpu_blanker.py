"""The wideband impulse blanker on the ingest ring (include/psdr.h: psdr_ring_set_blanker) on the GPU, bit for bit against
tests/nb_model.py.  Shapes: the smallest the library accepts - IQ at N = 2^12 (2048 samples, 8 blocks per half) in all six
formats, real at N = 2^13 (4096 samples, 16 blocks) in s16 and f32; a ring of 8 halves, max_batch 4, 24 halves of stream, so
the ring wraps twice and the slot-0 half is blanked through its mirror once per turn.  tests/test_blanker_host.py shows that
the model blanks every planted impulse of these streams with its full guard and nothing else: both sides cannot be idle."""
import numpy as np
import pytest

import nb_model as M
from nb_rig import Rig, run_blanked, run_plain, same

pytestmark = pytest.mark.gpu

CASES = [(f, False) for f in ("u8", "s8", "u16", "s16", "f32", "f64")] + [("s16", True), ("f32", True)]
IDS = ["%s-%s" % (f, "real" if r else "iq") for f, r in CASES]
GUARDS = [0, 7, 255]


@pytest.mark.parametrize("guard", GUARDS)
@pytest.mark.parametrize("fmt,is_real", CASES, ids=IDS)
def test_ring_counts_levels_and_spectra_under_both_splits(fmt, is_real, guard):
    """assertions 1 - 3: the ring's bytes, the counts and R_H are the model's under 4+4+.. and under 1+3+2+2+..; the spectra
    and pyramids of every frame are those of a twin with the blanker off that was fed the model-blanked stream"""
    fa, model_a, ca = run_blanked(fmt, is_real, guard, M.SPLIT_A)
    fb, model_b, cb = run_blanked(fmt, is_real, guard, M.SPLIT_B)
    assert ca == cb and len(ca) == M.STREAM_HALVES and sum(ca.values()) > 0
    assert all(same(a, b) for a, b in zip(model_a, model_b))
    twin = run_plain(fmt, is_real, model_a, M.SPLIT_A)
    assert sorted(fa) == sorted(fb) == sorted(twin) == list(range(M.STREAM_HALVES - 1))
    for f in twin:
        assert same(fa[f][0], twin[f][0]) and same(fa[f][1], twin[f][1]), f
        assert same(fb[f][0], twin[f][0]) and same(fb[f][1], twin[f][1]), f


@pytest.mark.parametrize("fmt,is_real", [("s16", False), ("f32", True)], ids=["s16-iq", "f32-real"])
def test_a_jump_in_first_half_restarts_the_reference(fmt, is_real):
    """assertion 5: halves 5..11 are never read; half 12 (with an impulse) takes its threshold from its own level"""
    frames, model, counts = run_blanked(fmt, is_real, 7, M.JUMP)
    assert sorted(counts) == list(range(0, 5)) + list(range(12, 21)) and counts[12] == 15
    twin = run_plain(fmt, is_real, model, M.JUMP)
    assert all(same(frames[f][0], twin[f][0]) and same(frames[f][1], twin[f][1]) for f in twin)


@pytest.mark.parametrize("fmt,is_real", [("s16", False), ("f64", False), ("f32", True)], ids=["s16-iq", "f64-iq", "f32-real"])
def test_ninety_db_on_the_noise_blanks_nothing(fmt, is_real):
    """assertion 6"""
    halves, _ = M.fixture(fmt, is_real, 0, planted=False)
    _, model, counts = run_blanked(fmt, is_real, 255, M.SPLIT_A, db=90.0, planted=False)
    assert set(counts.values()) == {0} and all(same(a, b) for a, b in zip(model, halves))


@pytest.mark.parametrize("fmt,is_real", [("s16", False), ("f32", True)], ids=["s16-iq", "f32-real"])
def test_off_on_and_off_again(fmt, is_real):
    """assertion 4: off leaves the ring as written; switched off mid-stream, later halves are untouched; switched on again, the
    first half uses its own R.  The model is switched with the context."""
    guard = 7
    halves, _ = M.fixture(fmt, is_real, guard)
    model = [h.copy() for h in halves]
    rig = Rig(fmt, is_real)
    try:
        def step(first, n, nb):
            want = nb.process(model, first, n) if nb else {}
            rig.call(halves, first, n)
            for h in range(first, first + n + 1):
                assert same(rig.ring_half(h), model[h]), h
                got = rig.ctx.ring_read_blanker(h)
                assert (got is None) if h not in want else (got[0] == want[h][0] and same(got[1], want[h][1])), (h, got)
            return want

        assert step(0, 2, None) == {} and same(rig.ring_half(2), halves[2])  # never switched on: half 2's impulse stays
        assert not any(rig.blanker_ptrs())
        rig.ctx.ring_set_blanker(True, M.THRESHOLD_DB, guard)
        assert all(rig.blanker_ptrs())
        nb = M.Blanker(fmt, is_real, M.THRESHOLD_DB, guard)
        # halves 0..2 were read with the blanker off: switching on starts at the call's first half, so they are blanked now
        w = step(2, 2, nb)
        assert sorted(w) == [2, 3, 4] and w[2][0] == 8 and w[3][0] == 8
        rig.ctx.ring_set_blanker(False)
        assert step(4, 3, None) == {} and same(rig.ring_half(5), halves[5]) and same(rig.ring_half(6), halves[6])
        rig.ctx.ring_set_blanker(True, M.THRESHOLD_DB, guard)
        nb = M.Blanker(fmt, is_real, M.THRESHOLD_DB, guard)  # afresh: half 8 (slot 0, an impulse) from its own level
        w = step(8, 2, nb)
        assert sorted(w) == [8, 9, 10] and w[8][0] == 15
        assert same(rig.mirror(), model[8])
        # a refused call changes nothing: the next halves are blanked with the old setting
        from phantomsdr_amd._lib import PsdrError
        for args in ((True, 90.5, 0), (True, float("nan"), 0), (True, 10.0, 256), (True, -1.0, 3)):
            with pytest.raises(PsdrError) as e:
                rig.ctx.ring_set_blanker(*args)
            assert e.value.code == -1
        w = step(10, 3, nb)
        assert sorted(w) == [11, 12, 13] and w[12][0] == 15
    finally:
        rig.close()


def test_a_silent_half_in_front_of_a_loud_one():
    """assertion 7: digital silence gives R = 0 and T = 0 for the next half, in which nothing is blanked - and the half behind
    that takes the loud half's level again"""
    fmt, is_real, guard = "s16", False, 7
    halves, _ = M.fixture(fmt, is_real, guard)
    halves[1][:] = 0
    model, nb = [h.copy() for h in halves], M.Blanker(fmt, is_real, M.THRESHOLD_DB, guard)
    rig = Rig(fmt, is_real)
    try:
        rig.ctx.ring_set_blanker(True, M.THRESHOLD_DB, guard)
        want = nb.process(model, 0, 4)
        rig.call(halves, 0, 4)
        got = {h: rig.ctx.ring_read_blanker(h) for h in range(5)}
        assert got[1] == (0, np.float32(0.0)) and got[2][0] == 0 and got[3][0] == 8  # half 2's impulse stays, half 3's goes
        for h in range(5):
            assert got[h][0] == want[h][0] and same(got[h][1], want[h][1]) and same(rig.ring_half(h), model[h])
        assert same(rig.ring_half(2), halves[2])
    finally:
        rig.close()


def test_without_a_ring_and_the_python_methods():
    from phantomsdr_amd import Context
    from phantomsdr_amd._lib import PsdrError
    ctx = Context(1 << 12, False, 3, input_format="s16", max_batch=2, max_clients=1)
    try:
        for fn in (lambda: ctx.ring_set_blanker(True, 10.0, 3), lambda: ctx.ring_read_blanker(0), lambda: ctx.ring_read(0)):
            with pytest.raises(PsdrError) as e:
                fn()
            assert e.value.code == -4  # PSDR_ERR_STATE
        ctx.ring_create(4)
        ctx.ring_set_blanker(False, float("nan"), -7)  # on = 0 ignores both
        assert ctx.ring_read_blanker(0) is None
        assert ctx.ring_read(0, np.int16).shape == (2 * 2048,)
    finally:
        ctx.close()

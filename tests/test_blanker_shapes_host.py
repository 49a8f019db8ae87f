"""The streams of tests/test_gpu_blanker_shapes.py ask what they claim - shown on tests/nb_model.py alone, without a GPU.  The
model blanks exactly what is planted, with the full clipped guard, and nothing else (no stream's lowered threshold admits a
noise sample: each count is the planted one); a quiet block alone decides R of its half; the dense calls and the large calls
exceed the caps of the sparse kernels' and the streaming kernel's grids, stated here for 256 compute units (the GPU file
asserts them again with the device's own count); and the host program of tests/test_blanker_host.py (blankerplan.h's text, the
kernels' own) finds the model's block maxima on one half of every stream."""
import numpy as np
import pytest

import nb_model as M
from test_blanker_host import bits, build, fields, run

CUS = 256
LIST_CAP, TILE_CAP = 2 * CUS, 16 * CUS  # the grids of k_nb_mark / k_nb_zero and of k_nb_block_max (blanker.hip)
A_CASES = [(f, True) for f in ("u8", "s8", "u16", "f64")]  # (a): the formats tests/test_gpu_blanker.py leaves out
B_GUARDS = [255, 0]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("blanker_shapes"), "blanker_plan_table")


def check_exact(st, calls, db, guard, whole=(), untouched=()):
    """the model zeroes the planted impulses' guards - every sample of a half in `whole`, none of one in `untouched` - and
    changes no other byte; -> {half: count}"""
    model, seen = M.run_model(st, calls, db, guard)
    assert sorted(seen) == list(range(len(st.halves)))
    imps = st.kinds("imp", "inf")
    for h, (count, R) in seen.items():
        want = M.expected_hits(st.hs, imps, h, guard)
        if h in whole:
            want[:] = True
        if h in untouched:
            want[:] = False
        assert count == int(want.sum()), (h, count, int(want.sum()))
        exp = st.halves[h].copy().reshape(st.hs, -1)
        exp[want] = M.zero_code(st.fmt)
        assert np.array_equal(exp.reshape(-1).view(np.uint8), model[h].view(np.uint8)), h
    return {h: c for h, (c, _) in seen.items()}


def check_quiet(st, calls, db, guard):
    """R of a quiet half is its quiet block's maximum, strictly below every other block's; the threshold made of it is lower
    than that of a plain half and still valid"""
    _, seen = M.run_model(st, calls, db, guard)
    quiet = st.kinds("quiet")
    assert quiet
    plain = min(R for h, (_, R) in seen.items() if h not in {q[0] for q in quiet})
    for h, blk, _ in quiet:
        bm = st.bmax(h)
        assert bits(seen[h][1]) == bits(bm[blk]) and 0 < bm[blk] < np.delete(bm, blk).min(), (h, blk)
        assert bm[blk] < plain and M.threshold(M.factor(db), bm[blk]) > 0


def check_program(exe, st_fmt, is_real, raw):
    """the host program's chunk maxima, folded per block, are the model's block maxima of the half `raw`"""
    words = raw.view(np.uint32).reshape(-1, 4)
    head = "chunk %d %d " % (M.FMT_ID[st_fmt], int(is_real))
    out = run(exe, "".join(head + "%d %d %d %d\n" % tuple(w) for w in words.tolist()), timeout=300).splitlines()
    assert len(out) == len(words)
    mx = np.array([int(fields(ln)["max"]) for ln in out], np.uint32).view(np.float32)
    cpb = M.BLOCK * raw.itemsize * (1 if is_real else 2) // 16
    want = M.block_maxima(M.power(raw, st_fmt, is_real))
    assert np.array_equal(mx.reshape(-1, cpb).max(axis=1).view(np.uint32), want.view(np.uint32))
    return want


# ---- (a) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,is_real", A_CASES)
@pytest.mark.parametrize("guard", [0, 7, 255])
def test_a_fixture_in_the_real_formats_blanks_what_is_planted(fmt, is_real, guard):
    hs = M.shape(is_real) // 2
    halves, pl = M.fixture(fmt, is_real, guard)
    raw = [h.copy() for h in halves]
    nb, seen = M.Blanker(fmt, is_real, M.THRESHOLD_DB, guard), {}
    for first, n in M.SPLIT_A:
        seen.update(nb.process(halves, first, n))
    assert len(seen) == M.STREAM_HALVES and sum(c for c, _ in seen.values()) > 0
    for h, (count, R) in seen.items():
        want = M.expected_hits(hs, pl, h, guard)
        exp = raw[h].copy().reshape(hs, -1)
        exp[want] = M.zero_code(fmt)
        assert count == int(want.sum()) and R > 0 and np.isfinite(R), (h, count)
        assert np.array_equal(exp.reshape(-1).view(np.uint8), halves[h].view(np.uint8)), h


@pytest.mark.parametrize("fmt,is_real", A_CASES)
def test_a_program_finds_the_block_maxima(exe, fmt, is_real):
    halves, _ = M.fixture(fmt, is_real, 7)
    bm = check_program(exe, fmt, is_real, halves[5])  # impulses at samples 255 and 256
    assert bm[0] > 100 * np.delete(bm, [0, 1]).max() and bm[1] == bm[0]


# ---- (b) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,is_real,N", M.B_SHAPES)
def test_b_streams(exe, fmt, is_real, N):
    st = M.stream_b(fmt, is_real, N)
    db = M.stream_db(fmt)
    assert (st.nblocks, st.cpb) == {"s16": (128, 64), "u8": (256, 16)}[fmt] and st.sb == (4 if fmt == "s16" else 1)
    a, b = st.split(8), st.split(1, 7, 3, 5)
    assert a == [(0, 8), (8, 8), (16, 8), (24, 8)] and b[:5] == [(0, 1), (1, 7), (8, 3), (11, 5), (16, 1)] and len(st.halves) == 33
    assert sum(n for _, n in a) == sum(n for _, n in b) == 32
    # quiet blocks where a shortened k_nb_ref loop would miss them: 64 exactly, 127 and the last one
    assert sorted({q[1] for q in st.kinds("quiet")}) == sorted({64, 127, st.nblocks - 1}) and st.nblocks > 64
    check_quiet(st, a, db, 0)
    for guard in B_GUARDS:
        counts = check_exact(st, a, db, guard)
        assert M.run_model(st, b, db, guard)[1] == M.run_model(st, a, db, guard)[1]  # any split, the same counts and levels
        for h in M.B_DENSE:
            # every second block, sample 0 and sample 255 of a block, two adjacent blocks; the odd blocks keep R at the noise
            offs = {s % M.BLOCK for hh, s, _ in st.kinds("imp") if hh == h}
            blks = {s // M.BLOCK for hh, s, _ in st.kinds("imp") if hh == h}
            assert {0, 255} <= offs and set(range(0, st.nblocks, 2)) <= blks and {4, 5, 6} <= blks
            assert st.bmax(h).min() < 4 * st.bmax(1).min()
            assert counts[h] == st.nblocks // 2 + 1 if guard == 0 else counts[h] > 20000, (h, counts[h])  # tens of thousands of samples a half
        assert all(counts[h] > 0 for h in (3, 5, 7, 19, 21, 16, 24, 32))  # behind the quiet halves; slot 0; a call's last half
    # the caps: the calls (8, 8) and (24, 8) list more blocks than k_nb_mark / k_nb_zero have work-groups, all blocks of their dense halves
    listed = st.listed(a, db)
    assert listed[1] > LIST_CAP and listed[3] > LIST_CAP, listed
    assert listed[1] >= 7 * st.nblocks and listed[3] >= 5 * st.nblocks
    if fmt == "s16":  # k_nb_list: 9 new halves of 128 blocks are four and a half work-groups (with 256 blocks a half every one is full)
        assert 9 * st.nblocks > 256 and 9 * st.nblocks % 256 == 128
    check_program(exe, fmt, is_real, st.halves[9])


# ---- (c) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(M.C_SHAPES)), ids=["%s-%s" % (f, "real" if r else "iq") for f, r, _ in M.C_SHAPES])
def test_c_streams(exe, k):
    fmt, is_real, N = M.C_SHAPES[k]
    st, db, guard = M.stream_c(fmt, is_real, N), M.stream_db(fmt), M.C_GUARD[k]
    assert st.hb == 2 << 20 and st.tiles == 512 and st.cpb == [256, 128, 64, 16][k] and len(st.halves) == 28
    # the caps: every call has more tiles than k_nb_block_max has work-groups
    new = [10, 9, 9]
    assert all(n * st.tiles > TILE_CAP for n in new)
    # quiet blocks and impulses in tiles of the second stride: tile index within the call >= the cap
    first_new = [0, 10, 19]
    for h, blk, _ in st.kinds("quiet"):
        c = max(i for i in range(3) if first_new[i] <= h)
        tile = (h - first_new[c]) * st.tiles + blk * M.BLOCK * st.sb // 4096
        assert TILE_CAP <= tile < new[c] * st.tiles, (h, blk, tile)
    assert {9, 18, 27} <= {h for h, _, _ in st.kinds("imp")}  # each call's last half (second stride), 18 in slot 0
    check_quiet(st, M.C_CALLS, db, guard)
    counts = check_exact(st, M.C_CALLS, db, guard)
    assert all(counts[h] > 0 for h in (4, 9, 10, 18, 19, 27))
    check_program(exe, fmt, is_real, st.halves[9])


# ---- (d) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,is_real,N", M.D_SHAPES)
def test_d_thresholds_that_blank_nothing(exe, fmt, is_real, N):
    st = M.stream_d(fmt, is_real, N)
    kf = M.factor(M.THRESHOLD_DB)
    for guard in (0, 7):
        # half 5 is zeroed whole by the plain threshold in front of it; the impulses of halves 6 and 13 stay
        counts = check_exact(st, M.SPLIT_A, M.THRESHOLD_DB, guard, whole=(5,), untouched=(6, 13))
        assert counts[5] == st.hs and counts[6] == counts[13] == 0 and counts[7] > 0 and counts[14] > 0
    _, seen = M.run_model(st, M.SPLIT_A, M.THRESHOLD_DB, 7)
    R5, R12 = seen[5][1], seen[12][1]
    assert np.isfinite(R5) and R5 > 1e37 and np.isposinf(M.threshold(kf, R5))  # kf * R overflows
    assert bits(R12) == 0 and bits(M.threshold(kf, R12)) == 0  # the all-NaN block: M_b = +0.0
    assert np.isnan(st.halves[12].reshape(st.hs, -1)[3 * M.BLOCK:4 * M.BLOCK]).all() and st.bmax(12)[3] == 0 and np.delete(st.bmax(12), 3).min() > 0
    assert np.isfinite(seen[6][1]) and 0 < seen[6][1] < 1 and 0 < seen[13][1] < 1  # ... and the halves behind are blanked from a finite level
    check_program(exe, fmt, is_real, st.halves[5])
    check_program(exe, fmt, is_real, st.halves[12])


# ---- (e) -----------------------------------------------------------------------------------------------------------------------
def test_e_stream(exe):
    st = M.stream_e()
    calls = st.split(8)
    assert calls == [(f, 8) for f in range(0, 48, 8)] and len(st.halves) == 49 and st.nhalves == 16 and st.hb == 2 << 20
    counts = check_exact(st, calls, M.THRESHOLD_DB, 7)
    t = 4096 // st.sb
    for h in (0, 16, 32, 48, 8, 24, 40):  # slot 0; the last half of a call
        assert counts[h] == 8 + 16 + 8  # the half's first and last sample clipped, two neighbours across a tile's edge
        assert {0, 3 * t - 1, 3 * t, st.hs - 1} == {s for hh, s, _ in st.plants if hh == h}
    check_program(exe, st.fmt, st.is_real, st.halves[16])

"""The ingest-ring blanker (include/psdr.h: psdr_ring_set_blanker) on the GPU beyond the smallest shapes, byte for byte against
tests/nb_model.py: the ring bytes of every half a call read, the count and level of every new half (None for the others), the
mirror whenever a half sits in slot 0.  tests/test_blanker_shapes_host.py shows on the model alone that these streams ask what
is claimed here; the two caps that depend on the device are asserted again below with its own count of compute units.
  (a) real u8, s8, u16, f64 at 2^13: 16 lanes a block (one byte a sample), one-byte stores, the real f64 decode
  (b) IQ 2^16 s16 (128 blocks a half), real 2^17 u8 (256): k_nb_ref's lane + 64 loop, k_nb_list over several work-groups, work
      lists longer than the grids of k_nb_mark / k_nb_zero, counts of tens of thousands from many waves
  (c) 2 MiB halves, 10 or 9 new ones a call: k_nb_block_max's grid-stride loop, for 256, 128, 64 and 16 chunks a block
  (d) kf * R = +Inf and R = 0 from a block of NaN: nothing is blanked behind either
  (e) slots rewritten as soon as the call that read them is issued, without a host wait in between"""
import numpy as np
import pytest

import nb_model as M
from nb_rig import Rig, run_blanked, run_plain, same

pytestmark = pytest.mark.gpu

A_CASES = [(f, True) for f in ("u8", "s8", "u16", "f64")]
GUARDS = [0, 7, 255]


def ids(cases):
    return ["%s-%s" % (c[0], "real" if c[1] else "iq") for c in cases]


def compute_units():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def frames_equal(got, twin):
    return sorted(got) == sorted(twin) and all(same(got[f][0], twin[f][0]) and same(got[f][1], twin[f][1]) for f in twin)


@pytest.mark.parametrize("guard", GUARDS)
@pytest.mark.parametrize("fmt,is_real", A_CASES, ids=ids(A_CASES))
def test_a_real_formats_under_both_splits(fmt, is_real, guard):
    """the procedure of test_gpu_blanker.py::test_ring_counts_levels_and_spectra_under_both_splits, its parameter list completed"""
    fa, model_a, ca = run_blanked(fmt, is_real, guard, M.SPLIT_A)
    fb, model_b, cb = run_blanked(fmt, is_real, guard, M.SPLIT_B)
    assert ca == cb and len(ca) == M.STREAM_HALVES and sum(ca.values()) > 0
    assert all(same(a, b) for a, b in zip(model_a, model_b))
    twin = run_plain(fmt, is_real, model_a, M.SPLIT_A)
    assert sorted(fa) == sorted(fb) == sorted(twin) == list(range(M.STREAM_HALVES - 1))
    for f in twin:
        assert same(fa[f][0], twin[f][0]) and same(fa[f][1], twin[f][1]), f
        assert same(fb[f][0], twin[f][0]) and same(fb[f][1], twin[f][1]), f


@pytest.mark.parametrize("guard", [255, 0])
@pytest.mark.parametrize("fmt,is_real,N", M.B_SHAPES, ids=ids(M.B_SHAPES))
def test_b_many_blocks_and_long_work_lists(fmt, is_real, N, guard):
    """quiet blocks at 64, 127 and nblocks - 1; dense halves whose every block is listed; 8+8+8+8 and 1+7+3+5+.. over a ring of 16
    halves that wraps twice; every frame against the twin"""
    st, db = M.stream_b(fmt, is_real, N), M.stream_db(fmt)
    a, b = st.split(8), st.split(1, 7, 3, 5)
    listed, cap = st.listed(a, db), 2 * compute_units()
    assert listed[1] > cap and listed[3] > cap, (listed, cap)  # more listed blocks than k_nb_mark / k_nb_zero have work-groups
    fa, model_a, ca = run_blanked(fmt, is_real, guard, a, db=db, st=st)
    fb, model_b, cb = run_blanked(fmt, is_real, guard, b, db=db, st=st)
    assert ca == cb and len(ca) == len(st.halves) and all(same(x, y) for x, y in zip(model_a, model_b))
    assert min(ca[h] for h in M.B_DENSE) > (20000 if guard else 64)
    twin = run_plain(fmt, is_real, model_a, a, st=st)
    assert sorted(twin) == list(range(len(st.halves) - 1)) and frames_equal(fa, twin) and frames_equal(fb, twin)


@pytest.mark.parametrize("k", range(len(M.C_SHAPES)), ids=ids(M.C_SHAPES))
def test_c_streaming_kernel_past_one_grid_of_tiles(k):
    """three calls of 9 frames on 2 MiB halves; quiet blocks and impulses in tiles the second stride of k_nb_block_max takes; the
    spectrum and pyramid of frame 8 (half 9: an impulse of the second stride) and of frame 17 (the ring's wrap) against the twin"""
    fmt, is_real, N = M.C_SHAPES[k]
    st, db, guard = M.stream_c(fmt, is_real, N), M.stream_db(fmt), M.C_GUARD[k]
    cap = 16 * compute_units()
    assert all(n * st.tiles > cap for n in (10, 9, 9)), (st.tiles, cap)  # more tiles than k_nb_block_max has work-groups
    first_new = [0, 10, 19]
    for h, blk, _ in st.kinds("quiet"):
        c = max(i for i in range(3) if first_new[i] <= h)
        assert (h - first_new[c]) * st.tiles + blk * M.BLOCK * st.sb // 4096 >= cap, (h, blk, cap)
    keep = {8, 17}
    frames, model, counts = run_blanked(fmt, is_real, guard, M.C_CALLS, db=db, st=st, keep=keep)
    assert sorted(counts) == list(range(28)) and all(counts[h] > 0 for h in (9, 10, 18, 19, 27))
    twin = run_plain(fmt, is_real, model, M.C_CALLS[:2], st=st, keep=keep)
    assert sorted(twin) == [8, 17] and frames_equal(frames, twin)


@pytest.mark.parametrize("guard", [0, 7])
@pytest.mark.parametrize("fmt,is_real,N", M.D_SHAPES, ids=ids(M.D_SHAPES))
def test_d_thresholds_that_blank_nothing(fmt, is_real, N, guard):
    """half 5 near 7e18 throughout: kf * R_5 = +Inf, so the impulse of half 6 stays and that of half 7 goes; half 12 with a block
    of nothing but NaN: R_12 = 0, so the impulse of half 13 stays, that of half 14 goes, and the NaN bytes are unchanged"""
    st = M.stream_d(fmt, is_real, N)
    for calls in (M.SPLIT_A, M.SPLIT_B):
        _, model, counts = run_blanked(fmt, is_real, guard, calls, st=st)
        assert counts[5] == st.hs and counts[6] == counts[13] == counts[12] == 0 and counts[7] > 0 and counts[14] > 0
        assert same(model[6], st.halves[6]) and same(model[13], st.halves[13]) and same(model[12], st.halves[12])


def test_e_slots_rewritten_without_a_host_wait():
    """psdr.h: "A slot may be rewritten as soon as the psdr_process_ring() call that read it has been issued".  The blanker stores
    into the slots a call reads; behind every process_ring the eight slots no later call reads are overwritten at once, each
    half from a pinned buffer of its own.  Counts, levels and the first, middle and last frame of every call are those of the
    run that waits on the host in front of every write; the ring holds the model's bytes at the end."""
    fmt, is_real, _ = M.E_SHAPE
    st, guard, db = M.stream_e(), 7, M.THRESHOLD_DB
    calls = st.split(8)
    keep = {first + f for first, _ in calls for f in (0, 4, 7)}
    waited, model, counts = run_blanked(fmt, is_real, guard, calls, db=db, st=st, keep=keep)
    _, seen = M.run_model(st, calls, db, guard)
    assert sorted(waited) == sorted(keep) and {h: c for h, (c, _) in seen.items()} == counts  # the waiting run is the model's
    nh, last = st.nhalves, len(st.halves) - 1
    rig = Rig(fmt, is_real, st)
    try:
        src = [rig.ctx.pinned_array(rig.hb) for _ in st.halves]  # no source is reused: only the ring's slots are
        for h, buf in enumerate(src):
            buf[:] = st.halves[h].view(np.uint8)
        rig.ctx.ring_set_blanker(True, db, guard)
        for h in range(nh):  # (half 16 would overwrite half 0 unread: it is the first write behind the first call)
            rig.ctx.ring_write_async(h, src[h])
        frames, got = {}, {}
        for first, n in calls:
            rig.ctx.process_ring(first, n)
            for h in range(first + nh, min(first + nh + n, last + 1)):  # the slots of halves first .. first + n - 1
                rig.ctx.ring_write_async(h, src[h])
            for h in range(first + 1 if first else 0, first + n + 1):
                got[h] = rig.ctx.ring_read_blanker(h)
            frames.update(rig.read_frames(first, n, keep))
        for h in range(last + 1):
            assert got[h] is not None and got[h][0] == seen[h][0] and same(got[h][1], seen[h][1]), (h, got[h], seen[h])
        assert frames_equal(frames, waited)
        for h in range(last + 1 - nh, last + 1):
            assert same(rig.ring_half(h), model[h]), h
        assert last % nh == 0 and same(rig.mirror(), model[last])
    finally:
        rig.close()

"""Waterfall detectors without a GPU: the ABI additions (include/psdr.h, libpsdr_hip.so, the ctypes binding) and the
numpy model of the contract (tests/wf_detector_model.py) on hand-made arrays."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

import wf_detector_model as M


def _header():
    return open(os.path.join(ROOT, "include", "psdr.h")).read()


def test_library_exports_the_detector_entry_point_and_keeps_the_abi_number():
    lib = ctypes.CDLL(os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so"))
    assert hasattr(lib, "psdr_waterfall_set_detector")
    lib.psdr_abi_version.restype = ctypes.c_int
    assert lib.psdr_abi_version() == 3
    # (no device needed: the argument check comes first)
    lib.psdr_waterfall_set_detector.restype = ctypes.c_int
    lib.psdr_waterfall_set_detector.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert lib.psdr_waterfall_set_detector(None, 0, 1) == -1


def test_header_declares_the_detectors():
    h = _header()
    assert re.search(r"#define\s+PSDR_ABI_VERSION\s+3\b", h)
    assert re.search(r"int\s+psdr_waterfall_set_detector\s*\(\s*psdr_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", h)
    for name, val in (("PSDR_WF_SAMPLE", 0), ("PSDR_WF_PEAK", 1), ("PSDR_WF_MEAN", 2)):
        assert re.search(rf"\b{name}\s*=\s*{val}\b", h), name
    assert re.search(r"#define\s+PSDR_OPT_WATERFALL_DETECTOR\s+4\b", h)
    # the earlier options keep their numbers
    for name, val in (("PSDR_OPT_POST_CHAIN_STREAMS", 1), ("PSDR_OPT_POST_CHAIN_AGC", 2), ("PSDR_OPT_POST_CHAIN_PCM16", 3)):
        assert re.search(rf"\b{name}\s*=\s*{val}\b", h), name


def test_python_binding_knows_the_detectors():
    from phantomsdr_amd import _lib, core
    assert any(name == "psdr_waterfall_set_detector" for name, _, _ in _lib.SYMBOLS)
    assert core.WF_DETECTORS == {"sample": 0, "peak": 1, "mean": 2}
    assert core.Context.OPT_WATERFALL_DETECTOR == 4
    assert callable(core.WaterfallClient.set_detector)


def test_fanout_params_gain_the_detector_as_last_member():
    src = open(os.path.join(ROOT, "phantomsdr_amd", "host", "hip_fanout.h")).read()
    body = src[src.index("struct Params {"):]
    body = body[:body.index("\n    };")]
    members = [ln.strip() for ln in body.splitlines() if ln.strip() and not ln.strip().startswith("//")]
    assert members[-1].startswith("int waterfall_detector = PSDR_WF_SAMPLE;")


# ---- the model ---------------------------------------------------------------------------------------------------

def _rows(*cols):
    return np.array(cols, np.int8).T.copy()      # each argument: one output index over the frames


def test_model_mean_rounds_half_up_also_below_zero():
    assert M.reduce_window(_rows([-1, 0]), M.MEAN).tolist() == [0]          # -0.5 -> 0
    assert M.reduce_window(_rows([-2, -1]), M.MEAN).tolist() == [-1]        # -1.5 -> -1
    assert M.reduce_window(_rows([1, 2]), M.MEAN).tolist() == [2]           # 1.5 -> 2
    assert M.reduce_window(_rows([-128, -128, -127]), M.MEAN).tolist() == [-128]   # -127.67 -> -128
    assert M.reduce_window(_rows([127, 127], [-128, -128]), M.MEAN).tolist() == [127, -128]
    assert M.reduce_window(_rows([-3, -3, -2]), M.MEAN).tolist() == [-3]    # -2.67 -> -3


def test_model_peak_is_signed():
    assert M.reduce_window(_rows([-128, -1, -5], [3, -128, 127]), M.PEAK).tolist() == [-1, 127]


def test_model_one_frame_windows_equal_sample():
    rows = np.arange(-6, 6, dtype=np.int8).reshape(6, 2)
    for det in (M.SAMPLE, M.PEAK, M.MEAN):
        got = M.expected_rows(rows, [(0, 6)], 1, det)
        assert np.array_equal(got[0], rows)
    assert M.reduce_window(_rows([-7]), M.MEAN).tolist() == [-7]


def test_model_windows_runs_and_splits():
    rows = np.array([[10], [-20], [30], [-40], [50], [-60], [70], [-80]], np.int8)   # frames 0..7
    # skip 3: sent 0, 3, 6; frame 0 stands for itself
    pk = M.expected_rows(rows, [(0, 8)], 3, M.PEAK)[0]
    assert pk.ravel().tolist() == [10, 30, 70]
    mn = M.expected_rows(rows, [(0, 8)], 3, M.MEAN)[0]
    assert mn.ravel().tolist() == [10, -10, 20]           # (-20+30-40)/3 = -10; (50-60+70)/3 = 20
    sa = M.expected_rows(rows, [(0, 8)], 3, M.SAMPLE)[0]
    assert sa.ravel().tolist() == [10, -40, 70]
    # the same frames in other batches: the same rows, wherever the cut falls
    for calls in ([(0, 4), (4, 4)], [(k, 1) for k in range(8)], [(0, 1), (1, 1), (2, 5), (7, 1)]):
        got = M.expected_rows(rows, calls, 3, M.PEAK)
        assert np.concatenate(got).ravel().tolist() == [10, 30, 70]
        assert [g.shape[0] for g in got] == [sum(1 for t in range(f, f + n) if t % 3 == 0) for f, n in calls]
    # first_frame_num not a multiple of skip_num: frames 4..11, sent 6, 9; the first row has only the run's 3 frames
    got = M.expected_rows(rows, [(4, 8)], 3, M.PEAK)[0]
    assert got.ravel().tolist() == [30, 50]               # max(10,-20,30), max(-40,50,-60)
    # a window across three calls (skip 8 > batches of 3): frames 1..8, sent 8
    got = M.expected_rows(rows, [(1, 3), (4, 3), (7, 2)], 8, M.MEAN)
    assert [g.shape[0] for g in got] == [0, 0, 1]
    assert got[2].ravel().tolist() == [-5]                # sum = -40, n = 8


def test_model_gap_and_repeat_start_a_new_run():
    rows = np.array([[100], [1], [2], [3], [4], [5]], np.int8)
    # frames 1, 2 | gap | 5, 6, 7, 8 with skip 4: row of frame 8 covers 5..8 = all of the new run, not frame 1 (100)
    got = M.expected_rows(rows, [(1, 2), (5, 4)], 4, M.PEAK)
    assert got[1].ravel().tolist() == [5]
    # continued instead: frames 1, 2 | 3, 4, 5, 6 -> sent 4 covers 1..4
    got = M.expected_rows(rows, [(1, 2), (3, 4)], 4, M.PEAK)
    assert got[1].ravel().tolist() == [100]
    # a repeated first_frame_num starts over: the second call's row of frame 4 sees only its own frames 3, 4
    got = M.expected_rows(np.array([[100], [1], [2], [3]], np.int8), [(3, 2), (3, 2)], 4, M.PEAK)
    assert got[0].ravel().tolist() == [100] and got[1].ravel().tolist() == [3]
    # no client with a detector at the first call: its frames are not kept
    got = M.expected_rows(rows, [(1, 2), (3, 4)], 4, M.PEAK, holding=[False, True])
    assert got[1].ravel().tolist() == [3]

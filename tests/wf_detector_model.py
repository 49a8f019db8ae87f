"""Pure-numpy model of the waterfall detectors' contract (include/psdr.h: psdr_wf_detector, psdr_waterfall_batch).

    rows   int8 [T][len]: one client's values q_t[j] of every processed frame, in processing order (frame k of the
           i-th call is row sum(nframes of the calls before) + k)
    calls  [(first_frame_num, nframes), ...]: the psdr_waterfall_batch calls, one per processed batch
    ->     one int8 array [nsent][len] per call: the rows that call gathers

A sent frame s (s % skip_num == 0) stands for the frames t of the current run with s - skip_num < t <= s.  A call
continues the run when its first_frame_num is the previous call's first_frame_num + nframes; any other call starts a new
run.  `holding` (optional, one bool per call): whether an active client had a detector at that call - the library keeps
the run's history only while one has, so a call after one without starts a new run too.

It keeps every frame of the run and slices the window out for each sent frame: nothing of the library's carry /
in-batch split is repeated here.
"""
import numpy as np

SAMPLE, PEAK, MEAN = 0, 1, 2


def reduce_window(w, detector):
    """w: int8 [n][len], the frames of one window, the sent frame last"""
    w = np.asarray(w, np.int8)
    if detector == SAMPLE:
        return w[-1].copy()
    if detector == PEAK:
        return w.max(axis=0)
    assert detector == MEAN
    n = w.shape[0]
    s = w.astype(np.int64).sum(axis=0)
    return ((2 * s + n) // (2 * n)).astype(np.int8)      # floor division: round half up


def expected_rows(rows, calls, skip_num, detector, holding=None):
    rows = np.asarray(rows, np.int8)
    out, run, nxt, pos, prev_hold = [], [], None, 0, False
    for i, (first, nf) in enumerate(calls):
        hold = True if holding is None else bool(holding[i])
        if nxt is None or first != nxt or not (hold and prev_hold):
            run = []                                      # (frame number, row) of the run so far
        got = []
        for k in range(nf):
            t = first + k
            run.append((t, rows[pos + k]))
            if t % skip_num == 0:
                got.append(reduce_window(np.stack([r for (u, r) in run if t - skip_num < u <= t]), detector))
                run = []                                  # the next window starts behind the sent frame
        out.append(np.stack(got) if got else np.zeros((0, rows.shape[1]), np.int8))
        pos += nf
        nxt, prev_hold = first + nf, hold
    assert pos == rows.shape[0], "the calls do not cover the rows"
    return out

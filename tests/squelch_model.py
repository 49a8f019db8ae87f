"""The squelch rule of include/psdr.h (psdr_client_set_squelch) as a model, written from the header's words: what
tests/test_squelch_host.py holds the shared step function against and tests/test_gpu_squelch.py the kernel."""
import numpy as np


def threshold(db):
    """T = (float)pow(10, db / 10): computed in double, rounded once"""
    return np.float32(10.0 ** (db / 10))


def run(pwr, t_open, t_close, attack, hang, state=(0, 0)):
    """frames' flags [len(pwr)] (int32) and the state behind them; pwr, t_open, t_close are f32; state = (open, cnt)"""
    is_open, cnt = state
    t_open, t_close = np.float32(t_open), np.float32(t_close)
    flags = np.zeros(len(pwr), np.int32)
    for f, p in enumerate(np.asarray(pwr, np.float32)):
        if not is_open:
            cnt = cnt + 1 if p >= t_open else 0  # (NaN: false - it never opens)
            if cnt >= attack:
                is_open, cnt = 1, 0
        else:
            cnt = cnt + 1 if not (p >= t_close) else 0  # (NaN: it counts as below)
            if cnt > hang:
                is_open, cnt = 0, 0
        flags[f] = is_open  # AFTER the update
    return flags, (is_open, cnt)


def events(pwr, flags, t_open, t_close, attack, hang):
    """which of the five events a flag sequence holds - a condition on a test's INPUT, not on the code:
    opening, closing, a gap shorter than the hang (bridged), a burst shorter than the attack (rejected), a NaN frame"""
    pwr = np.asarray(pwr, np.float32)
    ge_o, ge_c = pwr >= np.float32(t_open), pwr >= np.float32(t_close)
    n = len(flags)
    ev = set()
    for f in range(n):
        prev = flags[f - 1] if f else 0
        if flags[f] and not prev:
            ev.add("opening")
        if prev and not flags[f]:
            ev.add("closing")
        if np.isnan(pwr[f]):
            ev.add("nan")
    f = 0
    while f < n:
        # a run of frames below T_close that begins and ends inside an open stretch: bridged by the hang
        if f and flags[f - 1] and flags[f] and not ge_c[f]:
            g = f
            while g < n and not ge_c[g]:
                g += 1
            if g < n and all(flags[f:g + 1]) and g - f <= hang:
                ev.add("bridged")
            f = g
        # a run of frames at or above T_open shorter than the attack that leaves the client closed: rejected
        elif not flags[f] and ge_o[f] and (f == 0 or not ge_o[f - 1]):
            g = f
            while g < n and ge_o[g]:
                g += 1
            if g < n and g - f < attack and not any(flags[f:g + 1]):
                ev.add("rejected")
            f = g
        else:
            f += 1
    return ev

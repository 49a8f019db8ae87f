"""Builds and runs tests/forward_plan_table.cpp - the forward path's planners (phantomsdr_amd/csrc/forwardplan.h) behind a
script - for the tests that need to know what the library plans: tests/test_forward_plan.py holds the planners to their rules,
tests/test_real_fused_model.py and tests/test_gpu_bench_shapes.py take the chain segments of the fused real second pass from
here.  The header is plain C++17: the program is built with the host compiler and needs neither a GPU nor the library."""
import functools
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

_TMP = []


def build(directory, name="forward_plan_table", extra=()):
    exe = os.path.join(str(directory), name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(ROOT, "phantomsdr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "forward_plan_table.cpp"), "-o", exe])
    return exe


@functools.lru_cache(maxsize=1)
def program():
    _TMP.append(tempfile.TemporaryDirectory(prefix="forward_plan_"))  # (removed when the interpreter exits)
    return build(_TMP[-1].name)


def run(exe, text, timeout=300):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def fields(ln):
    return dict(kv.split("=", 1) for kv in ln.split()[1:])


def tables(out):
    """the `segtab` blocks of an output: [(fields, table [count][5] = frame, first tile, tiles, segment above, carry-in through memory)]"""
    lines = out.splitlines()
    res = []
    for i, ln in enumerate(lines):
        if ln.startswith("segtab "):
            assert lines[i + 1].startswith("T")
            f = fields(ln)
            tab = np.array(lines[i + 1].split()[1:], dtype=np.int64).reshape(-1, 5)
            assert len(tab) == int(f["count"])
            res.append((f, tab))
    return res


@functools.lru_cache(maxsize=None)
def seg_plan(G, nframes, num_cus=256, seg_len_env=0):
    """The chain segments the library plans for a batch of nframes frames of G tiles.  Returns (table, handoff, nseam): table[sg] =
    (frame, first tile, tiles, segment above, carry-in through memory); nseam: the segments without a carry-in."""
    (f, tab), = tables(run(program(), "segtab %d %d %d %d\n" % (G, num_cus, seg_len_env, nframes)))
    rows = [(int(a), int(b), int(c), int(d), bool(e)) for a, b, c, d, e in tab]
    return rows, f["handoff"] == "1", sum(1 for t in rows if not t[4])

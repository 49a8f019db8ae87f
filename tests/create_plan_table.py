"""Builds and runs tests/create_plan_table.cpp - the create-time planners (phantomsdr_amd/csrc/createplan.h) behind a script -
for the tests that need to know what psdr_create plans: tests/test_create_plan.py holds the planners to their rules,
tests/test_forward_plan.py and tests/test_gpu_family_plans.py ask for the shape of a config and the plan of an audio size, and
tests/test_gpu_create_plan.py holds the library's answers against them.  The header is plain C++17: the program is built with
the host compiler and needs neither a GPU nor the library."""
import functools
import os
import subprocess
import tempfile

from conftest import ROOT

_TMP = []


def build(directory, name="create_plan_table", extra=()):
    exe = os.path.join(str(directory), name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(ROOT, "phantomsdr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "create_plan_table.cpp"), "-o", exe])
    return exe


@functools.lru_cache(maxsize=1)
def program():
    _TMP.append(tempfile.TemporaryDirectory(prefix="create_plan_"))  # (removed when the interpreter exits)
    return build(_TMP[-1].name)


def run(exe, text, timeout=300):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def fields(ln):
    """{key: text} of a line; `msg`, always last, is the rest of the line"""
    head, sep, msg = ln.partition(" msg=")
    d = dict(kv.split("=", 1) for kv in head.split()[1:])
    if sep:
        d["msg"] = msg
    return d


def env(split=0, three_pass=0, seg_len=0, log2m2=0, cus=256):
    return "env %d %d %d %d %d" % (split, three_pass, seg_len, log2m2, cus)


def cfg(N, is_real, levels=1, brightness=0, additional=0, audio=0, rate=12000, fmt=3, batch=1, clients=1, wf_clients=1, skip=1, wf_size=0):
    return "cfg %d %d %d %d %d %d %d %d %d %d %d %d %d" % (N, is_real, levels, brightness, additional, audio, rate, fmt, batch, clients, wf_clients, skip, wf_size)


def blocks(out):
    """the output of a script cut at its `check` lines: [{first word: [fields of each such line]}]"""
    res = []
    for ln in out.splitlines():
        if ln.startswith("S"):
            continue
        if ln.startswith("check "):
            res.append({})
        res[-1].setdefault(ln.split()[0], []).append(fields(ln))
    return res


@functools.lru_cache(maxsize=None)
def plan(N, is_real, **kw):
    """the lines of one accepted config under the default environment: {first word: fields}"""
    (b,) = blocks(run(program(), env() + "\n" + cfg(N, is_real, **kw) + "\n"))
    assert b["check"][0]["code"] == "0", b
    return {k: v[0] for k, v in b.items()}


@functools.lru_cache(maxsize=None)
def idft(n):
    """(radices, kernel) of an audio size: kernel is fixed / wave / lds0 / lds1 / lds2 (the work-group kernel by lds_mode), none for n = 0"""
    f = fields(run(program(), "idft %d 0\n" % n))
    assert f["code"] == "0", f
    kind = {"fixed360": "fixed", "fixed720": "fixed", "lds": "lds" + f["lds_mode"]}.get(f["kind"], f["kind"])
    return tuple(int(r) for r in f["radix"].split(",") if r), kind

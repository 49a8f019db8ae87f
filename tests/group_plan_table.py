"""Builds and runs tests/group_plan_table.cpp - the multi-GPU group's planner (phantomsdr_amd/csrc/groupplan.h) behind a script -
for tests/test_group_plan.py.  The header is plain C++17: the program is built with the host compiler and needs neither a GPU
nor the library."""
import functools
import os
import subprocess
import tempfile

from conftest import ROOT

_TMP = []


def build(directory, name="group_plan_table", extra=()):
    exe = os.path.join(str(directory), name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(ROOT, "phantomsdr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "group_plan_table.cpp"), "-o", exe])
    return exe


@functools.lru_cache(maxsize=1)
def program():
    _TMP.append(tempfile.TemporaryDirectory(prefix="group_plan_"))  # (removed when the interpreter exits)
    return build(_TMP[-1].name)


def run(exe, text, timeout=300):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def fields(ln):
    return dict(kv.split("=", 1) for kv in ln.split()[1:] if "=" in kv)

"""Notch filters without a GPU: the ABI additions (include/psdr.h, libpsdr_hip.so, the ctypes binding), the interval rounding of
psdr_client_set_notch through the library's debug entry psdr_debug_notch_interval (exported beside psdr_debug_trace, not in the header), and what the built library's code objects say about the
kernels that now carry the notch test."""
import ctypes
import inspect
import math
import os
import re

import pytest

from conftest import ROOT

import codeobj


def _lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so"))
    lib.psdr_debug_notch_interval.restype = ctypes.c_int
    lib.psdr_debug_notch_interval.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    return lib


def test_header_declares_the_calls_and_keeps_the_abi_number():
    h = open(os.path.join(ROOT, "include", "psdr.h")).read()
    assert re.search(r"#define\s+PSDR_ABI_VERSION\s+3\b", h)
    assert re.search(r"#define\s+PSDR_NOTCH_MANUAL\s+2\b", h) and re.search(r"#define\s+PSDR_NOTCH_AUTO\s+2\b", h)
    assert re.search(r"#define\s+PSDR_OPT_AUTO_NOTCH\s+7\b", h)
    assert re.search(r"int\s+psdr_client_set_notch\s*\(\s*psdr_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*\)\s*;", h)
    assert re.search(r"int\s+psdr_client_set_auto_notch\s*\(\s*psdr_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", h)
    assert re.search(r"int\s+psdr_read_notches\s*\(\s*psdr_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*int\s+first\[4\]\s*,\s*int\s+end\[4\]\s*\)\s*;", h)


# (centre, width) -> [first, end): floor(centre - width/2 + 0.5), floor(centre + width/2 + 0.5), at least one bin; width <= 0 clears
ROUNDING = [
    ((100.0, 3.0), (99, 102)), ((100.0, 1.0), (100, 101)), ((100.0, 2.0), (99, 101)), ((100.5, 2.0), (100, 102)),
    ((100.0, 0.25), (100, 101)),     # narrower than a bin: end <= first -> one bin
    ((100.49, 0.01), (100, 101)), ((100.5, 0.01), (100, 101)),
    ((0.0, 4.0), (-2, 2)),           # straddling bin 0: floor, not truncation
    ((-0.75, 1.0), (-1, 0)), ((7.25, 4.5), (5, 10)), ((1e6 + 0.5, 360.0), (999821, 1000181)),
    ((100.0, 0.0), (0, 0)), ((100.0, -3.0), (0, 0)),
]


@pytest.mark.parametrize("args,want", ROUNDING)
def test_interval_rounding(args, want):
    lib = _lib()
    first, end = ctypes.c_int(-7), ctypes.c_int(-7)
    assert lib.psdr_debug_notch_interval(args[0], args[1], ctypes.byref(first), ctypes.byref(end)) == 0
    assert (first.value, end.value) == want
    c, w = args
    if w > 0:
        a, b = math.floor(c - w / 2 + 0.5), math.floor(c + w / 2 + 0.5)
        assert want == (a, b if b > a else a + 1)


def test_non_finite_arguments_and_null_contexts_are_rejected():
    lib = _lib()
    first, end = ctypes.c_int(5), ctypes.c_int(6)
    for c, w in ((float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0), (1.0, float("-inf"))):
        assert lib.psdr_debug_notch_interval(c, w, ctypes.byref(first), ctypes.byref(end)) == -1
        assert (first.value, end.value) == (5, 6)
    lib.psdr_client_set_notch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double]
    assert lib.psdr_client_set_notch(None, 0, 0, 1.0, 1.0) == -1
    assert lib.psdr_client_set_auto_notch(None, 0, 1) == -1
    assert lib.psdr_read_notches(None, 0, None, None) == -1


def test_python_wrappers():
    from phantomsdr_amd import _lib as L, core
    bound = {name for name, _, _ in L.SYMBOLS}
    assert {"psdr_client_set_notch", "psdr_client_set_auto_notch", "psdr_read_notches"} <= bound
    assert core.Context.OPT_AUTO_NOTCH == 7
    assert list(inspect.signature(core.AudioClient.set_notch).parameters) == ["self", "index", "centre_bin", "width_bins"]
    assert list(inspect.signature(core.AudioClient.set_auto_notch).parameters) == ["self", "on"]
    assert list(inspect.signature(core.AudioClient.notches).parameters) == ["self"]


needs_lib = pytest.mark.skipif(not (os.path.exists(codeobj.SO) and os.path.exists(codeobj.READELF)),
                               reason="needs the built library and llvm-readelf")

# VGPRs of the parent commit: no instantiation that carries the notch test may use more, none may use scratch
PARENT_VGPR = {
    "psdr::k_demod_chain_fixed<360": 77, "psdr::k_demod_chain_fixed<720": 125, "psdr::k_demod_chain_iq<360": 62,
    "psdr::k_demod_chain_iq<720": 113, "psdr::k_demod_chain_sam<360": 87, "psdr::k_demod_chain_sam<720": 128,
    "psdr::k_demod_chain_ft<360": 69, "psdr::k_demod_chain_ft<720": 115, "psdr::k_demod_chain_sbsam<360": 83,
    "psdr::k_demod_chain_sbsam<720": 128, "psdr::k_demod_idft_fixed<360": 44, "psdr::k_demod_idft_fixed<720": 88,
}


@needs_lib
def test_no_kernel_pays_registers_for_the_notch_test():
    meta = codeobj.kernel_metadata()
    for prefix, vgpr in PARENT_VGPR.items():
        hits = {k: v for k, v in meta.items() if k.startswith(prefix)}
        assert hits, prefix
        for k, v in hits.items():
            assert v["vgpr"] <= vgpr and v["scratch"] == 0, (k, v, vgpr)
    twins = {k: v for k, v in meta.items() if k.startswith("psdr::k_demod_chain_iq_nz<")}
    assert len(twins) == 2
    for k, v in twins.items():
        assert v["scratch"] == 0 and v["vgpr"] <= (80 if "<360" in k else 128), (k, v)
    det = {k: v for k, v in meta.items() if k.startswith("psdr::k_notch_detect")}
    assert len(det) == 1 and all(v["scratch"] == 0 for v in det.values())

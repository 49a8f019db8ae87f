"""Fine tuning below one FFT bin without a GPU: the ABI additions (include/psdr.h, libpsdr_hip.so, the ctypes binding) and
what the built library's code objects say about the new chain kernel and its neighbours."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

import codeobj


def _header():
    return open(os.path.join(ROOT, "include", "psdr.h")).read()


def test_header_declares_the_flag_and_the_option():
    h = _header()
    assert re.search(r"#define\s+PSDR_ABI_VERSION\s+3\b", h)
    assert re.search(r"int\s+psdr_client_set_fine_tune\s*\(\s*psdr_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", h)
    assert re.search(r"#define\s+PSDR_OPT_FINE_TUNE\s+5\b", h)
    assert re.search(r"#define\s+PSDR_OPT_WATERFALL_DETECTOR\s+4\b", h)   # the earlier option keeps its number


def test_library_exports_the_entry_point_and_keeps_the_abi_number():
    lib = ctypes.CDLL(os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so"))
    assert hasattr(lib, "psdr_client_set_fine_tune")
    lib.psdr_abi_version.restype = ctypes.c_int
    assert lib.psdr_abi_version() == 3
    # (no device needed: the argument check comes first)
    lib.psdr_client_set_fine_tune.restype = ctypes.c_int
    lib.psdr_client_set_fine_tune.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert lib.psdr_client_set_fine_tune(None, 0, 1) == -1


def test_python_binding_knows_the_flag():
    from phantomsdr_amd import _lib, core
    assert any(name == "psdr_client_set_fine_tune" for name, _, _ in _lib.SYMBOLS)
    assert core.Context.OPT_FINE_TUNE == 5
    assert callable(core.AudioClient.set_fine_tune)


needs_lib = pytest.mark.skipif(not (os.path.exists(codeobj.SO) and os.path.exists(codeobj.READELF)),
                               reason="needs the built library and llvm-readelf")


@pytest.fixture(scope="module")
def meta():
    return codeobj.kernel_metadata()


@needs_lib
def test_tuned_chain_kernel_fits_beside_a_pass(meta):
    """k_demod_chain_ft takes the wave slots of k_demod_chain_iq: exactly the two compile-time plans for each of the two
    families (USB / LSB, IQ), no scratch, no accumulator registers, at most the 128 registers beside a pass - and at
    n = 360 the 96 of five waves per SIMD (the launch bounds; DESIGN.md 3.9 records the seat reached)"""
    hits = {k: v for k, v in meta.items() if k.startswith("psdr::k_demod_chain_ft<")}
    want = {f"psdr::k_demod_chain_ft<{plan}, {ssb}>" for plan in ("360, 8, 9, 5", "720, 8, 9, 10") for ssb in ("true", "false")}
    assert {k.split("(")[0] for k in hits} == want
    for k, v in hits.items():
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["vgpr"] <= 128, (k, v)
        if k.startswith("psdr::k_demod_chain_ft<360"):
            assert v["vgpr"] <= 96, (k, v)


@needs_lib
def test_existing_chain_kernels_keep_their_budgets(meta):
    """the budgets test_code_objects.py states, with the new kernels in the same translation unit"""
    def find(prefix):
        hits = {k: v for k, v in meta.items() if k.startswith(prefix)}
        assert hits, prefix
        return hits.items()
    for name in ("psdr::k_demod_chain_fixed<", "psdr::k_demod_chain_iq<", "psdr::k_demod_chain_sam<"):
        for k, v in find(name):
            assert v["vgpr"] <= 128 and v["scratch"] == 0, (k, v)
    for name in ("psdr::k_demod_chain_fixed<360", "psdr::k_demod_chain_iq<360"):
        for k, v in find(name):
            assert v["vgpr"] <= 80, (k, v)
    assert len(list(find("psdr::k_demod_chain_fixed<"))) == len(list(find("psdr::k_demod_chain_iq<"))) == len(list(find("psdr::k_demod_chain_sam<"))) == 2
    for k, v in find("psdr::k_col_tail<"):
        assert v["vgpr"] <= 96 and v["scratch"] == 0, (k, v)

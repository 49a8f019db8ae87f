"""Selectable-sideband synchronous AM without a GPU: the ABI additions (include/psdr.h, libpsdr_hip.so, the ctypes binding)
and what the built library's code objects say about the two new kernels and their neighbours."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

import codeobj


def _header():
    return open(os.path.join(ROOT, "include", "psdr.h")).read()


def test_header_declares_the_enum_the_call_and_the_option():
    h = _header()
    assert re.search(r"#define\s+PSDR_ABI_VERSION\s+3\b", h)
    assert re.search(r"typedef\s+enum\s+psdr_sam_sideband\s*\{\s*PSDR_SAM_BOTH\s*=\s*0\s*,\s*PSDR_SAM_UPPER\s*=\s*1\s*,\s*PSDR_SAM_LOWER\s*=\s*2\s*\}"
                     r"\s*psdr_sam_sideband\s*;", h)
    assert re.search(r"int\s+psdr_client_set_sam_sideband\s*\(\s*psdr_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", h)
    assert re.search(r"#define\s+PSDR_OPT_SAM_SIDEBAND\s+6\b", h)
    assert re.search(r"#define\s+PSDR_OPT_FINE_TUNE\s+5\b", h)  # the earlier option keeps its number
    assert re.search(r"\bPSDR_SAM\s*=\s*5\b", h)  # ... and the sideband is no mode: SAM stays the last one


def test_library_exports_the_entry_point_and_keeps_the_abi_number():
    lib = ctypes.CDLL(os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so"))
    assert hasattr(lib, "psdr_client_set_sam_sideband")
    lib.psdr_abi_version.restype = ctypes.c_int
    assert lib.psdr_abi_version() == 3
    # (no device needed: the argument check comes first)
    lib.psdr_client_set_sam_sideband.restype = ctypes.c_int
    lib.psdr_client_set_sam_sideband.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert lib.psdr_client_set_sam_sideband(None, 0, 1) == -1


def test_python_binding_knows_the_sidebands():
    import phantomsdr_amd
    from phantomsdr_amd import _lib, core
    assert any(name == "psdr_client_set_sam_sideband" for name, _, _ in _lib.SYMBOLS)
    assert (core.SAM_BOTH, core.SAM_UPPER, core.SAM_LOWER) == (0, 1, 2)
    assert core.SAM_SIDEBANDS == {"both": 0, "upper": 1, "lower": 2}
    assert (phantomsdr_amd.SAM_BOTH, phantomsdr_amd.SAM_UPPER, phantomsdr_amd.SAM_LOWER) == (0, 1, 2)
    assert phantomsdr_amd.SAM_SIDEBANDS is core.SAM_SIDEBANDS
    assert core.Context.OPT_SAM_SIDEBAND == 6
    assert callable(core.AudioClient.set_sam_sideband)


needs_lib = pytest.mark.skipif(not (os.path.exists(codeobj.SO) and os.path.exists(codeobj.READELF)),
                               reason="needs the built library and llvm-readelf")


@pytest.fixture(scope="module")
def meta():
    return codeobj.kernel_metadata()


def _find(meta, prefix):
    return {k: v for k, v in meta.items() if k.startswith(prefix)}


@needs_lib
def test_sideband_chain_kernel_takes_its_siblings_seat(meta):
    """k_demod_chain_sbsam: exactly the two compile-time plans, no scratch, no accumulator registers, the registers of
    k_demod_chain_sam's launch bounds - at most 96 at n = 360 (five waves per SIMD), at most 128 at 720 (four); the kernel
    behind the IDFT without scratch"""
    hits = _find(meta, "psdr::k_demod_chain_sbsam<")
    assert {k.split("(")[0] for k in hits} == {"psdr::k_demod_chain_sbsam<360, 8, 9, 5>", "psdr::k_demod_chain_sbsam<720, 8, 9, 10>"}
    for k, v in hits.items():
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["wg"] == 256, (k, v)
        assert v["vgpr"] <= (96 if k.startswith("psdr::k_demod_chain_sbsam<360") else 128), (k, v)
    ola = _find(meta, "psdr::k_demod_ola_sbsam")
    assert len(ola) == 1
    for k, v in ola.items():
        assert v["scratch"] == 0, (k, v)
    # ... and its names start with none of the existing families' prefixes: those are as many as before, within their budgets
    for name, count in (("psdr::k_demod_chain_sam<", 2), ("psdr::k_demod_chain_iq<", 2), ("psdr::k_demod_chain_fixed<", 2),
                        ("psdr::k_demod_chain_ft<", 4)):
        hits = _find(meta, name)
        assert len(hits) == count, (name, sorted(hits))
        for k, v in hits.items():
            assert v["scratch"] == 0 and v["agpr"] == 0 and v["vgpr"] <= 128, (k, v)
            if k.startswith(name + "360"):
                assert v["vgpr"] <= (80 if name in ("psdr::k_demod_chain_fixed<", "psdr::k_demod_chain_iq<") else 96), (k, v)
    assert len(_find(meta, "psdr::k_demod_ola_sam")) == 1

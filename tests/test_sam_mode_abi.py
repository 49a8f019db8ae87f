"""Synchronous AM client mode without a GPU: the ABI additions (include/psdr.h, libpsdr_hip.so, the ctypes binding) and what
the built library's code objects say about the SAM chain kernel."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

import codeobj


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psdr.h")).read(), flags=re.S)


def test_header_declares_the_mode_and_the_calls_and_keeps_the_abi_number():
    h = _header()
    assert re.search(r"#define\s+PSDR_ABI_VERSION\s+3\b", h)
    assert re.search(r"\bPSDR_SAM\s*=\s*5\b", h)
    for name, val in (("PSDR_USB", 0), ("PSDR_LSB", 1), ("PSDR_AM", 2), ("PSDR_FM", 3), ("PSDR_IQ", 4)):  # the earlier modes keep their numbers
        assert re.search(rf"\b{name}\s*=\s*{val}\b", h), name
    assert re.search(r"int\s+psdr_read_carrier\s*\(\s*psdr_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*float\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,"
                     r"\s*int\s*\*\s*\w+\s*\)\s*;", h)
    assert re.search(r"int\s+psdr_fetched_carrier\s*\(\s*psdr_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*float\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)\s*;", h)


def test_library_exports_the_carrier_entry_points_and_keeps_the_abi_number():
    lib = ctypes.CDLL(os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so"))
    for name in ("psdr_read_carrier", "psdr_fetched_carrier"):
        assert hasattr(lib, name), name
    lib.psdr_abi_version.restype = ctypes.c_int
    assert lib.psdr_abi_version() == 3
    # (no device needed: the argument check comes first)
    lib.psdr_read_carrier.restype = ctypes.c_int
    lib.psdr_read_carrier.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    assert lib.psdr_read_carrier(None, 0, 1, None, None, None) == -1
    lib.psdr_fetched_carrier.restype = ctypes.c_int
    lib.psdr_fetched_carrier.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.psdr_fetched_carrier(None, 0, 0, None, None) == -1


def test_python_binding_knows_the_mode():
    from phantomsdr_amd import _lib, core
    import phantomsdr_amd
    assert core.SAM == 5 and core.MODES["SAM"] == 5 and phantomsdr_amd.SAM == 5
    assert {k: core.MODES[k] for k in ("USB", "LSB", "AM", "FM", "IQ")} == {"USB": 0, "LSB": 1, "AM": 2, "FM": 3, "IQ": 4}
    bound = {name for name, _, _ in _lib.SYMBOLS}
    assert {"psdr_read_carrier", "psdr_fetched_carrier"} <= bound
    assert callable(core.AudioClient.read_carrier) and callable(core.Context.fetched_carrier)


needs_code_objects = pytest.mark.skipif(not (os.path.exists(codeobj.SO) and os.path.exists(codeobj.READELF)),
                                        reason="needs the built library and llvm-readelf")


@pytest.fixture(scope="module")
def meta():
    return codeobj.kernel_metadata()


def _find(meta, prefix):
    hits = {k: v for k, v in meta.items() if k.startswith(prefix)}
    assert hits, f"no kernel {prefix}* in the library"
    return hits


@needs_code_objects
def test_sam_chain_kernel_has_no_scratch_and_keeps_its_launch_bounds(meta):
    """k_demod_chain_sam for n = 360 and 720: no scratch, no AGPRs, and the registers its launch bounds promise - five waves
    per SIMD at n = 360 (at most 96 VGPRs), four at 720 (at most 128), the seats of k_demod_chain_fixed and k_demod_chain_iq."""
    assert len(_find(meta, "psdr::k_demod_chain_sam<")) == 2
    assert len(_find(meta, "psdr::k_demod_chain_sam<360")) == 1 and len(_find(meta, "psdr::k_demod_chain_sam<720")) == 1
    for k, v in _find(meta, "psdr::k_demod_chain_sam<").items():
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["vgpr"] <= 128, (k, v)
    for k, v in _find(meta, "psdr::k_demod_chain_sam<360").items():
        assert v["vgpr"] <= 96, (k, v)
    for k, v in _find(meta, "psdr::k_demod_ola_sam").items():
        assert v["scratch"] == 0, (k, v)
    # ... and the siblings still meet their budgets beside it
    for name in ("psdr::k_demod_chain_fixed<", "psdr::k_demod_chain_iq<"):
        for k, v in _find(meta, name).items():
            assert v["vgpr"] <= 128 and v["scratch"] == 0, (k, v)

"""IQ client mode without a GPU: the ABI additions (include/psdr.h, libpsdr_hip.so, the ctypes binding) and what the built
library's code objects say about the IQ chain kernel."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

import codeobj


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psdr.h")).read(), flags=re.S)


def test_header_declares_the_mode_the_fetch_bit_and_the_calls_and_keeps_the_abi_number():
    h = _header()
    assert re.search(r"#define\s+PSDR_ABI_VERSION\s+3\b", h)
    assert re.search(r"\bPSDR_IQ\s*=\s*4\b", h)
    for name, val in (("PSDR_USB", 0), ("PSDR_LSB", 1), ("PSDR_AM", 2), ("PSDR_FM", 3)):    # the earlier modes keep their numbers
        assert re.search(rf"\b{name}\s*=\s*{val}\b", h), name
    assert re.search(r"#define\s+PSDR_FETCH_IQ\s+8u\b", h)
    for name, val in (("PSDR_FETCH_AUDIO", 1), ("PSDR_FETCH_PCM", 2), ("PSDR_FETCH_WATERFALL", 4)):
        assert re.search(rf"#define\s+{name}\s+{val}u\b", h), name
    assert re.search(r"int\s+psdr_read_iq\s*\(\s*psdr_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*float\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,"
                     r"\s*int32_t\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+\s*\)\s*;", h)
    assert re.search(r"int\s+psdr_fetched_iq\s*\(\s*psdr_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+float\s*\*\*\s*\w+\s*,"
                     r"\s*float\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)\s*;", h)
    assert re.search(r"int\s+psdr_iq_device_ptr\s*\(\s*psdr_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+float\s*\*\*\s*\w+\s*,"
                     r"\s*const\s+float\s*\*\*\s*\w+\s*\)\s*;", h)


def test_library_exports_the_iq_entry_points_and_keeps_the_abi_number():
    lib = ctypes.CDLL(os.path.join(ROOT, "phantomsdr_amd", "libpsdr_hip.so"))
    for name in ("psdr_read_iq", "psdr_fetched_iq", "psdr_iq_device_ptr"):
        assert hasattr(lib, name), name
    lib.psdr_abi_version.restype = ctypes.c_int
    assert lib.psdr_abi_version() == 3
    # (no device needed: the argument check comes first)
    lib.psdr_read_iq.restype = ctypes.c_int
    lib.psdr_read_iq.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4
    assert lib.psdr_read_iq(None, 0, 1, None, None, None, None) == -1
    lib.psdr_iq_device_ptr.restype = ctypes.c_int
    lib.psdr_iq_device_ptr.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.psdr_iq_device_ptr(None, 0, None, None) == -1


def test_python_binding_knows_the_mode():
    from phantomsdr_amd import _lib, core
    assert core.IQ == 4 and core.MODES["IQ"] == 4
    assert {k: core.MODES[k] for k in ("USB", "LSB", "AM", "FM")} == {"USB": 0, "LSB": 1, "AM": 2, "FM": 3}
    assert core.Context.FETCH_IQ == 8
    bound = {name for name, _, _ in _lib.SYMBOLS}
    assert {"psdr_read_iq", "psdr_fetched_iq", "psdr_iq_device_ptr"} <= bound
    assert callable(core.AudioClient.read_iq) and callable(core.Context.fetched_iq)


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
def test_iq_chain_kernel_fits_beside_a_pass(meta):
    """k_demod_chain_iq takes k_demod_chain_fixed's seat beside a pass: no scratch, at most 128 registers
    at n = 720 and the 80 that cfg2's second pass and the PAIR first passes leave at n = 360."""
    assert len(_find(meta, "psdr::k_demod_chain_iq<")) == 2
    for k, v in _find(meta, "psdr::k_demod_chain_iq<").items():
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["vgpr"] <= 128, (k, v)
    for k, v in _find(meta, "psdr::k_demod_chain_iq<360").items():
        assert v["vgpr"] <= 80, (k, v)
    for k, v in _find(meta, "psdr::k_demod_ola_iq").items():
        assert v["scratch"] == 0, (k, v)
    # ... and its sibling still meets the same budgets beside it
    for k, v in _find(meta, "psdr::k_demod_chain_fixed<").items():
        assert v["vgpr"] <= 128 and v["scratch"] == 0, (k, v)
    for k, v in _find(meta, "psdr::k_demod_chain_fixed<360").items():
        assert v["vgpr"] <= 80, (k, v)

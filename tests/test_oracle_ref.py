"""Pins the oracle against the REFERENCE'S OWN compiled code (oracle/_ref, built in place
from the reference's src/utils/{dsp,audioprocessing}.cpp with the reference's flags):
bit-exact for the Hann window, AM envelope, FM discriminator, float->int16 and the AGC.

What the reference's code returned for each input below is recorded as a SHA-256 of its
output bytes in tests/golden/ref_dsp_sha256.json (tools/gen_ref_golden.py writes it from
oracle/_ref), so the oracle is held to it on every machine; where oracle/_ref is built, the
reference is also called live and compared array for array, and must still match the record."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

R = O.ref()  # None without the reference tree
p = O._p
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_dsp_sha256.json")
HANN_SIZES = [16, 1000, 1 << 16, 1 << 20]
AGC_ARGS = (0.2, 50.0, 300.0, 200.0, 12000.0)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)


def am_fm_int16_inputs():
    rng = np.random.default_rng(3)
    n = 50000
    z = O.aligned(2 * n, np.float32)
    z[:] = rng.standard_normal(2 * n).astype(np.float32) * 0.1
    x = O.aligned(n, np.float32)
    x[:] = rng.standard_normal(n).astype(np.float32) * 3
    return z, x


def negate_add_inputs():
    rng = np.random.default_rng(4)
    n = 4096
    a = O.aligned(n, np.float32)
    b = O.aligned(n, np.float32)
    a[:] = rng.standard_normal(n)
    b[:] = rng.standard_normal(n)
    return a, b


def agc_blocks():
    rng = np.random.default_rng(7)
    return [(rng.standard_normal(180) * (0.01 + 0.5 * (it % 7 == 0))).astype(np.float32) for it in range(120)]


def ref_outputs(R):
    """the reference's outputs for the inputs above, by golden key"""
    out = {}
    for n in HANN_SIZES:
        a = O.aligned(n, np.float32)
        R.ref_build_hann_window(p(a), n)
        out[f"hann_{n}"] = a.copy()
    z, x = am_fm_int16_inputs()
    n = x.size
    o = O.aligned(n, np.float32)
    R.ref_dsp_am_demod(p(z), p(o), n)
    out["am"] = o.copy()
    R.ref_polar_discriminator_fm(p(z), 0.3, -0.2, p(o), n)
    out["fm"] = o.copy()
    i = O.aligned(n, np.int32)
    R.ref_dsp_float_to_int16(p(x), p(i), 16384.0, n)
    out["int16"] = i.copy()
    a, b = negate_add_inputs()
    R.ref_dsp_negate_float(p(a), a.size)
    out["negate_float"] = a.copy()
    R.ref_dsp_add_float(p(a), p(b), a.size)
    out["add_float"] = a.copy()
    R.ref_dsp_negate_complex(p(a), a.size // 2)
    R.ref_dsp_add_complex(p(a), p(b), a.size // 2)
    out["negate_add_complex"] = a.copy()
    ra = R.ref_agc_create(*AGC_ARGS)
    for it, s in enumerate(agc_blocks()):
        s1 = O.aligned(s.size, np.float32)
        s1[:] = s
        R.ref_agc_process(ra, p(s1), s.size)
        out[f"agc_{it}"] = s1.copy()
        if it == 60:
            R.ref_agc_reset(ra)
    R.ref_agc_destroy(ra)
    return out


def input_digests():
    z, x = am_fm_int16_inputs()
    a, b = negate_add_inputs()
    return {"am_fm_z": digest(z), "int16_x": digest(x), "negate_add_a": digest(a), "negate_add_b": digest(b),
            "agc_blocks": digest(np.concatenate(agc_blocks()))}


def pin(key, ours, live=None):
    """`ours` is bit for bit what the reference returned for `key`: the recorded digest, and the live call where built"""
    if live is not None:
        assert np.array_equal(live[key], ours), key
        assert digest(live[key]) == golden()["outputs"][key], f"{key}: the reference no longer matches its record"
    assert digest(ours) == golden()["outputs"][key], key


@pytest.fixture(scope="module")
def live():
    return ref_outputs(R) if R is not None else None


def test_inputs_are_the_recorded_ones():
    """the seeded inputs are those the record was made from (a different random stream would void the digests)"""
    assert input_digests() == golden()["inputs"]


@pytest.mark.parametrize("n", HANN_SIZES)
def test_hann_window(n, live):
    a = O.hann(n)
    pin(f"hann_{n}", a, live)
    assert a[0] == 0.0 and abs(a[n // 2] - 1.0) < 1e-6


def test_am_fm_int16_bit_exact(live):
    z, x = am_fm_int16_inputs()
    n = x.size
    L = O.lib()
    o = np.zeros(n, np.float32)
    L.orc_am_demod(p(z), p(o), n)
    pin("am", o, live)
    L.orc_polar_discriminator_fm(p(z), 0.3, -0.2, p(o), n)
    pin("fm", o, live)
    i = np.zeros(n, np.int32)
    L.orc_float_to_int16(p(x), p(i), 16384.0, n)
    pin("int16", i, live)
    assert i.max() == 32767 and i.min() == -32768  # clamps exercised


def test_negate_add_helpers(live):
    a0, b = negate_add_inputs()
    pin("negate_float", -a0, live)
    pin("add_float", -a0 + b, live)
    pin("negate_add_complex", -(-a0 + b) + b, live)


def test_agc_bit_exact_including_reset(live):
    L = O.lib()
    oa = L.orc_agc_create(*AGC_ARGS)
    for it, s in enumerate(agc_blocks()):
        s2 = s.copy()
        L.orc_agc_process(oa, p(s2), s.size)
        pin(f"agc_{it}", s2, live)
        if it == 60:
            L.orc_agc_reset(oa)
    L.orc_agc_destroy(oa)

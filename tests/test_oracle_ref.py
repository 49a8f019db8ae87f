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


EDGE_RATE, EDGE_BLOCK = 12000, 180


def agc_edge_blocks():
    """(blocks of 180 samples, the block in front of which the AGC is reset): the script of tests/post_chain_edges.py at
    12 kHz as the AGC's own input - a tone of each frame's amplitude times 4 (what the USB client's audio is), exact zeros in
    the silent frames (desired gain 0.2 / 1e-10 = 2e9, reached to about a third in (d)), the burst of amplitude 4 behind them,
    float32 denormals in (f)"""
    import post_chain_edges as E
    s = E.Script(EDGE_RATE, 2 * EDGE_BLOCK)
    t = np.arange(s.nframes * EDGE_BLOCK)
    tone = np.cos(2 * np.pi * E.TONE * t / (2 * EDGE_BLOCK) + 0.3)
    x = (4.0 * np.repeat(s.amp, EDGE_BLOCK) * tone).astype(np.float32)
    return [x[k * EDGE_BLOCK:(k + 1) * EDGE_BLOCK] for k in range(s.nframes)], s.reset_at




def int16_edge_inputs():
    """+-0, denormals, every boundary of the conversion (t = fma(x, 16384, 32768.5) = -1, -0.5, 0, 65535, 65535.5, 65536) with
    its float32 neighbours, decades, and magnitudes up to the last for which the reference's expression `(int32)t - 32768` is
    defined: t < 2^31 for the conversion and t >= -2^31 + 32768 for the subtraction behind it (x = -131072 is the last)"""
    f32 = np.float32
    at = [f32((t - 32768.5) / 16384.0) for t in (-1.0, -0.5, 0.0, 0.5, 1.0, 32768.0, 65534.5, 65535.0, 65535.5, 65536.0, 65536.5)]
    v = []
    for x in at:
        v += [np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))]
    v += [f32(0.0), f32(-0.0)]
    for m in (1.4e-45, 1e-39, 1.1754942e-38, 1.1754944e-38, 1e-30, 1e-10, 1e-5, 6.1e-5, 1e-3, 0.1, 1.0, 1.99993, 2.0, 3.0, 10.0, 1e2, 1e3, 1e4,
              1e5, 131069.0, 131069.98):
        v += [f32(m), f32(-m)]
    v += [f32(-131072.0), f32(-131071.99), f32(-131071.0), np.nextafter(f32(131070.0), f32(0))]
    rng = np.random.default_rng(11)
    v += list((rng.standard_normal(400) * 10.0 ** rng.uniform(-3, 5, 400)).astype(f32).clip(-131071.0, 131069.0))
    v += [f32(0.0)] * (-len(v) % 64)
    x = O.aligned(len(v), f32)
    x[:] = np.array(v, f32)
    t = (x.astype(np.float64) * 16384.0 + 32768.5).astype(f32)
    assert (t >= -2.0 ** 31 + 32768).all() and (t < 2.0 ** 31).all()
    return x


def int16_contract(x, mult=16384.0):
    """include/psdr.h, psdr_set_post_chain: t = fma(x, mult, 32768.5); t >= 65536 -> 32767, t < 0 -> -32768, else (int)t - 32768
    (x * mult is exact in float64 and so is the sum wherever it decides anything: one rounding, like the fma)"""
    with np.errstate(over="ignore"):  # (beyond float32: +-Inf, as the fma gives)
        t = (np.asarray(x, np.float32).astype(np.float64) * mult + 32768.5).astype(np.float32)
    return np.where(t >= 65536, 32767, np.where(t < 0, -32768, np.trunc(np.clip(t, 0, 65535)) - 32768)).astype(np.int32)


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
    blocks, reset_at = agc_edge_blocks()
    ra = R.ref_agc_create(0.2, 50.0, 300.0, 200.0, float(EDGE_RATE))
    got = []
    for it, s in enumerate(blocks):
        if it == reset_at:
            R.ref_agc_reset(ra)
        s1 = O.aligned(s.size, np.float32)
        s1[:] = s
        R.ref_agc_process(ra, p(s1), s.size)
        got.append(s1.copy())
    R.ref_agc_destroy(ra)
    out["agc_edges"] = np.concatenate(got)
    x = int16_edge_inputs()
    i = O.aligned(x.size, np.int32)
    R.ref_dsp_float_to_int16(p(x), p(i), 16384.0, x.size)
    out["int16_edges"] = i.copy()
    return out


def input_digests():
    z, x = am_fm_int16_inputs()
    a, b = negate_add_inputs()
    return {"am_fm_z": digest(z), "int16_x": digest(x), "negate_add_a": digest(a), "negate_add_b": digest(b),
            "agc_blocks": digest(np.concatenate(agc_blocks())), "agc_edge_blocks": digest(np.concatenate(agc_edge_blocks()[0])),
            "int16_edge_x": digest(int16_edge_inputs())}


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


def test_agc_far_from_its_target_bit_exact(live):
    """silence (the gain climbs towards 2e9), a burst behind it (the attack from 1e8 down), a reset in mid-silence, denormals:
    orc_agc_process against the reference's own code, every sample of every block"""
    L = O.lib()
    blocks, reset_at = agc_edge_blocks()
    oa = L.orc_agc_create(0.2, 50.0, 300.0, 200.0, float(EDGE_RATE))
    got = []
    for it, s in enumerate(blocks):
        if it == reset_at:
            L.orc_agc_reset(oa)
        s2 = s.copy()
        L.orc_agc_process(oa, p(s2), s.size)
        got.append(s2)
    L.orc_agc_destroy(oa)
    y = np.concatenate(got)
    pin("agc_edges", y, live)
    x = np.concatenate(blocks)
    gain = np.abs(y[x != 0].astype(np.float64) / x[x != 0])
    assert gain.max() > 1e8 and np.isfinite(y).all()   # the regime, from the input and the pinned output alone
    assert np.count_nonzero(np.abs(y.astype(np.float64)) * 16384 > 2.0 ** 31) >= 20
    silent = np.repeat([not b.any() for b in blocks], EDGE_BLOCK)
    assert not y[reset_at * EDGE_BLOCK:][:EDGE_RATE // 5 - 1].any() and silent[reset_at * EDGE_BLOCK]


def test_int16_conversion_at_every_edge_bit_exact(live):
    """inside int32 the reference's expression is defined, and the oracle's definition - the argument clamped BEFORE the
    conversion - is that value bit for bit; the contract restated in numpy agrees"""
    x = int16_edge_inputs()
    i = np.zeros(x.size, np.int32)
    O.lib().orc_float_to_int16(p(x), p(i), 16384.0, x.size)
    pin("int16_edges", i, live)
    assert np.array_equal(i, int16_contract(x))
    assert i.max() == 32767 and i.min() == -32768 and not i[np.abs(x) < 1e-5].any()  # (+-0 and denormals: 0)


def test_int16_conversion_beyond_int32_saturates_by_sign():
    """where the reference's expression is undefined (its x86 build: +32767 for both signs) the definition is plain saturation
    by sign - checked against the contract alone, nothing of this is sent to the reference"""
    big = np.array([131070.0, 131072.0, 2e5, 1e6, 1e10, 1e20, 3.4e38, np.inf], np.float32)
    x = np.concatenate([big, -np.concatenate([[131072.5, 131074.5], big[1:]]).astype(np.float32)])
    i = np.zeros(x.size, np.int32)
    O.lib().orc_float_to_int16(p(x), p(i), 16384.0, x.size)
    assert np.array_equal(i, np.where(x > 0, 32767, -32768)), (x, i)
    assert np.array_equal(i[np.isfinite(x)], int16_contract(x[np.isfinite(x)]))

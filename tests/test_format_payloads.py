"""The premise of tests/test_gpu_format_invariance.py, on the CPU: the members of a payload family (format_payloads) are
different byte streams that the converter (oracle.convert, bit-pinned to the reference's convert<T> of
src/samplereader.cpp:29-40) maps to the same f32 values bit for bit - so the reference alone satisfies what the GPU test
demands - and they carry the extreme codes where the GPU test needs them."""
import numpy as np
import pytest

from format_payloads import BITS, EXTREMES, FAMILIES, INTEGER_FORMATS, family, half_frame_bytes, plant_positions
from helpers import FMT_DTYPE
from oracle import oracle as O

SHAPES = [(1 << 12, False), (1 << 13, True), (1 << 16, False), (1 << 17, True)]
F = 3


def _ids(s):
    return f"{'real' if s[1] else 'iq'}{s[0].bit_length() - 1}"


@pytest.mark.parametrize("fam", sorted(FAMILIES))
@pytest.mark.parametrize("N,is_real", SHAPES, ids=[_ids(s) for s in SHAPES])
def test_members_convert_to_the_same_f32_bits(N, is_real, fam):
    members = family(fam, N, is_real, F, seed=5 + N.bit_length())
    assert tuple(f for f, _ in members) == FAMILIES[fam]
    first = O.convert(members[0][1], members[0][0])
    assert np.isfinite(first).all() and np.abs(first).max() <= 1.0 and first.std() > 0
    for fmt, raw in members:
        assert raw.dtype == FMT_DTYPE[fmt]
        got = O.convert(raw, fmt)
        bad = got.view(np.uint32) != first.view(np.uint32)
        assert not bad.any(), f"family {fam}: {fmt} and {members[0][0]} convert differently at {int(bad.sum())} samples, first at {int(np.argmax(bad))}"
    # different bytes: the identity is the converter's doing, not the payload's
    for (fa, ra), (fb, rb) in zip(members, members[1:]):
        assert ra.dtype != rb.dtype or not np.array_equal(ra, rb), (fa, fb)
    if fam == "C":  # full-mantissa values: the f64 member does not fit f32, and the f32 member is its nearest-even rounding
        f32, f64 = members[0][1], members[1][1]
        assert (f64 != f32.astype(np.float64)).mean() > 0.9
        assert np.array_equal(f32, f64.astype(np.float32))
    if fam == "B":  # the low bytes family A leaves at zero
        assert (members[0][1].astype(np.int32) & 0xFF).any()
    if fam == "A":
        assert not (members[0][1].astype(np.int32) & 0xFF).any()


@pytest.mark.parametrize("fam", sorted(EXTREMES))
@pytest.mark.parametrize("N,is_real", SHAPES, ids=[_ids(s) for s in SHAPES])
def test_extreme_codes_are_planted_in_every_integer_member(N, is_real, fam):
    members = family(fam, N, is_real, F, seed=5 + N.bit_length())
    lo, hi = EXTREMES[fam]
    full = 1 << (8 if fam == "A" else 16)   # the family's values in units of its own step
    per_half = (N // 2) * (1 if is_real else 2)
    pos = plant_positions(N, is_real)
    assert pos[0][0] == 0 and pos[1][0] == per_half - 2 and pos[2][0] == per_half          # first half-frame, start of the second
    assert 2 * per_half <= pos[3][0] and pos[4][0] + 1 < 3 * per_half                      # inside half-frame 2
    seen = 0
    for fmt, raw in members:
        if fmt not in INTEGER_FORMATS:
            continue
        seen += 1
        bits = BITS[fmt]
        signed = raw.astype(np.int64) - ((1 << (bits - 1)) if fmt.startswith("u") else 0)
        step = (1 << bits) // full
        for at, which in pos:
            want = [(lo, hi)[w] * step for w in which]
            assert [int(signed[at]), int(signed[at + 1])] == want, (fmt, at)
        # the format's own lowest code, and the highest code the family's values reach in it
        assert signed.min() == -(1 << (bits - 1)) and signed.max() == hi * step
        if fmt.startswith("u"):
            assert raw.min() == 0
        if step == 1:
            assert signed.max() == (1 << (bits - 1)) - 1
    assert seen == (4 if fam == "A" else 2)
    # and they survive the conversion: -1.0 and the largest value below 1.0
    conv = O.convert(members[0][1], members[0][0])
    assert conv.min() == -1.0 and conv.max() == np.float32(hi / (full // 2))


@pytest.mark.parametrize("fam", sorted(FAMILIES))
@pytest.mark.parametrize("N,is_real", SHAPES + [(1 << 22, False), (1 << 23, True)], ids=[_ids(s) for s in SHAPES] + ["iq22", "real23"])
def test_member_byte_lengths(N, is_real, fam):
    """half_frame_bytes * (F + 1) as computed from the format (what Context.half_frame_bytes answers on the GPU)"""
    if N > 1 << 17:   # the arithmetic only: no stream of that size here
        for fmt in FAMILIES[fam]:
            assert half_frame_bytes(N, is_real, fmt) == (N // 2) * (1 if is_real else 2) * {"u8": 1, "s8": 1, "u16": 2, "s16": 2, "f32": 4, "f64": 8}[fmt]
        return
    for fmt, raw in family(fam, N, is_real, F, seed=1):
        assert raw.ndim == 1 and raw.nbytes == half_frame_bytes(N, is_real, fmt) * (F + 1), fmt

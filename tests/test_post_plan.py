"""The post chain's plan (phantomsdr_amd/csrc/postplan.h pc_resolve) as a table, without a GPU and without the library:
tests/post_plan_table.cpp is compiled with the host C++ compiler - the header is plain C++17 - and prints the plan of every
case below.  For an audio rate, a frame size and a slot count this is the one place that says which chain a context runs:
the moving-average form, the AGC form, the work-group shape and the dynamic LDS of the recurrence launches."""
import os
import subprocess

import pytest

from conftest import ROOT

KiB = 1024
# facts: audio_rate, n, slots (+ max_batch 512, not pipelined, every option at its default unless named)
# the placement every row with 4 slots shares
SMALL = dict(groups=1, lanes=32, rgroups=2, reserve=8, own=1)
ONE, FIVE = "AGC_ONE_KERNEL", "AGC_FIVE"
CASES = {
    # ---- the table of rates, frame sizes and slot counts
    "12k n248": (dict(rate=12000, n=248, slots=4), dict(SMALL, D=32, L=2400, vo=1, agc_ok=1, ma="MA2_CMW", agc=ONE, direct=1, rows4=1, ma_lds=0)),
    "12k n248 agc0": (dict(rate=12000, n=248, slots=4, agc=0), dict(SMALL, D=32, L=2400, vo=1, agc_ok=1, ma="MA2", agc=FIVE, direct=0, ma_lds=0, gain_lds=0)),
    "12k n252": (dict(rate=12000, n=252, slots=4), dict(SMALL, D=32, L=2400, h=126, vo=1, agc_ok=0, ma="MA2", agc=FIVE, direct=0, rows4=0)),
    "12k n252 agc0": (dict(rate=12000, n=252, slots=4, agc=0), dict(SMALL, agc_ok=0, ma="MA2", agc=FIVE, direct=0, rows4=0)),
    "6k n360": (dict(rate=6000, n=360, slots=4), dict(SMALL, D=16, L=1200, vo=1, agc_ok=1, ma="MAD", ma_lds=16 * 32 * 4, agc=ONE, direct=0)),
    "6k n360 agc0": (dict(rate=6000, n=360, slots=4, agc=0), dict(SMALL, ma="MAD", ma_lds=16 * 32 * 4, agc=FIVE, direct=0)),
    "48k n248": (dict(rate=48000, n=248, slots=4), dict(SMALL, D=128, L=9600, vo=1, agc_ok=1, ma="MAD", ma_lds=128 * 32 * 4, agc=ONE, direct=0)),
    "48k n248 agc0": (dict(rate=48000, n=248, slots=4, agc=0), dict(SMALL, ma="MAD", agc=FIVE, direct=0)),
    "192k n248": (dict(rate=192000, n=248, slots=4), dict(SMALL, D=512, L=38400, vo=1, agc_ok=1, ma="MAD", ma_lds=64 * KiB, agc=ONE, direct=0)),
    "192k n248 agc0": (dict(rate=192000, n=248, slots=4, agc=0), dict(SMALL, ma="MAD", ma_lds=64 * KiB, agc=FIVE, direct=0)),
    "44.1k n248": (dict(rate=44100, n=248, slots=4), dict(SMALL, D=116, L=8820, vo=1, agc_ok=0, ma="MA_DIV", ma_lds=0, agc=FIVE, direct=0)),
    "44.1k n248 agc0": (dict(rate=44100, n=248, slots=4, agc=0), dict(SMALL, agc_ok=0, ma="MA_DIV", agc=FIVE, direct=0)),
    "12k n360 600 slots": (dict(rate=12000, n=360, slots=600),
                           dict(D=32, L=2400, vo=1, agc_ok=1, ma="MA2", agc=FIVE, direct=1, groups=10, lanes=64, rgroups=10, reserve=16, own=1, ma_lds=0, gain_lds=0)),
    "12k n360 600 slots agc0": (dict(rate=12000, n=360, slots=600, agc=0), dict(ma="MA2", agc=FIVE, direct=0, lanes=64, rgroups=10, reserve=16, own=1)),
    # (the form that shares CUs with the passes: test_gpu_post_chain_forms.py::test_post_chain_form_is_bit_exact[12000-n360-2000])
    "12k n360 2000 slots": (dict(rate=12000, n=360, slots=2000),
                            dict(D=32, L=2400, vo=1, agc_ok=1, ma="MA2", agc=FIVE, direct=1, groups=32, lanes=64, rgroups=32, reserve=24, own=0, ma_lds=0, gain_lds=0)),
    "12k n360 2000 slots agc0": (dict(rate=12000, n=360, slots=2000, agc=0), dict(ma="MA2", agc=FIVE, direct=0, lanes=64, rgroups=32, reserve=24, own=0, ma_lds=0)),
    # ---- the rates and frame sizes of test_gpu_post_chain_forms.py: the two one-wave moving averages (MA_POW2: D a power of two
    # below 16; MA_DIV: any D) in front of either AGC, a look-ahead of one sub-block, frames of one row group
    "1k n248": (dict(rate=1000, n=248, slots=4), dict(SMALL, D=2, L=200, vo=1, agc_ok=0, ma="MA_POW2", agc=FIVE, rows4=0, nsub=1, sb=200, direct=0, ma_lds=0)),
    "1.5k n248": (dict(rate=1500, n=248, slots=4), dict(SMALL, D=4, L=300, vo=1, agc_ok=0, ma="MA_POW2", agc=FIVE, rows4=1, nsub=2, sb=150, direct=0)),
    "3.2k n248": (dict(rate=3200, n=248, slots=4), dict(SMALL, D=8, L=640, vo=1, agc_ok=1, ma="MA_POW2", agc=ONE, rows4=1, nsub=3, direct=0, ma_lds=0)),
    "3.2k n248 agc0": (dict(rate=3200, n=248, slots=4, agc=0), dict(SMALL, ma="MA_POW2", agc=FIVE, rows4=1, direct=0)),
    "8k n248": (dict(rate=8000, n=248, slots=4), dict(SMALL, D=20, L=1600, vo=1, agc_ok=1, ma="MA_DIV", agc=ONE, rows4=1, direct=0, ma_lds=0)),
    "8k n360": (dict(rate=8000, n=360, slots=4), dict(SMALL, D=20, L=1600, h=180, agc_ok=1, ma="MA_DIV", agc=ONE, rows4=1, direct=0)),
    "8k n248 agc0": (dict(rate=8000, n=248, slots=4, agc=0), dict(SMALL, ma="MA_DIV", agc=FIVE, rows4=1, direct=0)),
    "16k n248": (dict(rate=16000, n=248, slots=4), dict(SMALL, D=42, L=3200, vo=1, agc_ok=0, ma="MA_DIV", agc=FIVE, rows4=0, direct=0)),
    "22.05k n248": (dict(rate=22050, n=248, slots=4), dict(SMALL, D=58, L=4410, agc_ok=0, ma="MA_DIV", agc=FIVE, rows4=0, direct=0)),
    "12k n8": (dict(rate=12000, n=8, slots=4), dict(SMALL, D=32, L=2400, h=4, agc_ok=0, ma="MA2", agc=FIVE, rows4=1, direct=1, ma_lds=0, gain_lds=0)),
    "12k n32": (dict(rate=12000, n=32, slots=4), dict(SMALL, D=32, L=2400, h=16, agc_ok=1, ma="MA2_CMW", agc=ONE, rows4=1, direct=1)),
    "12k n32 agc0": (dict(rate=12000, n=32, slots=4, agc=0), dict(SMALL, h=16, agc_ok=1, ma="MA2", agc=FIVE, direct=0)),
    # ---- ... and its slot counts: whole waves keep k_pc_mad's ring of D * 64 sums in LDS (192 kHz: 128 KiB, the largest request
    # the library makes), more than 24 work-groups no longer own their SIMDs
    "48k n248 600 slots": (dict(rate=48000, n=248, slots=600),
                           dict(D=128, L=9600, agc_ok=1, ma="MAD", agc=FIVE, direct=0, groups=10, lanes=64, rgroups=10, reserve=16, own=1, ma_lds=32 * KiB, gain_lds=0)),
    "192k n248 600 slots": (dict(rate=192000, n=248, slots=600, max_batch=128),
                            dict(D=512, L=38400, agc_ok=1, ma="MAD", agc=FIVE, groups=10, lanes=64, rgroups=10, reserve=16, own=1, ma_lds=128 * KiB, gain_lds=0)),
    "48k n248 1600 slots": (dict(rate=48000, n=248, slots=1600),
                            dict(D=128, L=9600, ma="MAD", agc=FIVE, groups=25, lanes=64, rgroups=25, reserve=24, own=0, ma_lds=32 * KiB, gain_lds=0)),
    "3.2k n248 600 slots": (dict(rate=3200, n=248, slots=600), dict(ma="MA_POW2", agc=FIVE, lanes=64, rgroups=10, reserve=16, own=1, ma_lds=0)),
    "8k n248 600 slots": (dict(rate=8000, n=248, slots=600), dict(ma="MA_DIV", agc=FIVE, lanes=64, rgroups=10, reserve=16, own=1, ma_lds=0)),
    # ---- the derived numbers of the first row, spelled out (max_batch 512: Tm = 63488)
    "12k n248 numbers": (dict(rate=12000, n=248, slots=4),
                         dict(h=124, px=63840, pv=66208, nsub=10, sb=240, nch=150 + 3968 + 8, h_magic=34636834, nblk=28, att_faster=1, pcm16=0, skip=0)),
    # ---- rates the chain refuses
    "749": (dict(rate=749, n=248, slots=4), dict(verdict="RATE_TOO_SMALL")),
    "750": (dict(rate=750, n=248, slots=4), dict(verdict="OK", D=2, L=150)),
    "D 12288": (dict(rate=4608000, n=248, slots=4), dict(verdict="OK", D=12288)),
    "D 12290": (dict(rate=4608750, n=248, slots=4), dict(verdict="RATE_UNSUPPORTED", D=12290)),
    # ... and frames without a sample (nothing is divided by h = 0)
    "n 0": (dict(rate=12000, n=0, slots=4), dict(verdict="NO_FRAME")),
    "n 1": (dict(rate=12000, n=1, slots=4), dict(verdict="NO_FRAME")),
    "n 2": (dict(rate=12000, n=2, slots=4), dict(verdict="OK", h=1, agc_ok=0)),
    # ---- every knob overrides what its comment says
    "LANES=16": (dict(rate=12000, n=248, slots=4, knobs="LANES=16"), dict(lanes=16, rgroups=4, reserve=8, own=1, ma="MA2_CMW", agc=ONE)),
    # (waves that do not own a SIMD ask for 34 KiB of LDS in all: less the 17 KiB / 8 KiB the kernels declare themselves)
    "OWN=0": (dict(rate=12000, n=248, slots=4, knobs="OWN=0"), dict(SMALL, own=0, ma="MA2", agc=FIVE, direct=1, ma_lds=17 * KiB, gain_lds=26 * KiB)),
    "FUSED=0": (dict(rate=12000, n=248, slots=4, knobs="FUSED=0"), dict(SMALL, ma="MA2", agc=FIVE, direct=1)),
    "CMW=0": (dict(rate=12000, n=248, slots=4, knobs="CMW=0"), dict(SMALL, ma="MA2", agc=ONE, direct=1)),
    "DIRECT=0": (dict(rate=12000, n=248, slots=4, knobs="DIRECT=0"), dict(SMALL, ma="MA2_CMW", agc=ONE, direct=0)),
    "RESERVE=0": (dict(rate=12000, n=248, slots=4, knobs="RESERVE=0"), dict(reserve=0, own=0, ma="MA2", agc=FIVE, ma_lds=0, gain_lds=0)),
    "RESERVE=20": (dict(rate=12000, n=248, slots=4, knobs="RESERVE=20"), dict(reserve=16, own=1, ma="MA2_CMW")),
    "SKIP=0x42": (dict(rate=12000, n=248, slots=4, knobs="SKIP=0x42"), dict(skip=0x42)),
    # ---- options and streams
    "pcm16": (dict(rate=12000, n=248, slots=4, pcm16=1), dict(pcm16=1, ma="MA2_CMW", agc=ONE)),
    "one stream": (dict(rate=12000, n=248, slots=4), dict(s_ma=-1, s_gain=-1, s_peak=-1, split_peak=0, pick_streams=0)),
    "piped": (dict(rate=12000, n=248, slots=4, piped=1), dict(s_ma=0, s_gain=2, s_peak=2, split_peak=1, pick_streams=0)),
    "piped measured": (dict(rate=12000, n=248, slots=4, piped=1, streams=1), dict(s_ma=0, s_gain=2, s_peak=2, pick_streams=1)),
    "PICK=0": (dict(rate=12000, n=248, slots=4, piped=1, streams=1, knobs="PICK=0"), dict(pick_streams=0)),
    "STREAMS=1": (dict(rate=12000, n=248, slots=4, piped=1, knobs="STREAMS=1"), dict(s_ma=0, s_gain=2, s_peak=0, split_peak=0)),
    "STREAMS=2": (dict(rate=12000, n=248, slots=4, piped=1, knobs="STREAMS=2"), dict(s_ma=0, s_gain=1, s_peak=1, split_peak=1)),
    "STREAMS=3": (dict(rate=12000, n=248, slots=4, piped=1, knobs="STREAMS=3"), dict(s_ma=0, s_gain=2, s_peak=1, split_peak=0)),
    "STREAMS=3 one stream": (dict(rate=12000, n=248, slots=4, knobs="STREAMS=3"), dict(s_ma=-1, s_gain=-1, s_peak=-1, split_peak=0)),
    "SPLIT_PEAK=0": (dict(rate=12000, n=248, slots=4, piped=1, knobs="SPLIT_PEAK=0"), dict(s_peak=2, split_peak=0)),
}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("post_plan") / "post_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "phantomsdr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "post_plan_table.cpp"), "-o", exe])
    lines = []
    for f, _ in CASES.values():
        lines.append("%d %d %d %d %d %d %d %d %s" % (f["rate"], f["n"], f.get("max_batch", 512), f["slots"], f.get("piped", 0), f.get("agc", 1),
                                                    f.get("pcm16", 0), f.get("streams", 0), f.get("knobs", "")))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(CASES), r.stdout
    return {name: dict(kv.split("=", 1) for kv in ln.split()) for name, ln in zip(CASES, out)}


@pytest.mark.parametrize("name", list(CASES))
def test_plan_table(plans, name):
    got, want = plans[name], dict(CASES[name][1])
    want.setdefault("verdict", "OK")
    assert {k: got[k] for k in want} == {k: str(v) for k, v in want.items()}, got


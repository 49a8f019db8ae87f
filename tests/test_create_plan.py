"""The create-time planners (phantomsdr_amd/csrc/createplan.h) without a GPU and without the library:
tests/create_plan_table.cpp is compiled with the host C++ compiler - the header is plain C++17 - and runs the scripts below.
What it plans: the configs psdr_create accepts, the split M = M1 * M2 with every stride and layout that hangs off it, every
create-time buffer, the twiddle tables, the audio clients' inverse DFT and the band regions of psdr_set_band_layout.  Every
expectation here is written from the rules (include/psdr.h), and the whole output of one fixed script is held
against the hash of what the same derivation printed while it still sat in psdr_create, build() and psdr_set_band_layout,
between the allocations."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import create_plan_table as T
import forward_plan_table as FT
from conftest import ROOT

INVALID, UNSUPPORTED = -1, -6
LOG2M = range(12, 23)                   # every complex transform length psdr_create accepts
FUSED = {(1024, 1024), (2048, 1024), (1024, 2048)}  # (M1, M2) of the real shapes whose second pass untangles
SPOT = 61                               # permutations from 2^17 points on: every 61st index one-to-one, every index in bounds
BANDS = ((1, 0), (2, 360), (4, 1), (8, 1024), (16, 720), (16, 65536))  # (nbands, halo): the last one's halo is a whole band
AUDIO = (0, 8, 360, 720, 1000, 6400, 10068)


def shape_cases():
    """(log2 M, is_real, environment) - the default environment for all 22, the two that change a real shape where they do"""
    cases = [(m, r, T.env()) for m in LOG2M for r in (0, 1)]
    cases += [(m, 1, T.env(three_pass=1)) for m in (20, 21)] + [(21, 1, T.env(split=1)), (21, 1, T.env(split=1, three_pass=1))]
    return cases


def cfg_of(m, is_real, k):
    """the k-th case's config: every level the shape has, audio sizes of every plan kind in turn, a batch of 1, 2 or 3"""
    return T.cfg(1 << (m + is_real), is_real, levels=m + 1, brightness=k % 3 - 1, additional=AUDIO[k % len(AUDIO)], audio=AUDIO[k % len(AUDIO)],
                 batch=1 + k % 3, clients=k % 5, wf_clients=k % 4, skip=k % 3, wf_size=(0, 1024)[k % 2])


REJECTED = [  # (config, code, text): every rejection of create_check once, in the order it answers them
    (T.cfg(0, 0), INVALID, "fft_size must be a power of two"),
    (T.cfg(4096 + 8, 0), INVALID, "fft_size must be a power of two"),
    (T.cfg(2048, 0), UNSUPPORTED, "fft_size 2048 unsupported: complex transform length must be 2^12..2^22"),
    (T.cfg(1 << 23, 0), UNSUPPORTED, "fft_size 8388608 unsupported: complex transform length must be 2^12..2^22"),
    (T.cfg(4096, 1), UNSUPPORTED, "fft_size 4096 unsupported: complex transform length must be 2^12..2^22"),
    (T.cfg(4096, 0, levels=0), INVALID, "downsample_levels 0 invalid"),
    (T.cfg(4096, 0, levels=14), INVALID, "downsample_levels 14 invalid"),
    (T.cfg(4096, 0, audio=-4), INVALID, "audio_fft_size must be a non-negative multiple of 4"),
    (T.cfg(4096, 0, audio=362), INVALID, "audio_fft_size must be a non-negative multiple of 4"),
    (T.cfg(4096, 0, fmt=-1), INVALID, "unknown input_format -1"),
    (T.cfg(4096, 0, fmt=6), INVALID, "unknown input_format 6"),
    (T.cfg(4096, 0, batch=0), INVALID, "max_batch must be >= 1"),
    (T.cfg(4096, 0, wf_size=-1), INVALID, "waterfall_size must be >= 0"),
]
TWO_FAULTS = [  # the first rule in create_check's order answers
    (T.cfg(1000, 0, levels=0, batch=0), INVALID, "fft_size must be a power of two"),
    (T.cfg(2048, 0, audio=3, wf_size=-1), UNSUPPORTED, "fft_size 2048 unsupported: complex transform length must be 2^12..2^22"),
    (T.cfg(4096, 0, levels=40, fmt=9), INVALID, "downsample_levels 40 invalid"),
    (T.cfg(4096, 0, audio=2, fmt=9), INVALID, "audio_fft_size must be a non-negative multiple of 4"),
    (T.cfg(4096, 0, fmt=9, batch=-2), INVALID, "unknown input_format 9"),
    (T.cfg(4096, 0, batch=0, wf_size=-5), INVALID, "max_batch must be >= 1"),
]
TOO_MANY = 4 * 5 ** 12  # thirteen radices
BAND_REJECTED = [  # on a 2^20-point IQ context: (nbands, halo, code, text)
    (3, 360, INVALID, "nbands 3: a power of two <= 16"), (0, 360, INVALID, "nbands 0: a power of two <= 16"), (32, 0, INVALID, "nbands 32: a power of two <= 16"),
    (8, (1 << 20) + 1, INVALID, "halo of 1048577 bins"),
    (16, 65537, INVALID, "halo of 65537 bins = 65 columns of 1024 bins exceeds a band of 64 columns (16 bands)"),
]
BAND_UNSUPPORTED = "banded spectrum: 2^20- and 2^21-point IQ frames only (use psdr_pack_band)"


def trace_script():
    """every shape, the environment's variants, the rejected configs and the band layouts: what the golden trace was recorded for"""
    lines = []
    for k, (m, r, e) in enumerate(shape_cases()):
        lines += [e, cfg_of(m, r, k)]
        if not r and m in (20, 21):
            for nb, halo in BANDS:
                lines.append("band %d %d" % (nb, halo))  # (each on the banded layout the one before left)
            lines += ["band %d %d" % b[:2] for b in BAND_REJECTED]
        else:
            lines.append("band 2 360")
    lines.append(T.env())
    lines += [c[0] for c in REJECTED + TWO_FAULTS] + [T.cfg(4096, 0, audio=TOO_MANY)]
    for cus in (1, 64, 304):  # the seam buffers of the fused real shapes follow the device's size and PSDR_SEG_LEN
        for seg_len in (0, 4):
            lines += [T.env(seg_len=seg_len, cus=cus)] + [T.cfg(1 << 21, 1, levels=3, batch=b) for b in (1, 2, 65, 305, 512)]
    return "\n".join(lines) + "\n"


TRACE = trace_script()


def rules_script():
    lines = []
    for k, (m, r, e) in enumerate(shape_cases()):
        lines += [e, cfg_of(m, r, k), "perm %d" % (1 if m <= 16 else SPOT)]
        if not r and m in (20, 21):
            for nb, halo in BANDS:
                lines += ["band %d %d" % (nb, halo), "perm %d" % SPOT]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def trace():
    return T.run(T.program(), TRACE)


@pytest.fixture(scope="module")
def rules():
    return T.blocks(T.run(T.program(), rules_script()))


def ints(f, *keys):
    return tuple(int(f[k]) for k in keys)


def test_trace_is_what_create_computed_before_the_planners_moved(trace):
    """recorded before any code moved: the parent's psdr_create, build() and the checks and arithmetic of its psdr_set_band_layout,
    compiled verbatim in front of stand-ins for HIP and the context that note every allocation and upload, printed this script
    (tests/golden/create_plan_trace.json): a mismatch is a change of behaviour"""
    with open(os.path.join(ROOT, "tests", "golden", "create_plan_trace.json")) as f:
        golden = json.load(f)
    assert hashlib.sha256(TRACE.encode()).hexdigest() == golden["input_sha256"], "the script changed: the trace was recorded for another"
    assert hashlib.sha256(trace.encode()).hexdigest() == golden["output_sha256"]


# ---- shapes
def test_every_shape_against_the_rules(rules):
    cases = shape_cases()
    assert len(rules) == len(cases) == 26
    fused_seen = set()
    for (m, r, e), b in zip(cases, rules):
        three_pass, split = e.split()[2] == "1", e.split()[1] == "1"
        s, rec, lay = b["shape"][0], b["recmap"][0], b["lay"][0]
        N, M, R, M1, M2, T1, T2, l2M1, l2M2 = ints(s, "N", "M", "R", "M1", "M2", "T1", "T2", "l2M1", "l2M2")
        assert (N, M, R, int(s["real"])) == (1 << (m + r), 1 << m, 1 << m, r)
        assert M1 * M2 == M and (M1, M2) == (1 << l2M1, 1 << l2M2)
        assert l2M2 == (11 if r and m == 21 and not split else m // 2)  # 2^22-point real frames: 1024 x 2048 unless PSDR_REAL_SPLIT=2048x1024
        assert T1 == min(16384 // M1, M2) and T2 == min(16384 // M2, M1)
        fused = bool(r) and (M1, M2) in FUSED and not three_pass
        assert int(s["fused"]) == fused
        if fused:
            fused_seen.add((M1, M2))
        levels = int(s["levels"])
        q_len, q_stride, p_stride, LT, tiled_lt, ch = ints(s, "q_len", "q_stride", "p_stride", "LT", "tiled_lt", "tile_ch")
        assert levels == m + 1 and q_len == sum(R >> i for i in range(levels)) == 2 * R - 1
        assert q_stride % 128 == 0 and 0 <= q_stride - q_len < 128 and p_stride == max(R >> LT, 64) >= 64
        assert int(s["spec_stride"]) == (M + 2 if r else N)
        # records: IQ tiles of 16 (T2 >= 16) or 8 channels, fused real tiles of T2 / 2 couples, three-pass real none
        mapped = int(rec["mapped"])
        if not r:
            assert (mapped, ch, LT, tiled_lt) == (1, min(T2, 16), 4 if T2 >= 16 else 3, 4 if T2 >= 16 else 3)
        elif fused:
            assert (mapped, ch, LT, tiled_lt, int(rec["pair"])) == (2, T2 // 2, (T2 // 2).bit_length() - 1, (T2 // 2).bit_length() - 1, int(T2 == 8))
        else:
            assert (mapped, LT, tiled_lt) == (0, 8, -1)
        assert int(s["qt_stride"]) == (2 * R if tiled_lt >= 0 else 0)
        assert int(lay["mode"]) == (2 if fused else 1 if not r and (M2, T2) == (1024, 16) else 0)
        assert int(s["l2UB"]) == (min(10, m + 1) if r else 0)
        # every index map is a permutation (whole up to 2^16 points, on a fixed stride above; bounds for every index)
        perms = {p["what"]: p for p in b["perm"][:2]}
        assert set(perms) == ({"bins", "records"} if tiled_lt >= 0 else {"bins"})
        for p in perms.values():
            assert ints(p, "inside", "distinct", "stride") == (1, 1, 1 if m <= 16 else SPOT), p
        assert int(perms["bins"]["count"]) == R and int(perms["bins"]["size"]) == (M + 2 if r else N)
        if tiled_lt >= 0:
            assert int(perms["records"]["count"]) == int(perms["records"]["size"]) == R // ch
    assert fused_seen == FUSED


def test_band_regions_hold_every_bin_once(rules):
    """mode 3: pos() one-to-one, in one of the nbands regions and inside its first frame's stride - for a layout set on the natural
    tile-major one and for every layout set on a banded one"""
    seen = 0
    for (m, r, e), b in zip(shape_cases(), rules):
        if r or m not in (20, 21):
            assert "band" not in b
            continue
        M1 = int(b["shape"][0]["M1"])
        assert len(b["band"]) == len(BANDS) and len(b["perm"]) == 2 + 2 * len(BANDS)
        for i, ((nb, halo), f) in enumerate(zip(BANDS, b["band"])):
            H, Lb = -(-halo // M1), 1024 // nb
            assert ints(f, "code", "H", "Lb", "Lw", "frame_stride", "region") == (0, H, Lb, Lb + H, M1 * (Lb + H), int(b["shape"][0]["maxb"]) * M1 * (Lb + H))
            lay = b["lay"][1 + i]
            assert ints(lay, "mode", "l2Lb", "Lw", "band_stride", "c2_0", "m1", "L") == (3, Lb.bit_length() - 1, Lb + H, int(f["region"]), 0, M1, 1024)
            p = b["perm"][2 + 2 * i + 1]
            assert p["what"] == "bins" and ints(p, "count", "size", "inside", "distinct") == (1 << m, nb * M1 * (Lb + H), 1, 1)
            seen += 1
    assert seen == 2 * len(BANDS)


# ---- rejections
def test_every_rejection_once_with_its_code_and_text():
    out = T.blocks(T.run(T.program(), "\n".join(c[0] for c in REJECTED + TWO_FAULTS) + "\n"))
    assert len(out) == len(REJECTED + TWO_FAULTS)
    for (line, code, text), b in zip(REJECTED + TWO_FAULTS, out):
        assert list(b) == ["check"] and (int(b["check"][0]["code"]), b["check"][0]["msg"]) == (code, text), line


def test_band_layout_rejections():
    lines = [T.env(), T.cfg(1 << 20, 0)] + ["band %d %d" % b[:2] for b in BAND_REJECTED]
    for N, r in ((1 << 12, 0), (1 << 19, 0), (1 << 22, 0), (1 << 13, 1), (1 << 21, 1)):  # natural order, 2048-point rows, real
        lines += [T.cfg(N, r), "band 2 360"]
    lines += [T.cfg(1 << 21, 0), "band 1 0", "band 16 131073"]
    out = T.blocks(T.run(T.program(), "\n".join(lines) + "\n"))
    got = [(int(f["code"]), f["msg"]) for b in out for f in b.get("band", [])]
    assert got == [b[2:] for b in BAND_REJECTED] + [(UNSUPPORTED, BAND_UNSUPPORTED)] * 5 + [
        (0, ""), (INVALID, "halo of 131073 bins = 65 columns of 2048 bins exceeds a band of 64 columns (16 bands)")]
    assert all(len(b["lay"]) == 1 for b in out[:-1]) and len(out[-1]["lay"]) == 2  # a rejected call leaves no layout


# ---- buffers
def test_buffers_exist_where_create_allocates_them(rules):
    z_cases = set()
    for (m, r, e), b in zip(shape_cases(), rules):
        s = b["shape"][0]
        buf = {k: tuple(int(x) for x in v.split(":")) if ":" in v else int(v) for k, v in b["buffers"][0].items()}
        F, M, N, n, fused, tiled = ints(s, "maxb", "M", "N", "n", "fused", "tiled_lt")
        k = shape_cases().index((m, r, e))
        clients, wf = max(1, k % 5), max(1, k % 4)
        assert buf["tickets"] == (512, 1) and buf["Y"] == (F * M, 0)
        # Z: the three-pass real path's second array, one frame of k-order staging where the spectrum is tiled, or nothing
        lay = int(b["lay"][0]["mode"])
        z = "pass" if r and not fused else "staging" if lay else "none"
        assert buf["Z"] == {"pass": (F * M, 0), "staging": (M + 2, 0), "none": (0, 0)}[z]
        z_cases.add(z)
        for name in ("seamP", "seamC", "segflag"):
            assert (buf[name][0] > 0) == bool(fused), name
        assert (buf["seg_cap"] > 0) == bool(fused)
        if fused:
            M2, T2 = ints(s, "M2", "T2")
            cap = buf["seg_cap"]
            assert (buf["seamP"], buf["seamC"], buf["segflag"]) == ((cap * M2 * (T2 // 2), 0), (cap * M2, 0), (3 * cap, 1))
        assert buf["spec"] == (F * int(s["spec_stride"]), 1) and buf["q"] == (F * int(s["q_stride"]), 1) and buf["pscr"] == (F * int(s["p_stride"]), 0)
        assert buf["qt"] == ((F * int(s["qt_stride"]), 1) if tiled >= 0 else (0, 0))
        assert buf["stage"] == ((N if r else 2 * N), 0) and buf["h_q"] == (int(s["q_len"]), 0)
        assert buf["h_out"] == ((N // 2 + 1 if r else N + n), 0)  # (cfg_of: additional_size = the audio size)
        audio = ("ypost", "pwr", "audio", "nan", "real_prev", "bb_tail", "bb_last", "ssb_mark")
        if n == 0:
            assert all(buf[a] == (0, 0) for a in audio + ("gscratch",)) and buf["slots"] == buf["client_ring"] == 0
        else:
            S = clients
            assert buf["slots"] == S and buf["client_ring"] > 0
            assert [buf[a] for a in audio] == [(S * F * n, 0), (S * F, 1), (S * F * (n // 2), 1), (S * F, 1), (S * n, 1), (S * n, 1), (2 * S, 1), (S, 1)]
            assert buf["gscratch"] == ((S * F * 2 * n, 0) if 16 * n > 144 * 1024 else (0, 0))
        assert buf["wslots"] == wf and buf["wf_sent_off"] % 64 == 0 and buf["wf_sent_off"] >= wf * 40 and buf["wf_ring"] == buf["wf_sent_off"] + 4 * F
        assert int(s["skip"]) == max(1, k % 3) and int(s["mwf"]) == (1024 if k % 2 else 1)
    assert z_cases == {"pass", "staging", "none"}


def test_seam_capacity_is_seg_cap():
    """the fused shapes' seam buffers hold seg_cap (forwardplan.h) segments: the largest count over the batch sizes up to max_batch"""
    lines, want = [T.env(cus=256)], []
    for N, split in ((1 << 21, 0), (1 << 22, 0), (1 << 22, 1)):
        for maxb in (1, 2, 257, 512):
            lines += [T.env(split=split, cus=256), T.cfg(N, 1, batch=maxb)]
            G = {(1 << 21, 0): 64, (1 << 22, 0): 128, (1 << 22, 1): 128}[(N, split)]  # tiles of a frame: M1 / T2
            want.append((G, maxb))
    out = T.blocks(T.run(T.program(), "\n".join(lines) + "\n"))
    caps = FT.run(FT.program(), "".join("cap %d 256 0 %d\n" % w for w in want)).splitlines()
    for (G, maxb), b, c in zip(want, out, caps):
        assert ints(b["seg"][0], "G", "cus", "env") == (G, 256, 0)
        assert int(b["buffers"][0]["seg_cap"]) == int(FT.fields(c)["cap"]) == int(FT.fields(c)["brute"]) > 0, (G, maxb)


def test_twiddle_tables(rules):
    for (m, r, e), b in zip(shape_cases(), rules):
        s, tw = b["shape"][0], b["twiddles"][0]
        N, M, M1, M2, T2, n, fused = ints(s, "N", "M", "M1", "M2", "T2", "n", "fused")
        assert tw["Wl1"] == "%d:1:%d:-1" % (M1, M1) and tw["Wl2"] == ("none" if M2 == M1 else "%d:1:%d:-1" % (M2, M2)) and tw["TB"] == "%d:1:%d:-1" % (M2, M)
        UB = min(1024, N)
        assert (tw["UA"], tw["UB"]) == (("%d:%d:%d:-1" % (N // UB + 1, UB, N), "%d:1:%d:-1" % (UB, N)) if r else ("none", "none"))
        assert tw["UG"] == ("%d:%d:%d:-1" % (M1 // T2, T2 // 2, N) if fused else "none")
        assert tw["Wn"] == ("%d:1:%d:1" % (n, n) if n else "none")


# ---- the audio clients' inverse DFT
EDGES = {  # n -> kernel: the last size of a branch and the first of the next (multiples of 4), the compile-time plans, no audio
    512: "wave", 516: "lds0", 6144: "lds0", 6148: "lds1", 9216: "lds1", 9220: "lds2", 360: "fixed", 720: "fixed", 0: "none"}
TABLES = (8, 60, 124, 1000, 6400, 10068, 32, 48, 160, 224, 44, 512, 516, 6144, 6148, 9216, 9220, 360, 720)


def test_idft_branch_edges():
    for n, kernel in EDGES.items():
        rad, got = T.idft(n)
        assert got == kernel and int(np.prod(rad, dtype=np.int64)) == max(n, 1) and all(2 <= x for x in rad), (n, rad, got)
    assert 24 * 6144 == 16 * 9216 == 144 * 1024
    f = T.fields(T.run(T.program(), "idft 516 0\n"))
    assert (f["threads"], f["idft_lds"], T.fields(T.run(T.program(), "idft 512 0\n"))["threads"]) == ("256", str(24 * 516), "128")


def test_idft_factor_count_edge():
    """twelve radices are the most a plan holds: 4 * 5^11 is planned, 4 * 5^12 answers PSDR_ERR_UNSUPPORTED (no table for either)"""
    ok, bad = (T.fields(ln) for ln in T.run(T.program(), "idft %d 0\nidft %d 0\n" % (4 * 5 ** 11, TOO_MANY)).splitlines())
    assert (ok["code"], ok["nstages"], ok["radix"], ok["kind"], ok["lds_mode"]) == ("0", "12", "4" + ",5" * 11, "lds", "2")
    assert (int(bad["code"]), bad["msg"], bad["nstages"]) == (UNSUPPORTED, "audio_fft_size 976562500 has too many factors", "0")
    (b,) = T.blocks(T.run(T.program(), T.cfg(4096, 0, audio=TOO_MANY) + "\n"))
    assert b["check"][0]["code"] == "0" and int(b["idft"][0]["code"]) == UNSUPPORTED and "shape" not in b  # create_check first, then the plan


@pytest.mark.parametrize("n", TABLES)
def test_stage_table_is_the_inverse_dft(n):
    """each stage's (i, j, e1) entries applied in float64: output o = s * (n / R) + i reads x[i + q n / R], q < R, with the twiddle
    W^(q e1), W = exp(2 pi i / n), and goes to y[j].  Bound: tests/test_oracle_dft.py::test_any_length_backward_and_c2r's"""
    head, tab = T.run(T.program(), "idft %d 1\n" % n).splitlines()
    f = T.fields(head)
    rad = [int(r) for r in f["radix"].split(",")]
    tab = np.array(tab.split()[1:], dtype=np.int64).reshape(len(rad), n, 3)
    rng = np.random.default_rng(n)
    x0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x = x0.copy()
    for R, st in zip(rad, tab):
        i, j, e1 = st.T
        q = np.arange(R)[:, None]
        assert sorted(j.tolist()) == list(range(n)) and (i == np.arange(n) % (n // R)).all()
        y = np.empty_like(x)
        y[j] = (x[i[None, :] + q * (n // R)] * np.exp(2j * np.pi * ((q * e1[None, :]) % n) / n)).sum(axis=0)
        x = y
    ref = np.fft.ifft(x0) * n
    assert np.abs(x - ref).max() <= 2e-7 * np.abs(ref).max()


def test_sanitizers(tmp_path, trace):
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    probe = tmp_path / "sanitizer_probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17", *flags, str(probe), "-o", str(tmp_path / "sanitizer_probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime to link against")
    san = T.build(tmp_path, "create_plan_table_san", flags)
    assert T.run(san, TRACE, timeout=600) == trace
    assert T.run(san, rules_script() + "idft 10068 1\nidft %d 0\n" % TOO_MANY, timeout=600)

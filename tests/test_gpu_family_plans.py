"""The client families with launches of their own - PSDR_IQ, PSDR_SAM, SAM-U / SAM-L, tuned USB / LSB / IQ, notched clients - on
every plan the inverse DFT has.  Their family files, test_gpu_layout_clients.py and test_gpu_mixed_clients.py run n = 360 / 720
(the compile-time plans), 256 (k_demod_idft_wave, radices 16 16, h = 128) and 1024 (k_demod_idft in lds_mode 0, radices 16 16 4,
h = 512): h a multiple of the wave size both times, no run-time radix, no transform outside LDS.  Here the same clients run where
the plan behind psdr_create and launch_idft changes branch:

    n      plan           reaches
    8      (8)            k_demod_idft_wave, h = 4, carrier cutoff 0
    60     (12, 5)        k_demod_idft_wave, h = 30 < 64
    124    (4, 31)        k_demod_idft_wave, run-time radix (idft_stage<0>)
    1000   (8, 5, 5, 5)   k_demod_idft lds_mode 0, h = 500: the last round of 64 lanes is ragged
    6400   (16, 16, 5, 5) k_demod_idft lds_mode 1: buffers in LDS, twiddles from global memory
    10068  (12, 839)      k_demod_idft lds_mode 2: buffers in the per-work-group global scratch, run-time radix

plan_of() asks the library's own planner (createplan.h idft_plan, built host-only by tests/create_plan_table.py) and the first
test pins the table above to it: a changed grouping must not silently move a case onto another branch.

Rig: natural-order spectra (the layouts are test_gpu_layout_clients.py's), 2^15-point IQ and 2^16-point real (R = 32768 either
way: the 10064-bin window fits), s16 input, audio_rate 12000, 5 frames as batches of 3 + 1 + 1 with max_batch = 3.  One context
holds one client of each kind on the window +-(h - 2) bins about bin KC: IQ, SAM, SAM-U, SAM-L, tuned USB, tuned LSB, tuned IQ
(fractional audio_mid), a plain AM control, and an IQ and a SAM client with a manual notch of 3 bins beside the carrier,
[KC + 1, KC + 4): bin KC + 1 is a kept carrier bin at every n with cutoff >= 2, so notched() runs in the direct carrier sum and
in idft_item.  At n = 8 two more IQ clients sit on the windows clipped to each sideband.

Signal: test_gpu_sam_mode.py::stream's - noise of sigma 2^-9, one AM carrier of amplitude 8 / sqrt(N) with a 1 kHz tone at index
1.5, 0.37 bin above the even bin KC.

(a) truth: every client's rows, pwr, NaN flags, carrier records and (through the rotator) tuned phase against the float64
    evaluation of its family's definition ON THE SPECTRUM THE GPU PRODUCED (psdr_read_spectrum).  Truth functions and bounds are
    the family files' (SAM.truth_of / audio_bound, SB, FT, IQM.check_iq, helpers.pwr_tolerance): nothing here is a new tolerance.
    SAM's precondition is asserted on the truth first at every n with cutoff >= 1.  At n = 8 the cutoff is 0 and C = 0 exactly:
    audio = Re B for SAM and 2 Re B' for SAM-U / SAM-L, asserted as identities with IQ rows, bit for bit.
(b) bits: the same stream and clients as 1 + 1 + 3 give the same bytes as 3 + 1 + 1; every batch of every run is read through
    psdr_read_* and through psdr_fetch_begin / _end + psdr_fetched_* and must give the same bytes; a SAM-U / SAM-L client's
    carrier record equals its PSDR_SAM_BOTH twin's.
(c) the control list and the scratch, n = 10068: each kind alone in a context of its own gives the bytes it gives in the full
    list - a list that starts its scratch or its ypost rows at the wrong work-group index shows only behind another list.

The worst error / bound ratio per family and n is appended to build/records/family_plans.jsonl (git-ignored).

Measured on MI355X, worst error / bound over both shapes: 2.3e-3 up to n = 6400; at n = 10068 1.9e-2 (tuned, IQ, AM: a radix-839
sum in f32), 4.7e-3 (SAM), 6.6e-3 (SAM-U / SAM-L), 8.4e-4 (carrier records).  No bound of a family file had to be re-derived."""
import functools
import json
import os

import numpy as np
import pytest

import create_plan_table as T
import test_gpu_fine_tune as FT
import test_gpu_iq_mode as IQM
import test_gpu_sam_mode as SAM
import test_gpu_sam_sideband as SB
from helpers import CLIENT_KINDS, assert_same_bits, pwr_tolerance, quantize_raw, read_client, rel_l2, row_names, set_client_kind

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NF, MAXB, RATE = 5, 3, 12000
SPLIT, OTHER_SPLIT = (3, 1, 1), (1, 1, 3)
SHAPES = {"iq15": (1 << 15, 0), "real16": (1 << 16, 1)}  # shape -> (N, is_real)
R = 1 << 15
KC = R // 2  # the carrier sits 0.37 bin above this (even) bin, in client coordinates
OFFSET_BINS = 0.37
KINDS = ("IQ", "SAM", "SAMU", "SAML", "TUSB", "TLSB", "TIQ", "AM")
FRAC = {"TUSB": 0.37, "TLSB": 0.37, "TIQ": 0.63}
SIDE = {"SAM": SB.BOTH, "SAMU": SB.UPPER, "SAML": SB.LOWER}
NOTCH = (KC + 2.5, 3.0)  # psdr_client_set_notch(centre, width) -> [KC + 1, KC + 4)
NOTCH_BINS = (KC + 1, KC + 4)
NOTCHED = ("IQ/nz", "SAM/nz")  # key -> kind: the part before the slash
CLIPPED = ("IQ/upper", "IQ/lower")  # n = 8 only: IQ clients on the clipped windows
# n -> (radices, kernel): what the case is here for
PLANS = {8: ((8,), "wave"), 60: ((12, 5), "wave"), 124: ((4, 31), "wave"), 1000: ((8, 5, 5, 5), "lds0"),
         6400: ((16, 16, 5, 5), "lds1"), 10068: ((12, 839), "lds2")}
RCASES = (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 16)  # demod.h idft_item: the compile-time radices; any other: idft_stage<0>
CASES = [(shape, n) for n in PLANS for shape in SHAPES]
assert SAM.RATE == SB.RATE == FT.RATE == RATE and SAM.OFFSET_BINS == OFFSET_BINS


def kind_of(key):
    return key.split("/")[0]


def keys_of(n):
    return KINDS + NOTCHED + (CLIPPED if n == 8 else ())


# ---- the plan an audio size gets -------------------------------------------------------------------------------------------

def plan_of(n):
    """(radices, kernel) as the library plans them (createplan.h idft_plan, through tests/create_plan_table.py)"""
    return T.idft(n)


def test_every_size_gets_the_plan_it_is_here_for():
    for n, want in PLANS.items():
        assert n % 4 == 0 and plan_of(n) == want, (n, plan_of(n))
        assert 2 * (n // 2 - 2) <= R - 2 and KC + n // 2 < R
    assert SAM.cutoff(8) == 0 and all(SAM.cutoff(n) >= 2 for n in PLANS if n != 8)
    assert all(any(r not in RCASES for r in PLANS[n][0]) for n in (124, 10068))
    assert all(all(r in RCASES for r in PLANS[n][0]) for n in (8, 60, 1000, 6400))
    assert (60 // 2) < 64 and (1000 // 2) % 64 != 0
    # test_gpu_parity.py::test_demod_audio_fft_sizes: the radix cases no other size instantiates, a small run-time prime, lds_mode 1
    assert [plan_of(n) for n in (32, 48, 160, 224, 44)] == [((16, 2), "wave"), ((16, 3), "wave"), ((16, 10), "wave"), ((16, 14), "wave"), ((4, 11), "wave")]


# ---- windows, signal -------------------------------------------------------------------------------------------------------

def window(n, key):
    """(l, audio_mid, r) of client `key`"""
    w = n // 2 - 2
    win = (KC - w, KC + FRAC.get(key, 0.0), KC + w)
    if key == "IQ/upper":
        return SB.clipped(win, SB.UPPER)
    if key == "IQ/lower":
        return SB.clipped(win, SB.LOWER)
    return win


@functools.lru_cache(maxsize=4)
def stream(shape, n):
    """raw s16 samples of NF + 1 half-frames: test_gpu_sam_mode.py::stream's signal at this shape"""
    N, is_real = SHAPES[shape]
    ns = (NF + 1) * (N // 2)
    rng = np.random.default_rng(340 + is_real)
    t = np.arange(ns, dtype=np.float64)
    amp = 8.0 / np.sqrt(N)
    env = 1.0 + 1.5 * np.cos(2 * np.pi * (n / 12.0) / N * t)  # 1 kHz at the audio rate: n / 12 bins
    if is_real:
        x = rng.standard_normal(ns) * 2.0 ** -9 + amp * env * np.cos(2 * np.pi * (KC + OFFSET_BINS) / N * t)
    else:
        fc = ((KC + OFFSET_BINS + N // 2 + 1) % N) / N  # client bin c is frequency index (c + N/2 + 1) mod N
        x = (rng.standard_normal(ns) + 1j * rng.standard_normal(ns)) * 2.0 ** -9 + amp * env * np.exp(2j * np.pi * fc * t)
    assert np.abs(x.real).max() < 1.0 and np.abs(x.imag).max() < 1.0
    return quantize_raw(x, "s16", bool(is_real))


class Frame:
    """what the truth reads of one frame's spectrum (k order, as psdr_read_spectrum gives it): the window's bins in client order
    and the rms of the R bins"""

    def __init__(self, spec, shape, n):
        N, is_real = SHAPES[shape]
        self.rms = float(np.sqrt(np.mean(np.abs(spec[:R].astype(np.complex128)) ** 2)))
        base = 0 if is_real else N // 2 + 1  # the reference's k order: client bin c is k = (c + N/2 + 1) mod N
        self.l0 = KC - (n // 2 - 2)
        self.piece = spec[(self.l0 + base + np.arange(n - 4)) % R].copy()


def slice_of(fr, l, ln):
    assert fr.l0 <= l and l + ln <= fr.l0 + len(fr.piece)
    return fr.piece[l - fr.l0:l - fr.l0 + ln]


def slice_notched(fr, l, ln):
    """the defining rule of a notch (psdr.h): the same client on a spectrum whose notched bins are zero"""
    s = slice_of(fr, l, ln).copy()
    a, b = max(NOTCH_BINS[0] - l, 0), min(NOTCH_BINS[1] - l, ln)
    if b > a:
        s[a:b] = 0
    return s


rms_of = lambda fr: fr.rms


# ---- one context -----------------------------------------------------------------------------------------------------------

def fetched_client(ctx, g, kind, F):
    """read_client's tuple of the fetched set: psdr_fetched_iq / psdr_fetched_audio / psdr_fetched_carrier, frame by frame"""
    mode = CLIENT_KINDS[kind][0]
    rows = [ctx.fetched_iq(g.id, f) if mode == "IQ" else ctx.fetched_audio(g.id, f) for f in range(F)]
    out = (np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.float32), np.array([r[2] for r in rows], np.int32))
    if mode == "SAM":
        car = [ctx.fetched_carrier(g.id, f) for f in range(F)]
        out = out + (np.array([c[0] for c in car], np.float32), np.array([c[1] for c in car], np.float32))
    return out


@functools.lru_cache(maxsize=None)
def run_case(shape, n, split=SPLIT, keys=None):
    """the 5 frames through one context with the clients `keys` (default: all of keys_of(n)) ->
    ({key: rows of the 5 frames}, the 5 Frames).  Every batch is read twice, psdr_read_* and psdr_fetch_begin / _end +
    psdr_fetched_*: the two must agree byte for byte"""
    from phantomsdr_amd import AudioClient, Context
    N, is_real = SHAPES[shape]
    keys = keys_of(n) if keys is None else keys
    raw = stream(shape, n)
    ctx = Context(N, is_real, R.bit_length() - 10, additional_size=n, audio_fft_size=n, audio_rate=RATE, input_format="s16",
                  max_batch=MAXB, max_clients=len(keys))
    d_raw = None
    try:
        d_raw = ctx.dev_alloc(raw.nbytes)
        ctx.h2d(d_raw, raw)
        cl = {}
        for key in keys:
            g = AudioClient(ctx)
            set_client_kind(g, kind_of(key))
            assert g.on_window_message(*window(n, key)), key
            if key in NOTCHED:
                g.set_notch(0, *NOTCH)
            cl[key] = g
        what = ctx.FETCH_AUDIO | (ctx.FETCH_IQ if any(CLIENT_KINDS[kind_of(k)][0] == "IQ" for k in keys) else 0)
        got, frames, frame = {k: [] for k in keys}, [], 0
        for F in split:
            ctx.process_batch(d_raw, F, offset_bytes=frame * ctx.half_frame_bytes())
            ctx.demod_batch(frame)
            for key, g in cl.items():
                got[key].append(tuple(x[:F].copy() for x in read_client(g, kind_of(key), MAXB)))
                if key in NOTCHED:
                    assert g.notches() == [NOTCH_BINS, (0, 0), (0, 0), (0, 0)], key
            frames += [Frame(ctx.read_spectrum(f), shape, n) for f in range(F)]
            ctx.fetch_begin(what)
            ctx.fetch_end()
            for key, g in cl.items():
                assert_same_bits(fetched_client(ctx, g, kind_of(key), F), got[key][-1],
                                 f"{shape} n {n} {key}, frames {frame}..{frame + F - 1}: psdr_fetched_* against psdr_read_*", row_names(kind_of(key)))
            frame += F
        assert frame == NF
        return {k: tuple(np.concatenate([b[i] for b in per]) for i in range(len(per[0]))) for k, per in got.items()}, frames
    finally:
        ctx.synchronize()
        if d_raw is not None:
            ctx.dev_free(d_raw)
        ctx.close()


# ---- (a) truth -------------------------------------------------------------------------------------------------------------

def record(row):
    d = os.path.join(ROOT, "build", "records")
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "family_plans.jsonl"), "a") as f:
            f.write(json.dumps(row) + "\n")
    except OSError:
        pass


def sam_truths(frames, shape, n):
    """{key: truth} of the SAM kinds (cutoff >= 1), SAM's precondition asserted on each before anything is compared"""
    is_real = SHAPES[shape][1]
    win = window(n, "SAM")
    T = {"SAM": SAM.truth_of(frames, slice_of, is_real, n, win, rms_of=rms_of),
         "SAM/nz": SAM.truth_of(frames, slice_notched, is_real, n, win, rms_of=rms_of)}
    for k in T:
        SAM.assert_signal_condition(T[k], (shape, n, k))
    for k in ("SAMU", "SAML"):
        T[k] = SB.truth_of(frames, slice_of, is_real, n, win, SIDE[k], rms_of=rms_of)  # (asserts its own)
    return T


def check_case(shape, n, got, frames, worst):
    """the clients of one context against the float64 definitions on `frames`; worst: {family: largest error / bound}"""
    is_real = SHAPES[shape][1]
    h, win = n // 2, window(n, "SAM")

    def note(fam, err, bound, tag):
        worst[fam] = max(worst.get(fam, 0.0), err / bound)
        assert err <= bound, f"{tag}: {err:.3e} > {bound:.3e}"

    def check_pwr(rows, T_pwr, T_fs, tag):
        assert not rows[2].any(), f"{tag}: NaN flags"
        for f in range(NF):
            note("pwr", abs(rows[1][f] - T_pwr[f]), pwr_tolerance(T_pwr[f], T_fs[f]), f"{tag} frame {f}: pwr {rows[1][f]} against {T_pwr[f]}")

    def check_iq_rows(key, sl, fam):
        B = FT.baseband64_of(frames, sl, is_real, n, window(n, key), 0, NF)
        rows, tag = got[key], f"{shape} n {n} {key}"
        assert rows[0].shape == (NF, h) and rows[0].dtype == np.complex64
        for f in range(NF):
            IQM.check_iq(rows[0][f], B[f], f"{tag} frame {f}")
            worst[fam] = max(worst.get(fam, 0.0), rel_l2(rows[0][f], B[f]) / 1e-4, float(np.abs(rows[0][f] - B[f]).max()) / (2e-4 * float(np.abs(B[f]).max())))
        return B

    # the window's pwr and fwd_scale, whole and notched (a notched client's pwr is the power of what is heard)
    P = {}
    for name, sl in (("whole", slice_of), ("nz", slice_notched)):
        S = [sl(fr, win[0], win[2] - win[0]).astype(np.complex128) for fr in frames]
        P[name] = ([float((np.abs(s) ** 2).sum()) for s in S], [fr.rms * np.sqrt(win[2] - win[0]) for fr in frames])
    for key in keys_of(n):
        if key not in CLIPPED:
            check_pwr(got[key], *P["nz" if key in NOTCHED else "whole"], f"{shape} n {n} {key}")
    # PSDR_IQ: test_gpu_iq_mode.py's bounds (check_iq), on the float64 baseband; AM: test_gpu_parity.py's, audio = |B|
    B = check_iq_rows("IQ", slice_of, "iq")
    check_iq_rows("IQ/nz", slice_notched, "iq_nz")
    assert got["IQ/nz"][0].tobytes() != got["IQ"][0].tobytes(), "the notch took nothing out of the IQ rows"
    rows, tag = got["AM"], f"{shape} n {n} AM"
    for f in range(NF):
        a = np.abs(B[f])
        note("am", rel_l2(rows[0][f], a), 1e-4, f"{tag} frame {f} rel L2")
        note("am", float(np.abs(rows[0][f] - a).max()), 2e-4 * max(float(a.max()), 1e-30), f"{tag} frame {f}")
    # the SAM kinds
    if SAM.cutoff(n) == 0:
        # C = 0 exactly (psdr.h): audio = Re B for SAM, 2 Re B' for SAM-U / SAM-L with B' the IQ row of the clipped window; the
        # carrier record is 0, 0.  Identities with IQ rows that were just compared with the truth - bit for bit
        for key in CLIPPED:
            check_iq_rows(key, slice_of, "iq")
        for key, twin, gain in (("SAM", "IQ", 1.0), ("SAM/nz", "IQ/nz", 1.0), ("SAMU", "IQ/upper", 2.0), ("SAML", "IQ/lower", 2.0)):
            a, iq = got[key][0], got[twin][0]
            assert a.shape == (NF, h) and a.dtype == np.float32 and np.abs(a).max() > 0
            assert a.tobytes() == np.ascontiguousarray(np.float32(gain) * iq.real).tobytes(), f"{shape} n {n} {key}: audio is not {gain} Re of {twin}'s rows"
            assert not got[key][3].any() and not got[key][4].any(), f"{shape} n {n} {key}: carrier record with cutoff 0"
            worst["sam" if gain == 1.0 else "sb"] = max(worst.get("sam" if gain == 1.0 else "sb", 0.0), 0.0)
    else:
        T = sam_truths(frames, shape, n)
        for key in ("SAM", "SAM/nz", "SAMU", "SAML"):
            rows, tag, Tk = got[key], f"{shape} n {n} {key}", T[key]
            fam = {"SAM": "sam", "SAM/nz": "sam_nz"}.get(key, "sb")
            Tc = T["SAM/nz"] if key == "SAM/nz" else T["SAM"]  # whose carrier it is
            assert rows[0].shape == (NF, h) and rows[0].dtype == np.float32
            for f in range(NF):
                bound = SB.audio_bound(Tk, f) if fam == "sb" else SAM.audio_bound(Tk, f)
                note(fam, float(np.abs(rows[0][f] - Tk["audio"][f]).max()), bound, f"{tag} frame {f}")
            lv, off = rows[3], rows[4]
            for f in range(1, NF):  # test_gpu_sam_mode.py::test_carrier_record, against the truth
                cm = np.abs(Tc["C"][f])
                note("carrier", abs(off[f] - Tc["offset_hz"][f]), RATE / (2 * np.pi) * 4 * 2e-4 * (cm.max() / cm.min()) ** 2, f"{tag} frame {f} offset")
                note("carrier", abs(lv[f] - Tc["level"][f]), 2e-4 * Tc["level"][f], f"{tag} frame {f} level")
        assert got["SAM/nz"][3].tobytes() != got["SAM"][3].tobytes(), "the notch took nothing out of the carrier sum"
    # tuned clients: test_gpu_fine_tune.py's float64 anchor - the transform's 2e-4 and the rotator's 2e-6 of the frame's
    # largest sample; USB / LSB are twice a real part
    for kind in ("TUSB", "TLSB", "TIQ"):
        rows, tag, w = got[kind], f"{shape} n {n} {kind}", window(n, kind)
        Bt = FT.baseband64_of(frames, slice_of, is_real, n, FT.clipped(CLIENT_KINDS[kind][0], w), 0, NF)
        rot = Bt * FT.w64(FT.Phase(n).batch(w[1], NF))
        for f in range(NF):
            scale = float(np.abs(Bt[f]).max())
            if kind == "TIQ":
                note("tuned", float(np.abs(rows[0][f] - rot[f]).max()), (2e-4 + 2e-6) * scale, f"{tag} frame {f}")
            else:
                note("tuned", float(np.abs(rows[0][f] - 2.0 * rot[f].real).max()), 2.0 * (2e-4 + 2e-6) * scale, f"{tag} frame {f}")


@pytest.mark.parametrize("shape,n", CASES, ids=[f"{s}-{n}" for s, n in CASES])
def test_every_client_equals_its_definition_on_the_gpus_own_spectrum(shape, n):
    got, frames = run_case(shape, n)
    assert len(frames) == NF and set(got) == set(keys_of(n))
    worst = {}
    try:
        check_case(shape, n, got, frames, worst)
    finally:
        row = dict(test="truth", shape=shape, n=n, plan=list(PLANS[n][0]), kernel=PLANS[n][1], worst_error_over_bound={k: float(v) for k, v in worst.items()})
        record(row)
        print(json.dumps(row))


# ---- (b) bits --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,n", CASES, ids=[f"{s}-{n}" for s, n in CASES])
def test_batch_split_and_way_of_reading_do_not_change_a_bit(shape, n):
    """3 + 1 + 1 against 1 + 1 + 3 (demod.h: "the bits do not depend on the batch split"); run_case itself compares psdr_read_*
    with psdr_fetched_* on every batch of both; SAM-U / SAM-L carry the carrier record of their PSDR_SAM_BOTH twin (psdr.h)"""
    a, _ = run_case(shape, n)
    b, _ = run_case(shape, n, OTHER_SPLIT)
    assert set(a) == set(b) == set(keys_of(n))
    for key, rows in a.items():
        assert rows[0].shape[0] == NF and np.abs(rows[0][1:]).max() > 0 and not rows[2].any(), key
        assert_same_bits(rows, b[key], f"{shape} n {n} {key}: 3 + 1 + 1 against 1 + 1 + 3", row_names(kind_of(key)))
    for res, split in ((a, SPLIT), (b, OTHER_SPLIT)):
        for key in ("SAMU", "SAML"):
            assert_same_bits(res[key][3:], res["SAM"][3:], f"{shape} n {n} {key}, batches {split}: carrier records against the SAM client's",
                             ("carrier level", "carrier offset"))


# ---- (c) the control list and the scratch ----------------------------------------------------------------------------------

def test_each_kind_alone_gives_the_bits_it_gives_in_the_full_list():
    """n = 10068: every list's k_demod_idft works in the global scratch from work-group 0 on and writes ypost by slot; alone, the
    kind is client 0 of slot 0 and no list ran before it"""
    shape, n = "iq15", 10068
    assert PLANS[n][1] == "lds2"
    full, _ = run_case(shape, n)
    for kind in KINDS:
        alone, _ = run_case(shape, n, SPLIT, (kind,))
        assert_same_bits(alone[kind], full[kind], f"{shape} n {n} {kind}: alone against the full list", row_names(kind))


# ---- the size PSDR_SAM is served up to -------------------------------------------------------------------------------------

def test_sam_is_refused_where_the_carrier_sums_index_would_wrap():
    """sam_carrier_dsum (demod.h) looks its twiddle up at (d * j) mod n in 32-bit arithmetic: exact for n < 65536.  From 65540,
    the first multiple of 4 above, a context exists and serves every other mode; PSDR_SAM answers PSDR_ERR_UNSUPPORTED, names
    the limit and leaves the mode alone.  Nothing is demodulated"""
    from phantomsdr_amd import AudioClient, Context, PsdrError
    for n, served in ((65532, True), (65540, False)):
        ctx = Context(1 << 12, 0, 3, additional_size=0, audio_fft_size=n, audio_rate=RATE, input_format="s16", max_batch=1, max_clients=1)
        try:
            g = AudioClient(ctx)
            g.set_audio_demodulation("AM")
            if served:
                g.set_audio_demodulation("SAM")
                g.set_sam_sideband("upper")
                continue
            g.set_sam_sideband("upper")  # (stored; no effect outside SAM)
            with pytest.raises(PsdrError) as e:
                g.set_audio_demodulation("SAM")
            assert e.value.code == SAM.UNSUPPORTED and "65536" in str(e.value) and str(n) in str(e.value)
            assert ctx.lib.psdr_client_set_audio_demodulation(ctx.h, g.id, 5) == SAM.UNSUPPORTED
            for mode in ("IQ", "FM", "USB", "LSB", "AM"):
                g.set_audio_demodulation(mode)
        finally:
            ctx.close()

"""The client families with kernels of their own - PSDR_IQ, PSDR_SAM, SAM-U / SAM-L, tuned USB / LSB / IQ - on every layout
of the spectrum a deployed shape has.  Their family files (test_gpu_iq_mode.py, _sam_mode, _sam_sideband, _fine_tune) and
test_gpu_mixed_clients.py run on 2^12-point IQ / 2^13-point real contexts, where the spectrum is in natural order
(SpecLayout::mode == 0, k0 == 0, pos(k) == k): a raw index where pos() belongs, a wrong base or a read outside a band region
passes all of them.  Here the same clients sit where SpecLayout::pos (csrc/quantize.h) changes branch.

Layouts (context.hip: psdr_create picks M = M1 * M2 and the layout from the shape):
  IQ 2^20    M1 = M2 = 1024, T2 = 16: mode 1, tile-major lines of 16 rows, columns of 1024 bins; with psdr_set_band_layout(4
             bands, halo n) mode 3 on the root and mode 4 on a receiver of one region
  IQ 2^21    M1 = 2048, M2 = 1024: mode 1 with 2048-bin columns (the 8-column pass-1 tiles); modes 3 and 4 likewise; n = 720:
             the chain kernels pre-compute HO = 6 rounds of 64 offsets, the 716-bin windows take the in-loop pos() branch too
  real 2^21  M = 2^20 = 1024 x 1024, fused real pass 2: mode 2, octet tiles (l2cp == 3, lines of 16 bins)
  real 2^22  M = 2^21 = 1024 x 2048 (log2M2 = 11), fused: mode 2, quartet tiles (l2cp == 2, lines of 8 bins)
  IQ 2^12, real 2^13   mode 0; only the linear band path gives it k0 != 0 (psdr_demod_batch_from_band): the cheap control

Rig: s16 input, audio_rate 12000, 9 frames as batches of 6 + 1 + 2 with max_batch = 6 (a chain with a warm-up frame, a one-frame
batch, a ragged last chain).  Paths as test_gpu_mixed_clients.py chooses them: n = 360 through the chain kernels, n = 360 with
PSDR_DEMOD_CHAIN=0 (k_demod_idft_fixed + k_demod_ola_*), n = 256 (k_demod_idft_wave + k_demod_ola_*), n = 720 chain on IQ 2^21.

Every window holds one client of each kind: IQ, SAM, SAM-U, SAM-L, tuned USB, tuned LSB, tuned IQ (fractional audio_mid) and a
plain AM client as the control.  Windows are +-(n/2 - 2) bins about their carrier (placements()): straddling a column boundary;
inside one column (every window crosses tile boundaries of 16 / 8 / 4 rows); real: straddling row M1/2 (the low / mirror
switch) and wholly in the upper half (mirror octets of the reversed column); l == 0; r == R - 1, the widest
psdr_client_on_window_message accepts; and for the band legs a window that starts on a band's first bin with
floor(audio_mid) == l (the carrier low-pass has no bin below it), on an inner band and on the last, and one that starts in a
band and ends in its halo.  (A window that reaches the last band's halo - the spectrum's first column - would hold bins >= R:
no context that owns a whole spectrum can serve it, and the band check refuses l < first_bin, so `cl < 0` in SpecLayout::pos
is not reachable through the checked entry points; the last band's receiver serves the window at the top of the spectrum from
a region - and the linear leg from a packed band - whose halo wraps.)

Signal: test_gpu_sam_mode.py's, one carrier per window - noise of sigma 2^-9, AM carriers of amplitude 8 / sqrt(N) with a 1 kHz
tone at index 1.5, each 0.37 bin above its window's centre bin, more than 2 n bins apart.

(a) truth: every client's rows, pwr, NaN flags, carrier records and (through the rotator) tuned phase against the float64
    evaluation of its family's definition ON THE SPECTRUM THE GPU PRODUCED for the frame (psdr_read_spectrum, which
    test_gpu_plan_sweep.py ties to a complex128 transform at every shape).  Truth functions and bounds are the family files':
    nothing here is a new tolerance.  SAM's precondition (min |C| >= 0.5 max |C|, max |B| / min |C| <= 4 after the first frame)
    is asserted on the truth of every window first.
(b) bits: the same stream, clients and batches through (i) psdr_demod_batch on the context's own spectrum, (ii) a context that
    never transforms, fed the whole spectrum packed linear, (iii) such a context fed one linear band with first_bin != 0 (one
    of them wraps past the end of the spectrum), (iv) IQ 2^20 / 2^21: the banded root's own psdr_demod_batch and receivers of
    an inner and of the last region - all outputs bit-identical to (i).
(c) state: one context that changes from (i) to (ii) and back between batches, against (i) throughout.

The worst error / bound ratio per family and shape is appended to build/records/layout_clients.jsonl (git-ignored)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import test_gpu_fine_tune as FT
import test_gpu_iq_mode as IQM
import test_gpu_sam_mode as SAM
import test_gpu_sam_sideband as SB
from helpers import CLIENT_KINDS, assert_same_bits, pwr_tolerance, quantize_raw, read_client, rel_l2, row_names, set_client_kind

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NF, BATCHES, MAXB, RATE = 9, (6, 1, 2), 6, 12000
OFFSET_BINS = 0.37
NBANDS = 4
KINDS = ("IQ", "SAM", "SAMU", "SAML", "TUSB", "TLSB", "TIQ", "AM")
FRAC = {"TUSB": 0.37, "TLSB": 0.37, "TIQ": 0.63}
SIDE = {"SAM": SB.BOTH, "SAMU": SB.UPPER, "SAML": SB.LOWER}
# shape -> (N, is_real, M1, rows per tile)
SHAPES = {"iq20": (1 << 20, 0, 1024, 16), "iq21": (1 << 21, 0, 2048, 16), "real21": (1 << 21, 1, 1024, 8), "real22": (1 << 22, 1, 1024, 4),
          "iq12": (1 << 12, 0, 0, 0), "real13": (1 << 13, 1, 0, 0)}
LARGE = [("iq20", 360, "1"), ("iq20", 360, "0"), ("iq20", 256, "1"), ("real21", 360, "1"), ("real21", 360, "0"), ("real21", 256, "1"),
         ("iq21", 720, "1"), ("real22", 360, "1")]
CONTROL = [("iq12", 360, "1"), ("real13", 360, "1")]
assert SAM.RATE == SB.RATE == FT.RATE == RATE and SAM.OFFSET_BINS == OFFSET_BINS


def case_id(c):
    return f"{c[0]}-{c[1]}-chain{c[2]}"


def result_size(shape):
    N, is_real = SHAPES[shape][:2]
    return N // 2 if is_real else N


# ---- windows ---------------------------------------------------------------------------------------------------------------

def placements(shape, n):
    """{name: (l, centre bin, r)}: the carrier sits 0.37 bin above the centre bin; a window whose centre bin is l is one-sided
    (floor(audio_mid) == l).  Bands are quarters of the spectrum: the windows of band 1 lie in [R/4, R/2 + n)"""
    R, w = result_size(shape), n // 2 - 2
    m1 = SHAPES[shape][2]
    two = lambda kc: (kc - w, kc, kc + w)
    one = lambda l: (l, l, l + w)
    if not m1:  # the control: band [1600, 2800) and the wrapping band [3500, 4500)
        return {"first": one(1600), "inner": two(2501), "top": two(R - 1 - w)}
    b = R // NBANDS
    p = {"l0": two(w), "first": one(b), "top": two(R - 1 - w), "last_first": one(3 * b)}
    if SHAPES[shape][1]:
        p.update(column=two(b + 44 * m1), tile=two(b + 94 * m1 + 257), half=two(b + 144 * m1 + m1 // 2), upper=two(b + 194 * m1 + 3 * m1 // 4 + 1))
    else:
        p.update(column=two(b + 37 * m1), tile=two(b + 100 * m1 + m1 // 2 + 1), halo=two(2 * b))
    return p


def bands(shape, n):
    """{leg: (first bin, bins)} of the linear bands with first_bin != 0 (band_bounds' shape: a quarter + 1 + n bins)"""
    R = result_size(shape)
    if not SHAPES[shape][2]:
        return {"band": (1600, 1200), "wrap": (3500, 1000)}
    from phantomsdr_amd.distributed import band_bounds
    return {"band": band_bounds(1, R, NBANDS, n), "wrap": band_bounds(NBANDS - 1, R, NBANDS, n)}


def client_window(place, kind):
    l, kc, r = place
    return (l, kc + FRAC[kind] if kind in FRAC else float(kc), r)


def test_the_placements_are_where_pos_changes_branch():
    for shape, n, _ in LARGE + CONTROL:
        N, is_real, m1, tile = SHAPES[shape]
        R, p = result_size(shape), placements(shape, n)
        cars = sorted(kc for _, kc, _ in p.values())
        assert all(b - a > 2 * n for a, b in zip(cars, cars[1:])), (shape, n)
        assert all(0 <= l < r <= R - 1 and r - l <= n for l, _, r in p.values())
        assert p["top"][2] == R - 1 and p["first"][0] == p["first"][1] == bands(shape, n)["band"][0]
        inside = lambda pl, band: band[0] <= pl[0] and pl[2] <= band[0] + band[1]
        assert inside(p["top"], bands(shape, n)["wrap"]) and sum(bands(shape, n)["wrap"]) > R
        if not m1:
            assert inside(p["inner"], bands(shape, n)["band"])
            continue
        col, row = (lambda k: k >> (m1.bit_length() - 1)), (lambda k: k & (m1 - 1))
        assert p["l0"][0] == 0
        l, _, r = p["column"]
        assert col(l) + 1 == col(r - 1) and inside(p["column"], bands(shape, n)["band"])
        l, _, r = p["tile"]
        assert col(l) == col(r - 1) and row(l) // tile < row(r - 1) // tile and (is_real == 0 or row(r - 1) < m1 // 2)
        assert p["last_first"][0] == 3 * R // NBANDS and inside(p["last_first"], bands(shape, n)["wrap"])
        if is_real:
            l, _, r = p["half"]
            assert col(l) == col(r - 1) and row(l) < m1 // 2 < row(r - 1)
            l, _, r = p["upper"]
            assert col(l) == col(r - 1) and m1 // 2 < row(l) < row(r - 1)
        else:
            from phantomsdr_amd.distributed import banded_bounds
            first, bins = banded_bounds(1, R, NBANDS, n, m1)
            l, _, r = p["halo"]
            assert first <= l < first + R // NBANDS < r <= first + bins  # starts in band 1, ends in its halo
            assert all(inside(p[k], (first, bins)) for k in ("first", "column", "tile", "halo"))
            assert all(inside(p[k], banded_bounds(NBANDS - 1, R, NBANDS, n, m1)) for k in ("last_first", "top"))


# ---- signal ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def stream(shape, n):
    """raw s16 samples of NF + 1 half-frames: test_gpu_sam_mode.py's signal with one carrier per window"""
    N, is_real = SHAPES[shape][:2]
    ns = (NF + 1) * (N // 2)
    rng = np.random.default_rng(310 + N.bit_length() + is_real)
    t = np.arange(ns, dtype=np.float64)
    amp = 8.0 / np.sqrt(N)
    env = 1.0 + 1.5 * np.cos(2 * np.pi * (n / 12.0) / N * t)  # 1 kHz at the audio rate: n / 12 bins
    if is_real:
        x, car = rng.standard_normal(ns) * 2.0 ** -9, np.zeros(ns)
    else:
        x, car = (rng.standard_normal(ns) + 1j * rng.standard_normal(ns)) * 2.0 ** -9, np.zeros(ns, np.complex128)
    for _, kc, _ in placements(shape, n).values():
        if is_real:
            car += np.cos(2 * np.pi * (kc + OFFSET_BINS) / N * t)
        else:
            fc = ((kc + OFFSET_BINS + N // 2 + 1) % N) / N  # client bin c is frequency index (c + N/2 + 1) mod N
            car += np.exp(2j * np.pi * fc * t)
    x += amp * env * car
    assert np.abs(x.real).max() < 1.0 and np.abs(x.imag).max() < 1.0
    return quantize_raw(x, "s16", bool(is_real))


# ---- spectra as the GPU produced them --------------------------------------------------------------------------------------

class Frame:
    """what the truth reads of one frame's spectrum: the windows' bins in client order and the rms of the R bins"""

    def __init__(self, spec, shape, n):
        N, is_real = SHAPES[shape][:2]
        R = result_size(shape)
        self.rms = float(np.sqrt(np.mean(np.abs(spec[:R].astype(np.complex128)) ** 2)))
        base = 0 if is_real else N // 2 + 1  # the reference's k order: client bin c is k = (c + N/2 + 1) mod N
        self.pieces = {l: spec[(l + base + np.arange(r - l)) % R].copy() for l, _, r in placements(shape, n).values()}

    def bins(self, l, ln):
        for l0, a in self.pieces.items():
            if l0 <= l and l + ln <= l0 + len(a):
                return a[l - l0:l - l0 + ln]
        raise KeyError((l, ln))


slice_of = lambda fr, l, ln: fr.bins(l, ln)
rms_of = lambda fr: fr.rms


# ---- contexts --------------------------------------------------------------------------------------------------------------

class Leg:
    """one context and its clients: {(window name, kind): AudioClient}"""

    def __init__(self, shape, n, names, max_clients):
        from phantomsdr_amd import AudioClient, Context
        N, is_real = SHAPES[shape][:2]
        R = result_size(shape)
        self.ctx = Context(N, is_real, R.bit_length() - 10, additional_size=n, audio_fft_size=n, audio_rate=RATE, input_format="s16",
                           max_batch=MAXB, max_clients=max_clients)
        self.cl, self.got = {}, {}
        pl = placements(shape, n)
        for name in names:
            for kind in KINDS:
                g = AudioClient(self.ctx)
                set_client_kind(g, kind)
                assert g.on_window_message(*client_window(pl[name], kind)), (name, kind)
                self.cl[(name, kind)] = g
                self.got[(name, kind)] = []

    def read(self, F):
        for key, g in self.cl.items():
            self.got[key].append(tuple(x[:F].copy() for x in read_client(g, key[1], MAXB)))

    def rows(self):
        return {key: tuple(np.concatenate([b[i] for b in per]) for i in range(len(per[0]))) for key, per in self.got.items()}

    def close(self):
        self.ctx.close()


def in_band(shape, n, first, bins):
    return [k for k, (l, _, r) in placements(shape, n).items() if first <= l and r <= first + bins]


def region_of(root, g):
    """(device pointer, frame stride, first bin, bins) of region g of the banded root's last batch"""
    from phantomsdr_amd._lib import check
    p, fs, fb, nb = C.c_void_p(), C.c_size_t(), C.c_uint32(), C.c_uint32()
    check(root.lib.psdr_band_region(root.h, g, C.byref(p), C.byref(fs), C.byref(fb), C.byref(nb)))
    return p, fs.value, fb.value, nb.value


@functools.lru_cache(maxsize=None)
def run_case(shape, n, chain, switch=False):
    """the 9 frames through every leg the shape has -> ({leg: {(window, kind): rows of the 9 frames}}, the 9 Frames of leg
    "own").  switch: leg "own" alone, its second batch demodulated from its own spectrum packed linear (leg (ii)'s source)"""
    from phantomsdr_amd._lib import check
    from phantomsdr_amd.distributed import banded_bounds
    N, is_real, m1, _ = SHAPES[shape]
    R, raw, names = result_size(shape), stream(shape, n), list(placements(shape, n))
    ncl = len(names) * len(KINDS)
    banded = bool(m1) and not is_real and not switch
    old_env = os.environ.get("PSDR_DEMOD_CHAIN")
    os.environ["PSDR_DEMOD_CHAIN"] = chain  # read by psdr_create
    legs, bufs, frames = {}, [], []
    try:
        own = legs["own"] = Leg(shape, n, names, ncl)
        lib = own.ctx.lib
        d_raw = own.ctx.dev_alloc(raw.nbytes)
        bufs.append(d_raw)
        own.ctx.h2d(d_raw, raw)
        hb = own.ctx.half_frame_bytes()
        d_lin = own.ctx.dev_alloc(MAXB * R * 8)
        bufs.append(d_lin)
        lin_bands = {}
        if not switch:
            legs["linear"] = Leg(shape, n, names, ncl)
            for leg, (first, bins) in bands(shape, n).items():
                legs[leg] = Leg(shape, n, in_band(shape, n, first, bins), ncl)
                lin_bands[leg] = (first, bins, own.ctx.dev_alloc(MAXB * bins * 8))
                bufs.append(lin_bands[leg][2])
        if banded:
            root = legs["root"] = Leg(shape, n, names, ncl)
            check(lib.psdr_set_band_layout(root.ctx.h, NBANDS, n))
            for g in (1, NBANDS - 1):
                legs[f"region{g}"] = Leg(shape, n, in_band(shape, n, *banded_bounds(g, R, NBANDS, n, m1)), ncl)
        frame = 0
        for bi, F in enumerate(BATCHES):
            own.ctx.process_batch(d_raw, F, offset_bytes=frame * hb)
            if switch and bi == 1:
                check(lib.psdr_pack_band(own.ctx.h, F, 0, R, d_lin, R))
                own.ctx.synchronize()
                check(lib.psdr_demod_batch_from_band(own.ctx.h, d_lin, R, 0, R, F, frame))
                own.ctx.last_demod_frames = F
            else:
                own.ctx.demod_batch(frame)
            own.read(F)
            if not switch:
                frames += [Frame(own.ctx.read_spectrum(f), shape, n) for f in range(F)]
                check(lib.psdr_pack_band(own.ctx.h, F, 0, R, d_lin, R))
                for first, bins, d in lin_bands.values():
                    check(lib.psdr_pack_band(own.ctx.h, F, first, bins, d, bins))
                own.ctx.synchronize()
                for leg, (first, bins, d) in dict(lin_bands, linear=(0, R, d_lin)).items():
                    check(lib.psdr_demod_batch_from_band(legs[leg].ctx.h, d, bins, first, bins, F, frame))
                    legs[leg].ctx.last_demod_frames = F
                    legs[leg].read(F)
            if banded:
                root.ctx.process_batch(d_raw, F, offset_bytes=frame * hb)
                root.ctx.demod_batch(frame)
                root.read(F)
                root.ctx.synchronize()
                for g in (1, NBANDS - 1):
                    p, fs, fb, nb = region_of(root.ctx, g)
                    assert (fb, nb) == banded_bounds(g, R, NBANDS, n, m1)
                    leg = legs[f"region{g}"]
                    check(lib.psdr_demod_batch_from_band_region(leg.ctx.h, p, fs, fb, nb, F, frame))
                    leg.ctx.last_demod_frames = F
                    leg.read(F)
            frame += F
        return {k: v.rows() for k, v in legs.items()}, frames
    finally:
        if "own" in legs:
            legs["own"].ctx.synchronize()
            for d in bufs:
                legs["own"].ctx.dev_free(d)
        for v in legs.values():
            v.close()
        if old_env is None:
            os.environ.pop("PSDR_DEMOD_CHAIN", None)
        else:
            os.environ["PSDR_DEMOD_CHAIN"] = old_env


# ---- (a) truth ---------------------------------------------------------------------------------------------------------------

def record(row):
    d = os.path.join(ROOT, "build", "records")
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "layout_clients.jsonl"), "a") as f:
            f.write(json.dumps(row) + "\n")
    except OSError:
        pass


def check_window(shape, n, name, got, frames, worst):
    """the eight clients of one window against the float64 definitions on `frames`; worst: {family: largest error / bound}"""
    N, is_real = SHAPES[shape][:2]
    h, place = n // 2, placements(shape, n)[name]

    def note(fam, err, bound, tag):
        worst[fam] = max(worst.get(fam, 0.0), err / bound)
        assert err <= bound, f"{tag}: {err:.3e} > {bound:.3e}"

    def check_pwr(rows, T_pwr, T_fs, tag):
        assert not rows[2].any(), f"{tag}: NaN flags"
        for f in range(NF):
            assert abs(rows[1][f] - T_pwr[f]) <= pwr_tolerance(T_pwr[f], T_fs[f]), f"{tag} frame {f}: pwr {rows[1][f]} against {T_pwr[f]}"

    # SAM, and with it B (PSDR_IQ, AM) and the whole window's pwr; its precondition before anything is compared
    win = client_window(place, "SAM")
    T = SAM.truth_of(frames, slice_of, is_real, n, win, rms_of=rms_of)
    SAM.assert_signal_condition(T, (shape, n, name))
    sides = {k: SB.truth_of(frames, slice_of, is_real, n, win, SIDE[k], rms_of=rms_of) for k in ("SAMU", "SAML")}  # (asserts its own)
    binw = RATE / n
    for kind in ("SAM", "SAMU", "SAML"):
        rows, tag = got[(name, kind)], f"{shape} n {n} window {name} {kind}"
        Tk = T if kind == "SAM" else sides[kind]
        assert rows[0].shape == (NF, h) and rows[0].dtype == np.float32
        check_pwr(rows, T["pwr"], T["fwd_scale"], tag)
        for f in range(NF):
            bound = SAM.audio_bound(T, f) if kind == "SAM" else SB.audio_bound(Tk, f)
            note("sam" if kind == "SAM" else "sb", float(np.abs(rows[0][f] - Tk["audio"][f]).max()), bound, f"{tag} frame {f}")
        lv, off = rows[3], rows[4]
        for f in range(1, NF):  # test_gpu_sam_mode.py::test_carrier_record
            cm = np.abs(T["C"][f])
            if place[0] < place[1]:  # (a one-sided low-pass sees half the carrier's line: its estimate is the truth's alone)
                assert abs(off[f] - OFFSET_BINS * binw) <= 0.1 * binw, f"{tag} frame {f}: offset {off[f]} Hz"
            note("carrier", abs(off[f] - T["offset_hz"][f]), RATE / (2 * np.pi) * 4 * 2e-4 * (cm.max() / cm.min()) ** 2, f"{tag} frame {f} offset")
            note("carrier", abs(lv[f] - T["level"][f]), 2e-4 * T["level"][f], f"{tag} frame {f} level")
        if kind != "SAM":  # test_gpu_sam_sideband.py: the carrier is the both-sideband twin's
            assert_same_bits(rows[3:], got[(name, "SAM")][3:], f"{tag}: carrier records against the SAM client's", ("carrier level", "carrier offset"))
    # PSDR_IQ: test_gpu_iq_mode.py's bounds (check_iq), on the float64 baseband; AM: test_gpu_parity.py's, audio = |B|
    B = FT.baseband64_of(frames, slice_of, is_real, n, win, 0, NF)
    rows, tag = got[(name, "IQ")], f"{shape} n {n} window {name} IQ"
    assert rows[0].shape == (NF, h) and rows[0].dtype == np.complex64
    check_pwr(rows, T["pwr"], T["fwd_scale"], tag)
    for f in range(NF):
        IQM.check_iq(rows[0][f], B[f], f"{tag} frame {f}")
        worst["iq"] = max(worst.get("iq", 0.0), rel_l2(rows[0][f], B[f]) / 1e-4, float(np.abs(rows[0][f] - B[f]).max()) / (2e-4 * float(np.abs(B[f]).max())))
    rows, tag = got[(name, "AM")], f"{shape} n {n} window {name} AM"
    check_pwr(rows, T["pwr"], T["fwd_scale"], tag)
    for f in range(NF):
        a = np.abs(B[f])
        note("am", rel_l2(rows[0][f], a), 1e-4, f"{tag} frame {f} rel L2")
        note("am", float(np.abs(rows[0][f] - a).max()), 2e-4 * max(float(a.max()), 1e-30), f"{tag} frame {f}")
    # tuned clients: test_gpu_fine_tune.py's float64 anchor - the transform's 2e-4 and the rotator's 2e-6 of the frame's
    # largest sample; USB / LSB are twice a real part
    for kind in ("TUSB", "TLSB", "TIQ"):
        rows, tag = got[(name, kind)], f"{shape} n {n} window {name} {kind}"
        win = client_window(place, kind)
        Bt = FT.baseband64_of(frames, slice_of, is_real, n, FT.clipped(CLIENT_KINDS[kind][0], win), 0, NF)
        rot = Bt * FT.w64(FT.Phase(n).batch(win[1], NF))
        check_pwr(rows, T["pwr"], T["fwd_scale"], tag)
        for f in range(NF):
            scale = float(np.abs(Bt[f]).max())
            if kind == "TIQ":
                note("tuned", float(np.abs(rows[0][f] - rot[f]).max()), (2e-4 + 2e-6) * scale, f"{tag} frame {f}")
            else:
                note("tuned", float(np.abs(rows[0][f] - 2.0 * rot[f].real).max()), 2.0 * (2e-4 + 2e-6) * scale, f"{tag} frame {f}")


@pytest.mark.parametrize("case", LARGE, ids=[case_id(c) for c in LARGE])
def test_every_client_equals_its_definition_on_the_gpus_own_spectrum(case):
    shape, n, chain = case
    res, frames = run_case(shape, n, chain)
    assert len(frames) == NF
    worst = {}
    try:
        for name in placements(shape, n):
            check_window(shape, n, name, res["own"], frames, worst)
    finally:
        row = dict(test="truth", shape=shape, n=n, chain=chain, worst_error_over_bound={k: float(v) for k, v in worst.items()})
        record(row)
        print(json.dumps(row))


# ---- (b) bit identity across layouts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", LARGE + CONTROL, ids=[case_id(c) for c in LARGE + CONTROL])
def test_every_leg_gives_the_bits_of_the_contexts_own_spectrum(case):
    shape, n, chain = case
    res, _ = run_case(shape, n, chain)
    want = {"own", "linear", "band", "wrap"} | ({"root", "region1", f"region{NBANDS - 1}"} if SHAPES[shape][2] and not SHAPES[shape][1] else set())
    assert set(res) == want
    own = res["own"]
    assert len(own) == len(placements(shape, n)) * len(KINDS)
    for key, rows in own.items():
        assert rows[0].shape[0] == NF and np.abs(rows[0][1:]).max() > 0 and not rows[2].any(), key
    for leg in sorted(want - {"own"}):
        assert len(res[leg]) >= len(KINDS) and (leg not in ("linear", "root") or len(res[leg]) == len(own)), leg
        for key, rows in res[leg].items():
            assert_same_bits(rows, own[key], f"{case_id(case)}: leg {leg}, window {key[0]}, {key[1]}", row_names(key[1]))


# ---- (c) state across a change of source -----------------------------------------------------------------------------------

def test_state_carries_over_a_change_of_source():
    """psdr_demod_batch, then psdr_demod_batch_from_band on the packed spectrum, then psdr_demod_batch again: overlap-add,
    carrier, tuned and sideband tails and the tuned phase carry over - the bits of a run on psdr_demod_batch throughout"""
    ref, _ = run_case("iq20", 360, "1")
    got, _ = run_case("iq20", 360, "1", switch=True)
    assert set(got) == {"own"} and len(got["own"]) == len(ref["own"])
    for key, rows in got["own"].items():
        assert_same_bits(rows, ref["own"][key], f"window {key[0]}, {key[1]}", row_names(key[1]))

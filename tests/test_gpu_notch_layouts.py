"""Notched clients on every layout of the spectrum a deployed shape has (the pattern and the shapes of test_gpu_layout_clients.py).

Every notched load goes through SpecLayout::pos or the chain kernels' cached offsets, and the detector k_notch_detect computes
positions of its own; test_gpu_notch.py runs all of that on natural-order spectra only.  Here a notched USB, a notched SAM and
a notched IQ client - two manual notches each and auto-notch on - sit on every window of test_gpu_layout_clients.placements():
  own      psdr_demod_batch on the context's own spectrum: tile-major IQ (2^20, 2^21), fused real (2^21)
  linear   a context that never transforms, fed the whole spectrum packed linear: the NATURAL layout of the same values - the
           reference every other leg must equal bit for bit
  band     such a context fed one linear band with first_bin != 0; wrap: the band that wraps past the spectrum's end
  root     IQ: the banded root's own psdr_demod_batch (band regions in place); region1 / region3: receivers of one region
Rows, pwr, NaN flags, carrier records and psdr_read_notches (manual and automatic entries) of every batch are compared as bytes.

audio_rate is 1440 (n = 360) / 2880 (n = 720), so the detector's period is 4 frames: in the 9 frames (6 + 1 + 2) it evaluates
twice and its entries - the AM carrier on each USB / IQ window's centre bin stands far above 16 x mean - are in force from the
second batch on.  The n = 720 case runs k_demod_chain_iq_nz<720> and the n = 720 chain kernels with a notch."""
import ctypes as C
import os

import numpy as np
import pytest

import test_gpu_layout_clients as LC
from helpers import assert_same_bits, read_client, row_names, set_client_kind

pytestmark = pytest.mark.gpu

KINDS = ("USB", "SAM", "IQ")
CASES = [("iq20", 360, "1"), ("iq20", 360, "0"), ("real21", 360, "1"), ("iq21", 720, "1")]
PERIOD = 4


class Leg:
    def __init__(self, shape, n, names, max_clients):
        from phantomsdr_amd import AudioClient, Context
        N, is_real = LC.SHAPES[shape][:2]
        R = LC.result_size(shape)
        self.ctx = Context(N, is_real, R.bit_length() - 10, additional_size=n, audio_fft_size=n, audio_rate=PERIOD * n, input_format="s16",
                           max_batch=LC.MAXB, max_clients=max_clients)
        self.cl, self.got = {}, {}
        pl = LC.placements(shape, n)
        for name in names:
            l, kc, r = pl[name]
            for kind in KINDS:
                g = AudioClient(self.ctx)
                set_client_kind(g, kind)
                assert g.on_window_message(l, float(kc), r), (name, kind)
                g.set_notch(0, kc + 10.0, 3.0)   # inside the window
                g.set_notch(1, float(l), 4.0)    # straddling l
                g.set_auto_notch(True)
                self.cl[(name, kind)] = g
                self.got[(name, kind)] = []

    def read(self, F):
        for key, g in self.cl.items():
            rows = tuple(x[:F].copy() for x in read_client(g, key[1], LC.MAXB))
            self.got[key].append(rows + (np.array(g.notches(), np.int32),))

    def close(self):
        self.ctx.close()


def run_case(shape, n, chain):
    from phantomsdr_amd._lib import check
    from phantomsdr_amd.distributed import banded_bounds
    N, is_real, m1, _ = LC.SHAPES[shape]
    R, raw, names = LC.result_size(shape), LC.stream(shape, n), list(LC.placements(shape, n))
    ncl = len(names) * len(KINDS)
    banded = not is_real
    old_env = os.environ.get("PSDR_DEMOD_CHAIN")
    os.environ["PSDR_DEMOD_CHAIN"] = chain  # read by psdr_create
    legs, bufs = {}, []
    try:
        own = legs["own"] = Leg(shape, n, names, ncl)
        lib = own.ctx.lib
        d_raw = own.ctx.dev_alloc(raw.nbytes)
        bufs.append(d_raw)
        own.ctx.h2d(d_raw, raw)
        hb = own.ctx.half_frame_bytes()
        d_lin = own.ctx.dev_alloc(LC.MAXB * R * 8)
        bufs.append(d_lin)
        legs["linear"] = Leg(shape, n, names, ncl)
        lin_bands = {}
        for leg, (first, bins) in LC.bands(shape, n).items():
            legs[leg] = Leg(shape, n, LC.in_band(shape, n, first, bins), ncl)
            lin_bands[leg] = (first, bins, own.ctx.dev_alloc(LC.MAXB * bins * 8))
            bufs.append(lin_bands[leg][2])
        if banded:
            root = legs["root"] = Leg(shape, n, names, ncl)
            check(lib.psdr_set_band_layout(root.ctx.h, LC.NBANDS, n))
            for g in (1, LC.NBANDS - 1):
                legs[f"region{g}"] = Leg(shape, n, LC.in_band(shape, n, *banded_bounds(g, R, LC.NBANDS, n, m1)), ncl)
        frame = 0
        for F in LC.BATCHES:
            own.ctx.process_batch(d_raw, F, offset_bytes=frame * hb)
            own.ctx.demod_batch(frame)
            own.read(F)
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
                for g in (1, LC.NBANDS - 1):
                    p, fs, fb, nb = LC.region_of(root.ctx, g)
                    leg = legs[f"region{g}"]
                    check(lib.psdr_demod_batch_from_band_region(leg.ctx.h, p, fs, fb, nb, F, frame))
                    leg.ctx.last_demod_frames = F
                    leg.read(F)
            frame += F
        return {k: v.got for k, v in legs.items()}
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


@pytest.mark.parametrize("case", CASES, ids=LC.case_id)
def test_notched_clients_on_every_layout(case):
    shape, n, chain = case
    got = run_case(shape, n, chain)
    want_legs = {"own", "linear", "band", "wrap"} | (set() if LC.SHAPES[shape][1] else {"root", "region1", f"region{LC.NBANDS - 1}"})
    assert set(got) == want_legs
    ref = got["linear"]
    pl = LC.placements(shape, n)
    seen_auto = 0
    for leg, rows in got.items():
        assert rows, leg
        for key, per in rows.items():
            name, kind = key
            for bi, (a, b) in enumerate(zip(per, ref[key])):
                assert_same_bits(a, b, f"{shape} n {n} chain {chain}: leg {leg}, window {name}, {kind}, batch {bi}", row_names(kind) + ("notches",))
    # the manual entries are the ones set; the detector found the carrier of the USB and IQ windows inside the first batch, and
    # its entry stands in the later ones (so the second and third batch were demodulated with an automatic notch in force)
    for (name, kind), per in ref.items():
        l, kc, r = pl[name]
        for nz in per:
            assert nz[-1][0].tolist() == [kc + 9, kc + 12] and nz[-1][1].tolist() == [l - 2, l + 2]
        if kind != "SAM":
            for nz in per:
                assert nz[-1][2, 1] > nz[-1][2, 0] and l - 1 <= nz[-1][2, 0] and nz[-1][2, 1] <= r + 1, (name, kind, nz[-1])
                assert abs(int(nz[-1][2, 0]) + 1 - kc) <= 1, (name, kind, nz[-1])
            seen_auto += 1
        else:
            # the carrier sits on floor(audio_mid): protected, and nothing else in the window stands 16 x above the mean
            for nz in per:
                for k in (2, 3):
                    assert nz[-1][k, 1] == nz[-1][k, 0] or abs(int(nz[-1][k, 0]) + 1 - kc) > 3, (name, nz[-1])
    assert seen_auto == 2 * len(pl)

"""The served end of the path (phantomsdr_amd/csrc/fetch.hip, planned by fetchplan.h) on the branches no other file reaches: the
spans of IQ, SAM and squelch slots with gaps between them, in both forms of the row copies (one plain copy when the batch fills
max_batch, one pitched copy when it does not); a psdr_fetch_begin onto a set of the ring that is still in flight; and which
error a call answers with when it is wrong in two ways at once.  Every comparison is bit identity between what psdr_fetched_*
hand out and what psdr_read_* copy per client after a synchronise: no tolerance.

Rig: a 2^16-point IQ context, audio_fft_size 248, max_batch 4, eight client slots, s16 input, post chain on."""
import ctypes as C

import numpy as np
import pytest

from helpers import quantize_raw, synth_stream

pytestmark = pytest.mark.gpu

N, n, MAXB, SLOTS = 1 << 16, 248, 4, 8
H = n // 2
LEVELS = 7  # 2^16 bins down to the 1024 of the narrowest waterfall level
INVALID, STATE, NO_DATA = -1, -4, -7
OPEN, SHUT = (-200.0, -200.0, 1, 0), (200.0, 200.0, 1, 0)  # squelch settings no signal stays under / reaches
# slot -> (mode, window, squelch): IQ at 1 and 5 (a span of five for two clients), SAM at 3 and 6, squelch at 0 and 4; slot 2 is
# taken and given back before the first batch, slot 7 never taken
POPULATION = [("USB", (9000, 9000.0, 9061), OPEN), ("IQ", (20000, 20100.0, 20200), None), None, ("SAM", (30000, 30100.5, 30200), None),
              ("AM", (41000, 41100.0, 41200), SHUT), ("IQ", (50000, 50060.0, 50120), None), ("SAM", (7209, 7300.5, 7400), None)]


class Rig:
    def __init__(self, nframes, pcm16=False, post=True, max_clients=SLOTS):
        from phantomsdr_amd import Context, WaterfallClient
        raw = quantize_raw(synth_stream((nframes + 1) * (N // 2), False, seed=31, fft_size=N), "s16", False)
        self.ctx = Context(N, False, LEVELS, additional_size=n, audio_fft_size=n, input_format="s16", max_batch=MAXB, max_clients=max_clients,
                           max_waterfall_clients=2, skip_num=1)
        self.d = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.d, raw)
        if pcm16:
            self.ctx.set_option(self.ctx.OPT_POST_CHAIN_PCM16, 1)
        if post:
            self.ctx.set_post_chain(True)
        self.pcm16 = pcm16
        self.wf = WaterfallClient(self.ctx)
        self.wf.set_waterfall_range(2, 1000, 1700)
        self.frame = 0

    def add(self, mode, win, squelch=None):
        from phantomsdr_amd import AudioClient
        g = AudioClient(self.ctx)
        g.set_audio_demodulation(mode)
        g.set_audio_range(*win)
        if squelch:
            g.set_squelch(True, *squelch)
        return g

    def populate(self):
        """[(mode, client)] of POPULATION, each in the slot of its index"""
        cl, leave = [], []
        for i, p in enumerate(POPULATION):
            g = self.add(*(p or ("USB", (100, 100.0, 160))))
            assert g.id == i
            (leave if p is None else cl).append((p and p[0], g))
        for _, g in leave:  # (once the slots behind it are taken)
            g.on_close()
        return cl

    def batch(self, F):
        self.ctx.process_batch(self.d, F, offset_bytes=self.frame * self.ctx.half_frame_bytes())
        self.ctx.demod_batch(self.frame)
        self.ctx.waterfall_batch(self.frame)
        self.frame += F

    def read(self, cl, F):
        """every output of every client through psdr_read_*, behind a synchronise"""
        self.ctx.synchronize()
        out = []
        for mode, g in cl:
            rec = {}
            if mode == "IQ":
                rec["iq"], rec["pwr"], rec["nan"] = g.read_iq(MAXB)
            else:
                rec["audio"], rec["pwr"], rec["nan"] = g.read_audio(MAXB)
                rec["pcm"] = g.read_pcm(MAXB)
            if mode == "SAM":
                rec["car"] = np.stack(g.read_carrier(MAXB), axis=1)
            rec["sq"] = g.read_squelch(MAXB)
            assert all(len(v) == F for v in rec.values())
            out.append(rec)
        rows, _ = self.wf.read_waterfall()
        return out, rows

    def fetched(self, cl, F):
        """... and through psdr_fetched_*"""
        ctx, out = self.ctx, []
        for mode, g in cl:
            rec = {}
            if mode == "IQ":
                rows = [ctx.fetched_iq(g.id, f) for f in range(F)]
                rec["iq"] = np.stack([r[0] for r in rows])
            else:
                rows = [ctx.fetched_audio(g.id, f, pcm=True) for f in range(F)]
                rec["audio"] = np.stack([r[0] for r in rows])
                if self.pcm16:
                    assert all(r[3] is None for r in rows)  # (int16 rows: psdr_fetched_pcm16)
                    rec["pcm"] = np.stack([ctx.fetched_pcm16(g.id, f) for f in range(F)]).astype(np.int32)
                else:
                    rec["pcm"] = np.stack([r[3] for r in rows])
            rec["pwr"] = np.array([r[1] for r in rows], np.float32)
            rec["nan"] = np.array([r[2] for r in rows], np.int32)
            if mode == "SAM":
                rec["car"] = np.array([ctx.fetched_carrier(g.id, f) for f in range(F)], np.float32)
            rec["sq"] = np.array([ctx.fetched_squelch(g.id, f) for f in range(F)], np.int32)
            out.append(rec)
        return out, ctx.fetched_waterfall(self.wf.id)[0]

    def close(self):
        self.ctx.dev_free(self.d)
        self.ctx.close()


def assert_same(got, want, tag):
    (gc, gw), (wc, ww) = got, want
    assert len(gc) == len(wc)
    for i, (g, w) in enumerate(zip(gc, wc)):
        assert sorted(g) == sorted(w), (tag, i)
        for k in w:
            assert g[k].shape == w[k].shape and g[k].dtype == w[k].dtype and g[k].tobytes() == w[k].tobytes(), f"{tag}: client {i}: {k} differ"
    assert gw.shape == ww.shape and np.array_equal(gw, ww), f"{tag}: waterfall rows differ"


@pytest.mark.parametrize("pcm16", [False, True], ids=["pcm32", "pcm16"])
def test_spans_with_gaps_in_both_copy_forms(pcm16):
    batches = [4, 4, 4, 3, 3, 3]  # max_batch: plain copies; one short of it: pitched ones
    rig = Rig(sum(batches), pcm16=pcm16)
    try:
        cl = rig.populate()
        what = rig.ctx.FETCH_AUDIO | rig.ctx.FETCH_PCM | rig.ctx.FETCH_IQ | rig.ctx.FETCH_WATERFALL
        flags, alive = set(), 0
        for bi, F in enumerate(batches):
            rig.batch(F)
            rig.ctx.fetch_begin(what)
            rig.ctx.fetch_end()
            got = rig.fetched(cl, F)
            want = rig.read(cl, F)
            assert_same(got, want, f"batch {bi} of {F} frames")
            assert rig.ctx.fetched_iq_span() == (1, 5, 5 * F * H * 8)  # slots 1..5 for the IQ clients at 1 and 5
            assert want[1].shape == (F, 700)
            for (mode, g), rec in zip(cl, want[0]):
                flags |= {(g.id, int(v)) for v in rec["sq"]}
                alive += int(rec["iq" if mode == "IQ" else "audio"].any()) + int(mode == "SAM" and rec["car"].any())
        # both values of the flags went through the span's copy, and a slot without squelch inside the span reads open
        assert {(0, 1), (4, 0), (1, 1), (3, 1)} <= flags and (4, 1) not in flags
        assert alive == len(batches) * (len(cl) + 2), "rows that are all zero compare nothing"
    finally:
        rig.close()


def test_fetch_begin_onto_a_set_in_flight_gives_up_the_oldest_fetch():
    batches = [4, 3, 4, 3, 4]  # PSDR_FETCH_SETS + 1 fetches begun, none ended: the fifth takes the first one's set
    twin = Rig(sum(batches))
    try:
        cl = twin.populate()
        want = []
        for F in batches:
            twin.batch(F)
            want.append(twin.read(cl, F))
    finally:
        twin.close()
    rig = Rig(sum(batches))
    try:
        cl = rig.populate()
        what = rig.ctx.FETCH_AUDIO | rig.ctx.FETCH_PCM | rig.ctx.FETCH_IQ | rig.ctx.FETCH_WATERFALL
        for F in batches:
            rig.batch(F)
            rig.ctx.fetch_begin(what)
        for bi in range(1, 5):
            rig.ctx.fetch_end()
            assert_same(rig.fetched(cl, batches[bi]), want[bi], f"end {bi}: batch {bi + 1} of five")
            assert rig.ctx.lib.psdr_fetched_squelch(rig.ctx.h, 0, batches[bi], C.byref(C.c_int32(0))) == INVALID  # the set knows its batch's frames
        assert rig.ctx.lib.psdr_fetch_end(rig.ctx.h) == STATE  # four sets, four fetches in flight: nothing left
    finally:
        rig.close()


def test_which_error_a_call_answers_when_it_is_wrong_in_two_ways():
    """one row per function: (call, two faults -> the code of the one that is tested first)"""
    F = 3
    pa, pp, p16 = C.POINTER(C.c_float)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int16)()
    p8 = C.POINTER(C.c_int8)()
    fl, i32, ci, dbl, sz = C.c_float(0), C.c_int32(0), C.c_int(0), C.c_double(0), C.c_size_t(0)
    vp = C.c_void_p()
    buf = np.zeros((MAXB, n), np.int32)
    b = buf.ctypes.data_as(C.c_void_p)
    four = (C.c_int * 4)()
    rig = Rig(2 * F, post=False)
    try:
        L, h = rig.ctx.lib, rig.ctx.h
        usb = rig.add("USB", (9000, 9000.0, 9061))
        iq = rig.add("IQ", (20000, 20100.0, 20200))
        sam = rig.add("SAM", (30000, 30100.5, 30200))
        old = rig.add("AM", (41000, 41100.0, 41200))
        BAD = 99

        def table(rows):
            for name, call, want in rows:
                assert call() == want, (name, L.psdr_last_error())

        table([  # no batch yet, no fetch yet, no post chain
            ("fetch_begin: unknown bits, no batch", lambda: L.psdr_fetch_begin(h, 16 | rig.ctx.FETCH_AUDIO), INVALID),
            ("fetch_begin: no bits, no batch", lambda: L.psdr_fetch_begin(h, 0), INVALID),
            ("fetch_begin: no batch, PCM without the chain", lambda: L.psdr_fetch_begin(h, rig.ctx.FETCH_PCM), STATE),
            ("fetch_batch: no batch", lambda: L.psdr_fetch_batch(h), STATE),
            ("fetch_end: nothing in flight", lambda: L.psdr_fetch_end(h), STATE),
            ("read_audio: unknown id, no batch", lambda: L.psdr_read_audio(h, BAD, MAXB, None, None, None, None), INVALID),
            ("read_iq: unknown id, no batch", lambda: L.psdr_read_iq(h, BAD, MAXB, None, None, None, None), INVALID),
            ("read_carrier: unknown id, no batch", lambda: L.psdr_read_carrier(h, BAD, MAXB, None, None, None), INVALID),
            ("read_squelch: unknown id, no batch", lambda: L.psdr_read_squelch(h, BAD, MAXB, b, None), INVALID),
            ("read_pcm: unknown id, no chain", lambda: L.psdr_read_pcm(h, BAD, MAXB, b, None), INVALID),
            ("read_notches: unknown id, no batch", lambda: L.psdr_read_notches(h, BAD, four, four), INVALID),
            ("read_notches: no batch", lambda: L.psdr_read_notches(h, usb.id, four, four), STATE),
            ("audio_device_ptr: unknown id", lambda: L.psdr_audio_device_ptr(h, BAD, C.byref(vp), C.byref(vp)), INVALID),
            ("fetched_window: unknown id, no fetch", lambda: L.psdr_fetched_window(h, BAD, C.byref(ci), C.byref(dbl), C.byref(ci)), INVALID),
            ("fetched_audio: unknown id, no fetch", lambda: L.psdr_fetched_audio(h, BAD, 0, C.byref(pa), C.byref(fl), C.byref(i32), C.byref(pp)), INVALID),
            ("fetched_pcm16: unknown id, no fetch", lambda: L.psdr_fetched_pcm16(h, BAD, 0, C.byref(p16)), INVALID),
            ("fetched_iq: unknown id, no fetch", lambda: L.psdr_fetched_iq(h, BAD, 0, C.byref(pa), C.byref(fl), C.byref(i32)), INVALID),
            ("fetched_carrier: unknown id, no fetch", lambda: L.psdr_fetched_carrier(h, BAD, 0, C.byref(fl), C.byref(fl)), INVALID),
            ("fetched_squelch: unknown id, no fetch", lambda: L.psdr_fetched_squelch(h, BAD, 0, C.byref(i32)), INVALID),
            ("fetched_audio: no fetch, frame outside", lambda: L.psdr_fetched_audio(h, usb.id, 99, C.byref(pa), None, None, None), STATE),
            ("fetched_iq_span: no fetch", lambda: L.psdr_fetched_iq_span(h, C.byref(ci), C.byref(ci), C.byref(sz)), STATE),
            ("fetched_waterfall: no fetch, unknown id", lambda: L.psdr_fetched_waterfall(h, BAD, C.byref(p8), None, None, None, None), STATE),
        ])
        rig.batch(F)
        table([
            ("read_pcm: no chain, short buffer", lambda: L.psdr_read_pcm(h, usb.id, F - 1, b, None), STATE),  # post_on before the batch size
            ("fetch_begin: PCM without the chain", lambda: L.psdr_fetch_begin(h, rig.ctx.FETCH_AUDIO | rig.ctx.FETCH_PCM), STATE),
        ])
        rig.ctx.synchronize()
        rig.ctx.set_post_chain(True)
        rig.batch(F)
        old_id = old.id
        old.on_close()
        late = rig.add("USB", (100, 100.0, 160))  # in the slot of a client of the batch, and not one of it
        assert late.id == old_id
        table([
            ("read_audio: short buffer, not of the batch", lambda: L.psdr_read_audio(h, late.id, F - 1, None, None, None, None), INVALID),
            ("read_audio: not of the batch", lambda: L.psdr_read_audio(h, late.id, F, None, None, None, None), NO_DATA),
            ("read_audio: short buffer, an IQ client", lambda: L.psdr_read_audio(h, iq.id, F - 1, None, None, None, None), INVALID),
            ("read_audio: an IQ client", lambda: L.psdr_read_audio(h, iq.id, F, None, None, None, None), NO_DATA),
            ("read_iq: short buffer, no IQ client", lambda: L.psdr_read_iq(h, usb.id, F - 1, None, None, None, None), INVALID),
            ("read_iq: no IQ client", lambda: L.psdr_read_iq(h, usb.id, F, None, None, None, None), NO_DATA),
            ("read_carrier: short buffer, no SAM client", lambda: L.psdr_read_carrier(h, usb.id, F - 1, None, None, None), INVALID),
            ("read_carrier: no SAM client", lambda: L.psdr_read_carrier(h, usb.id, F, None, None, None), NO_DATA),
            ("read_carrier: not of the batch", lambda: L.psdr_read_carrier(h, late.id, F, None, None, None), NO_DATA),
            ("read_squelch: short buffer, not of the batch", lambda: L.psdr_read_squelch(h, late.id, F - 1, b, None), INVALID),
            ("read_squelch: not of the batch", lambda: L.psdr_read_squelch(h, late.id, F, b, None), NO_DATA),
            ("read_pcm: short buffer, not of the batch", lambda: L.psdr_read_pcm(h, late.id, F - 1, b, None), INVALID),
            ("read_pcm: an IQ client", lambda: L.psdr_read_pcm(h, iq.id, F, b, None), NO_DATA),
            ("read_notches: not of the batch", lambda: L.psdr_read_notches(h, late.id, four, four), NO_DATA),
            ("iq_device_ptr: unknown id", lambda: L.psdr_iq_device_ptr(h, BAD, C.byref(vp), C.byref(vp)), INVALID),
        ])
        assert L.psdr_fetch_begin(h, rig.ctx.FETCH_AUDIO | rig.ctx.FETCH_PCM) == 0 and L.psdr_fetch_end(h) == 0
        table([  # a set with audio and int32 PCM, without IQ rows and without waterfall rows
            ("fetched_window: not of the batch", lambda: L.psdr_fetched_window(h, late.id, C.byref(ci), C.byref(dbl), C.byref(ci)), NO_DATA),
            ("fetched_audio: not of the batch, frame outside", lambda: L.psdr_fetched_audio(h, late.id, 99, C.byref(pa), None, None, None), NO_DATA),
            ("fetched_audio: an IQ client, frame outside", lambda: L.psdr_fetched_audio(h, iq.id, 99, C.byref(pa), None, None, None), NO_DATA),
            ("fetched_audio: frame outside", lambda: L.psdr_fetched_audio(h, usb.id, F, C.byref(pa), None, None, None), INVALID),
            ("fetched_pcm16: int32 rows, not of the batch", lambda: L.psdr_fetched_pcm16(h, late.id, 0, C.byref(p16)), STATE),  # PCM-ness before membership
            ("fetched_pcm16: int32 rows, frame outside", lambda: L.psdr_fetched_pcm16(h, usb.id, 99, C.byref(p16)), STATE),
            ("fetched_iq: no IQ client, frame outside", lambda: L.psdr_fetched_iq(h, usb.id, 99, C.byref(pa), None, None), NO_DATA),
            ("fetched_iq: frame outside", lambda: L.psdr_fetched_iq(h, iq.id, F, C.byref(pa), None, None), INVALID),
            ("fetched_carrier: no SAM client, frame outside", lambda: L.psdr_fetched_carrier(h, usb.id, 99, C.byref(fl), C.byref(fl)), NO_DATA),
            ("fetched_carrier: an IQ client, frame outside", lambda: L.psdr_fetched_carrier(h, iq.id, 99, C.byref(fl), C.byref(fl)), NO_DATA),
            ("fetched_carrier: frame outside", lambda: L.psdr_fetched_carrier(h, sam.id, F, C.byref(fl), C.byref(fl)), INVALID),
            ("fetched_squelch: not of the batch, frame outside", lambda: L.psdr_fetched_squelch(h, late.id, 99, C.byref(i32)), NO_DATA),
            ("fetched_squelch: frame outside", lambda: L.psdr_fetched_squelch(h, iq.id, F, C.byref(i32)), INVALID),
            ("fetched_iq_span: no IQ rows", lambda: L.psdr_fetched_iq_span(h, C.byref(ci), C.byref(ci), C.byref(sz)), STATE),
            ("fetched_waterfall: no rows, unknown id", lambda: L.psdr_fetched_waterfall(h, BAD, C.byref(p8), None, None, None, None), STATE),
        ])
        # (an IQ client's rows are not asked for: the call answers, with no pointer)
        assert L.psdr_fetched_iq(h, iq.id, 0, C.byref(pa), C.byref(fl), C.byref(i32)) == 0 and not pa
        assert L.psdr_fetch_begin(h, rig.ctx.FETCH_AUDIO) == 0 and L.psdr_fetch_end(h) == 0
        table([("fetched_pcm16: no PCM, not of the batch", lambda: L.psdr_fetched_pcm16(h, late.id, 0, C.byref(p16)), STATE)])
        assert L.psdr_fetch_begin(h, rig.ctx.FETCH_WATERFALL) == 0 and L.psdr_fetch_end(h) == 0
        table([  # a set of waterfall rows alone
            ("fetched_audio: unknown id, no audio", lambda: L.psdr_fetched_audio(h, BAD, 0, C.byref(pa), None, None, None), INVALID),
            ("fetched_audio: no audio, frame outside", lambda: L.psdr_fetched_audio(h, usb.id, 99, C.byref(pa), None, None, None), STATE),
            ("fetched_window: no audio, not of the batch", lambda: L.psdr_fetched_window(h, late.id, C.byref(ci), C.byref(dbl), C.byref(ci)), STATE),
            ("fetched_squelch: no audio, not of the batch", lambda: L.psdr_fetched_squelch(h, late.id, 0, C.byref(i32)), STATE),
            ("fetched_iq_span: no IQ rows", lambda: L.psdr_fetched_iq_span(h, C.byref(ci), C.byref(ci), C.byref(sz)), STATE),
            ("fetched_waterfall: unknown id", lambda: L.psdr_fetched_waterfall(h, BAD, C.byref(p8), None, None, None, None), NO_DATA),
        ])
    finally:
        rig.close()

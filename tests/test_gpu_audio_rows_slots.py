"""The audio-row kernels, the squelch and the noise floor at high and sparse slots (the cases: tests/audio_rows_shapes.py).

A context of 600 slots: every slot is filled, then all but (0, 1, 63, 64, 255, 256, 598, 599) are removed - tests/
test_gpu_post_chain_forms.py's way of making holes - and two batches later one more client goes into slot 597, through the holes
below it.  Each neighbouring pair of slots holds a featured client - audio blanker, noise reduction, a two-section audio filter,
squelch and noise floor, the squelch referenced to the noise floor in one pair - and its twin without any of it; which of the two
comes first changes from pair to pair, so a state stride that is off by one slot lands on a twin.  The late client is featured.

Expected, without a tolerance: a featured client's rows are anb_stream, nr_stream and af_stream (the host table programs) over
its twin's rows and flags; its squelch flags are tests/squelch_model.py's over its own pwr bits (the relative one: the noise
floor's host walk over its pwr and W bits); and every reading - rows, pwr, flags, squelch, W, the blanker's totals, through the
read calls and through psdr_fetch_begin / _end - equals, byte for byte, what the same nine clients give in a dense context of 9
slots on the same stream and batches.  audio_rate is 4 x audio_fft_size: the noise floor evaluates every fourth frame."""
import functools

import numpy as np
import pytest

import anb_model as ANB
import audio_filter_model as AF
import audio_rows_shapes as S
import nr_model as NR
import test_noise_host as NH
from conftest import ROOT
from helpers import assert_same_bits, read_client, set_client_kind
from test_gpu_audio_blanker import cat, expect, same_words
from test_gpu_audio_rows_long import sections
from test_gpu_noise_floor import rel_flags
from test_gpu_squelch import STD, Gate, stream

pytestmark = pytest.mark.gpu

# n -> (max_batch, batches, the NaN sample's half-frame).  Every client's stream - the late one's too - passes the blanker's
# delay by two blocks and ends inside a block; one batch is a single frame
CASES = {360: (9, (1, 3, 9, 9, 5, 9), 20), 12: (80, (1, 3, 80, 80, 37, 80), 150)}
KINDS = ("USB", "AM", "FM", "SAM", "LSB")          # per pair, then the late client
FEATURED_FIRST = (True, False, True, False)       # slots 0, 64, 255, 599 are featured
RELATIVE_PAIR = 2                                 # slot 255: the squelch in dB above the noise floor
REL = (9.0, 6.0, 2, 1)
PERIOD = 4


class SCtx:
    def __init__(self, n, max_clients):
        from phantomsdr_amd import Context
        maxb, batches, nan_half = CASES[n]
        self.n = n
        self.ctx = Context(S.N, False, S.LEVELS, additional_size=n, audio_fft_size=n, audio_rate=PERIOD * n, input_format="f32", max_batch=maxb,
                           max_clients=max_clients)
        key = tuple(1 if (i // 5) % 3 else 0 for i in range(sum(batches) + 1))
        raw = stream(S.SHAPE, key=key, nan_half=nan_half)
        self.d = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.d, raw)
        self.frame = 0

    def configure(self, g, kind, featured, relative):
        set_client_kind(g, kind)
        L0 = S.L0
        g.set_audio_range(*((L0, L0 + 50.3, L0 + 100) if self.n > 100 else (L0 + 28, L0 + 30.3, L0 + 31 + self.n // 4)))
        if featured:
            g.set_audio_blanker("normal", *S.PARITY)
            g.set_noise_reduction("normal", *S.NRP)
            g.set_audio_filter(sections())
            g.set_noise_floor(True)
            g.set_squelch(True, *(REL if relative else STD))
            if relative:
                g.set_squelch_reference("noise")
        return g

    def batch(self, F):
        self.ctx.process_batch(self.d, F, offset_bytes=self.frame * self.ctx.half_frame_bytes())
        self.ctx.demod_batch(self.frame)
        self.frame += F

    def close(self):
        self.ctx.dev_free(self.d)
        self.ctx.close()


def roles():
    """[(kind, featured, relative)] of the nine clients in slot order: the four pairs, then the late client"""
    out = []
    for p, first in enumerate(FEATURED_FIRST):
        out += [(KINDS[p], first, first and p == RELATIVE_PAIR), (KINDS[p], not first, (not first) and p == RELATIVE_PAIR)]
    return out + [(KINDS[4], True, False)]


@functools.lru_cache(maxsize=None)
def run(n, sparse):
    """-> per client (slot order): dict(read=(rows, pwr, flags, ...), squelch, noise, fetched=(rows, pwr, flags, squelch, noise),
    counts) over the client's own batches, and the slots"""
    from phantomsdr_amd import AudioClient
    maxb, batches, _ = CASES[n]
    A = SCtx(n, S.SLOTS if sparse else len(S.KEPT) + 1)
    try:
        if sparse:
            everyone = [AudioClient(A.ctx) for _ in range(S.SLOTS)]
            assert [g.id for g in everyone] == list(range(S.SLOTS))
            for g in everyone:
                if g.id not in S.KEPT:
                    g.on_close()
            cl = [everyone[s] for s in S.KEPT]
        else:
            cl = [AudioClient(A.ctx) for _ in S.KEPT]
        spec = roles()
        for g, (kind, featured, relative) in zip(cl, spec):
            A.configure(g, kind, featured, relative)
        out = [dict(read=[], squelch=[], noise=[], fetched=[], counts=None) for _ in spec]
        for b, F in enumerate(batches):
            if b == S.LATE_BATCH:
                fillers = []
                while True:
                    g = AudioClient(A.ctx)
                    if g.id == (S.LATE_SLOT if sparse else len(S.KEPT)):
                        break
                    assert sparse and g.id < S.LATE_SLOT and g.id not in S.KEPT, g.id
                    fillers.append(g)
                for f in fillers:
                    f.on_close()
                cl.append(A.configure(g, *spec[-1]))
            A.batch(F)
            A.ctx.fetch_begin(A.ctx.FETCH_AUDIO)
            A.ctx.fetch_end()
            for g, (kind, _, _), o in zip(cl, spec, out):
                o["read"].append(read_client(g, kind, F))
                o["squelch"].append(g.read_squelch(F).copy())
                o["noise"].append(g.read_noise(F).copy())
                fa = [A.ctx.fetched_audio(g.id, f) for f in range(F)]
                o["fetched"].append((np.stack([a[0] for a in fa]), np.array([a[1] for a in fa], np.float32), np.array([a[2] for a in fa], np.int32),
                                     np.array([A.ctx.fetched_squelch(g.id, f) for f in range(F)], np.int32),
                                     np.array([A.ctx.fetched_noise(g.id, f) for f in range(F)], np.float32)))
        for g, (_, featured, _), o in zip(cl, spec, out):
            o["counts"] = g.audio_blanker_counts() if featured else None
        slots = [g.id for g in cl]
        return [dict(read=cat(o["read"]), squelch=np.concatenate(o["squelch"]), noise=np.concatenate(o["noise"]), fetched=cat(o["fetched"]), counts=o["counts"])
                for o in out], slots
    finally:
        A.close()


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_audio_rows_slots")


@pytest.fixture(scope="module")
def progs(tmp):
    return ANB.build_table(tmp, ROOT), NR.build_table(tmp, ROOT), AF.build_table(tmp, ROOT), NH.build(tmp, "noise_plan_table")


@pytest.mark.parametrize("n", S.SLOT_N)
def test_sparse_slots_give_the_host_programs_rows_and_the_models_flags(progs, tmp, n):
    anb, nr, af, noise_exe = progs
    res, slots = run(n, True)
    assert slots == list(S.KEPT) + [S.LATE_SLOT]
    maxb, batches, _ = CASES[n]
    h, sizes, spec = n // 2, list(batches), roles()
    for p, first in enumerate(FEATURED_FIRST):
        feat, twin = (res[2 * p], res[2 * p + 1]) if first else (res[2 * p + 1], res[2 * p])
        kind, slot = KINDS[p], slots[2 * p + (0 if first else 1)]
        trows, tflags = twin["read"][0], twin["read"][2]
        flagged = tflags != 0
        assert flagged.any() and not flagged.all()
        ((blanked, st, tr),) = expect(lambda jobs: ANB.run_streams(anb, tmp, jobs), [S.PARITY + (trows, tflags, sizes)])
        ((reduced, _, _),) = NR.run_streams(nr, tmp, [S.NRP + (blanked.reshape(-1), tflags, h, sizes)], rate=PERIOD * n)
        ((filtered, _),) = AF.run_blocked(af, tmp, [(sections(), reduced, tflags, h, sizes)])
        T = h * sum(sizes)
        assert T >= ANB.D + 2 * ANB.B and T % ANB.B != 0 and len(tr["centres"]) >= 8 and 1 in sizes
        S.record("gpu_slots", n=n, h=h, slot=slot, kind=kind, batches=sizes, slots=S.SLOTS, centres=len(tr["centres"]), unusable_blocks=S.unusable_blocks(tr))
        same_words(feat["read"][0], filtered.reshape(trows.shape), (n, slot, kind, "anb_stream, nr_stream, then af_stream"))
        assert feat["read"][0][flagged].tobytes() == trows[flagged].tobytes(), (n, slot, "a flagged frame's row was touched")
        assert_same_bits(feat["read"][1:], twin["read"][1:], f"n {n} slot {slot}: pwr, flags, carrier records", ("pwr", "nan flags", "carrier level", "carrier offset"))
        assert feat["counts"] == (int(st["impulses"]), int(st["samples"])) and feat["counts"][0] == len(tr["centres"]), (n, slot, feat["counts"])
        # the twin has none of it: open, no W
        assert twin["squelch"].all() and not twin["noise"].any()
        pwr, W = feat["read"][1], feat["noise"]
        assert not W[:PERIOD - 1].any() and (W[PERIOD - 1:2 * PERIOD] > 0).all() and W[2 * PERIOD:].any(), (n, slot, "W")
        if p == RELATIVE_PAIR:
            want = rel_flags(noise_exe, pwr, W, *REL)
        else:
            want = Gate(STD).batch(pwr)
        assert np.array_equal(feat["squelch"], want), (n, slot, np.flatnonzero(feat["squelch"] != want).tolist())
        print(f"n {n} slot {slot} {kind}: squelch {want.tolist()}")
        if n == 360:  # (the thresholds are tests/test_gpu_squelch.py's, set for its 100-bin window: at n = 12 the model alone is held)
            assert set(want.tolist()) == {0, 1}, (n, slot, "the gate never moved")
    # the late client's stream is long enough too
    late = h * sum(sizes[S.LATE_BATCH:])
    assert late >= ANB.D + 2 * ANB.B and late % ANB.B != 0 and res[-1]["counts"][0] >= 8


@pytest.mark.parametrize("n", S.SLOT_N)
def test_sparse_slots_read_and_fetch_what_a_dense_context_does(n):
    sparse, slots = run(n, True)
    dense, dslots = run(n, False)
    assert dslots == list(range(len(S.KEPT) + 1))
    for a, b, slot, (kind, featured, relative) in zip(sparse, dense, slots, roles()):
        tag = f"n {n} slot {slot} ({kind}, {'featured' if featured else 'twin'})"
        assert_same_bits(a["read"], b["read"], tag + ": read")
        assert_same_bits((a["squelch"], a["noise"]), (b["squelch"], b["noise"]), tag, ("psdr_read_squelch", "psdr_read_noise"))
        assert_same_bits(a["fetched"], b["fetched"], tag + ": fetched", ("rows", "pwr", "nan flags", "squelch", "noise"))
        assert a["counts"] == b["counts"], (tag, a["counts"], b["counts"])
        # the fetch answers what the read calls answer (pwr went through a C float: a NaN's payload is not compared)
        fr, fp, ff, fs, fw = a["fetched"]
        assert_same_bits((fr, ff, fs, fw), (a["read"][0], a["read"][2], a["squelch"], a["noise"]), tag + ": fetched against read", ("rows", "nan flags", "squelch", "noise"))
        assert np.array_equal(fp, a["read"][1], equal_nan=True), tag
        if featured:
            assert a["counts"][0] >= 8 and a["noise"].any(), tag

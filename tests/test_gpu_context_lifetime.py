"""A create / use / destroy cycle gives all of its device memory back: every lazily allocating path of a context (ingest
ring, fetch ring, post chain, waterfall detector carry, band layout, segment plans and seam pools of the fused real
pass, a one-device group) is exercised, the context is destroyed, and the device's free memory is compared from cycle
to cycle.  Through the Python binding only; nothing is provoked - the cycles only create and destroy."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import quantize_raw, synth_stream

pytestmark = pytest.mark.gpu

CYCLES = 4          # after one warm-up cycle (the runtime settles its own lazy pools in it)
ALLOWED_GROWTH = 0  # bytes per cycle: a destroyed context owes the device everything it took


def _levels(R, ws=1024):
    lv, cur = 0, R
    while cur >= ws:
        lv += 1
        cur //= 2
    return max(lv, 1)


@functools.lru_cache(maxsize=None)
def _raw(N, is_real, F):
    """F + 1 half-frames of s16 samples (made once: the cycles only create, use and destroy)"""
    return quantize_raw(synth_stream((F + 1) * (N // 2), is_real, seed=5, fft_size=N), "s16", is_real)


def _use_everything(N, is_real, F, n, nclients):
    """one context of N points: batch, ring, demodulation, post chain, waterfall detectors, fetch"""
    from phantomsdr_amd import AudioClient, Context, WaterfallClient
    R = N // 2 if is_real else N
    ctx = Context(N, is_real, _levels(R), additional_size=0 if is_real else n, audio_fft_size=n, audio_rate=12000,
                  input_format="s16", max_batch=F, max_clients=nclients, max_waterfall_clients=2, skip_num=3)
    try:
        raw = _raw(N, is_real, F)
        d = ctx.dev_alloc(raw.nbytes)
        ctx.h2d(d, raw)
        ctx.process_batch(d, F)
        ctx.process_batch(d, 1)            # (a second batch size: a second segment plan where the real pass is fused)
        ctx.dev_free(d)
        # the ingest ring and one batch out of it
        hb = ctx.half_frame_bytes()
        ctx.ring_create(F + 2)
        halves = raw.view(np.uint8).reshape(F + 1, hb)
        pinned = ctx.pinned_array((F + 1) * hb).reshape(F + 1, hb)
        pinned[:] = halves
        for i in range(F + 1):
            ctx.ring_write_async(i, pinned[i])
        ctx.process_ring(0, F)
        # audio clients, the post chain on
        clients = []
        for i in range(nclients):
            a = AudioClient(ctx)
            a.set_audio_demodulation(("USB", "LSB", "AM", "FM")[i % 4])
            a.set_audio_range(200 + 40 * i, 200.0 + 40 * i + n // 4, 200 + 40 * i + n // 2)
            clients.append(a)
        ctx.set_post_chain(True)
        ctx.demod_batch(0)
        # a waterfall client per detector, over two batches (the second one continues the run: the carry is used)
        wfs = []
        for det in ("peak", "mean"):
            w = WaterfallClient(ctx)
            w.set_waterfall_range(1, 64, 64 + 512)
            w.set_detector(det)
            wfs.append(w)
        ctx.waterfall_batch(0)
        ctx.fetch_begin(Context.FETCH_AUDIO | Context.FETCH_PCM | Context.FETCH_WATERFALL)
        ctx.process_ring(0, F)
        ctx.demod_batch(F)
        ctx.waterfall_batch(F)
        ctx.fetch_end()
        audio, _, _, pcm = ctx.fetched_audio(clients[0].id, 0, pcm=True)
        assert audio is not None and pcm is not None and audio.shape == pcm.shape == (n // 2,)
        rows, _, l, r = ctx.fetched_waterfall(wfs[0].id)
        assert rows.shape[1] == r - l and rows.shape[0] >= 1
        ctx.synchronize()
    finally:
        ctx.close()


def _band_layout(F):
    """psdr_set_band_layout replaces the two spectrum sets of a 2^20-point IQ context (the smallest it accepts)"""
    from phantomsdr_amd import Context
    N = 1 << 20
    ctx = Context(N, False, _levels(N), audio_fft_size=360, audio_rate=12000, input_format="s16", max_batch=F, max_clients=2)
    try:
        assert ctx.lib.psdr_set_band_layout(ctx.h, 4, 360) == 0
        p, sz, fb, nb = C.c_void_p(), C.c_size_t(), C.c_uint32(), C.c_uint32()
        assert ctx.lib.psdr_band_region(ctx.h, 1, C.byref(p), C.byref(sz), C.byref(fb), C.byref(nb)) == 0 and p.value
    finally:
        ctx.close()


def _group(N, is_real, F, n):
    """a one-device group, created and closed (psdr_group_destroy)"""
    from phantomsdr_amd import Group
    R = N // 2 if is_real else N
    g = Group([0], "clients", N, is_real, _levels(R), peer_copy=True, additional_size=0 if is_real else n, audio_fft_size=n,
              input_format="s16", max_batch=F, max_clients=4)
    try:
        g.client_add(300, 300.0 + n // 4, 300 + n // 2, "USB")
        g.synchronize()
    finally:
        g.close()


def _cycle(N, is_real, F, n, nclients):
    _use_everything(N, is_real, F, n, nclients)
    _band_layout(2)
    _group(N, is_real, F, n)


@pytest.mark.parametrize("N,is_real", [(1 << 14, False), (1 << 21, True)], ids=["iq_2p14", "real_fused_2p21"])
def test_cycles_give_their_memory_back(N, is_real):
    """Free device memory after each of CYCLES create / use / destroy cycles against the value after a warm-up cycle:
    growth per cycle is at most ALLOWED_GROWTH.  2^14-point IQ frames (the small shape), and 2^21-point real frames - the
    smallest the fused real pass takes: seam pools, segment flags and one segment plan per batch size."""
    import torch
    F, n, nclients = 8, 248, 5

    def free_now():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    _cycle(N, is_real, F, n, nclients)
    base = free_now()
    after = []
    for _ in range(CYCLES):
        _cycle(N, is_real, F, n, nclients)
        after.append(free_now())
    growth = [base - a for a in after]  # bytes the device has less than after the warm-up cycle
    print(f"free after warm-up {base}, less after cycle 1..{CYCLES}: {growth}, per cycle {growth[-1] / CYCLES:.0f} bytes")
    assert growth[-1] <= ALLOWED_GROWTH * CYCLES, growth

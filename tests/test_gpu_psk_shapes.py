"""The PSK31 decoder on the GPU at every hop length, at the shortest and at long frames, at the widest and the narrowest symbol window
(the contexts, the window and the batches: tests/decoder_shapes.py).

Cases (audio_rate, n, baud); H = rtty_hop(audio_rate), h = n / 2, Wn the symbol window in hops:
  ( 4000,  360, 62.5 )  H =  8, Wn =  8  the narrowest window; 22.5 hops per frame: two groups of 16 in a one-frame batch
  ( 7900,  360, 31.25)  H =  8, Wn = 32  the widest window: the LDS ring holds the 31 hops behind a group and the group's 16
  (12000, 2400, 31.25)  H = 16, h = 1200: 75 hops per frame, more than 64 - emit()'s frame range is empty for most hops
  (16000,  360, 31.25)  H = 32, the first rate of its class
  (48000,  512, 62.5 )  H = 64 = PSK_HMAX, h = 256: four hops per frame
  (12000,    4, 62.5 )  h = 2: eight frames per hop, so every hop ends several records, and batches that complete no hop
Input: tests/test_gpu_psk_decoder.py's builder with the rate as a parameter - unit noise, behind 0.75 s of it a carrier of amplitude 4
(1000 Hz above the window's lower edge, 700 Hz at 4000) under 1.5 s of idle reversals, `CQ de` and LF and then steady, one NaN sample
in the idle; at h = 2 a shorter stream: 0.1 s of noise, 1 s of idle, `e`.  Every case runs whole and split by
decoder_shapes.split_of(): one-frame batches, 5 and 6 frames in turn (each ends inside a hop wherever h is no multiple of H), a
third of the stream, and the rest.

Expected, without a tolerance: the two runs' rows and NaN flags are the same bits, and every frame's record, the text and its length
are tests/psk_model.py's records() on those rows and flags.  The conditions a run must meet to be worth comparing are evaluated on
the model's records."""
import functools

import numpy as np
import pytest

import decoder_shapes as S
import psk_model as M
from helpers import assert_same_bits, read_client
from test_gpu_psk_decoder import IDLE, LEAD, TAIL, frames_of as frames_for, psk_raw, rec_of, same_records

pytestmark = pytest.mark.gpu

CASES = ((4000, 360, 62.5), (7900, 360, 31.25), (12000, 2400, 31.25), (16000, 360, 31.25), (48000, 512, 62.5), (12000, 4, 62.5))
TEXT = "CQ de\n"
GROUP = 16  # PSK_GROUP (pskplan.h)


def cfg_of(rate, baud):
    """(at 4000 the rig's window is 1111 Hz wide: the carrier lies lower)"""
    return dict(carrier_hz=700.0 if rate < 7000 else 1000.0, baud=baud)


def input_of(n):
    """(text, seconds of noise alone, seconds of idle reversals, seconds of carrier)"""
    return ("e", 0.1, 1.0, 0.2) if n < 360 else (TEXT, LEAD, IDLE, TAIL)


def frames_of(rate, n, baud):
    text, lead, idle, tail = input_of(n)
    return frames_for(n, rate=rate, text=text, baud=baud, lead=lead, idle=idle, tail=tail)


@functools.lru_cache(maxsize=1)  # (the whole and the split run of a case, one behind the other)
def raw_of(rate, n, baud):
    text, lead, idle, _ = input_of(n)
    return psk_raw(n, frames_of(rate, n, baud), rate=rate, text=text, baud=baud, carrier=cfg_of(rate, baud)["carrier_hz"], lead=lead, idle=idle, nan_at=lead + 0.05)


@functools.lru_cache(maxsize=None)
def run(rate, n, baud, whole):
    nf = frames_of(rate, n, baud)
    batches = (nf,) if whole else S.split_of(nf, n // 2)
    A = S.open_ctx(rate, n, max(batches), raw_of(rate, n, baud))
    try:
        A.add("AM")
        g = A.add("USB")
        g.set_psk_decoder(True, **cfg_of(rate, baud))
        A.ctx.set_profiling(1)
        a, t = [], []
        for F in batches:
            A.batch(F)
            a.append(read_client(g, "USB", F)), t.append(g.read_psk(F))
        return S.cat(a), S.cat(t), g.read_psk_text(), A.ctx.kernel_stats(), batches
    finally:
        A.close()


@pytest.mark.parametrize("rate,n,baud", CASES)
def test_records_and_text_are_the_models_at_every_hop_window_and_frame_length(rate, n, baud):
    h, H = n // 2, M.hop_of(rate)
    nf = frames_of(rate, n, baud)
    (rows, _, nan), _, _, _, _ = run(rate, n, baud, True)
    assert rows.shape == (nf, h) and nan.any()
    want, wtext = M.records(rows, nan, h, rate, **cfg_of(rate, baud))
    for whole in (True, False):
        (r, _, f), t, (text, total), stats, batches = run(rate, n, baud, whole)
        assert_same_bits((r, f), (rows, nan), "the rows of the two runs", ("audio", "nan"))
        got = rec_of(t)
        ms, cnt = stats["audio_psk"]
        print(f"rate {rate} n {n} baud {baud} Wn {M.wn_of(baud, rate)} batches {batches[:12]}: text {text!r} errors {got['errors'][-1]} level {got['level'].max():.4g} "
              f"quality {got['quality'].max():.3f}; {cnt} launches, {1e3 * ms / max(cnt, 1):.1f} us each")
        same_records(got, want, (rate, n, baud, batches[:12]))
        assert text == wtext and total == len(wtext) == got["nchars"][-1] and cnt == len(batches)
    # what the split run must be to be worth comparing, on the model's records
    assert want["present"].any() and not want["present"].all() and 1 in batches
    if h % H:
        assert np.any(S.bounds(batches, h) % H), "no batch boundary inside a hop"
    if h > GROUP * H:
        assert any(u > GROUP for u in S.single_frame_units(batches, h, H)), "no one-frame batch completes more than a group of hops"
    if h < H:
        assert 0 in S.batch_units(batches, h, H), "no batch completes no hop"
    if n >= 360:
        assert wtext == TEXT and want["errors"][-1] == 0  # (at h = 2 the window is one bin wide: the model alone is held)

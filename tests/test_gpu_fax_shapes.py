"""The radiofax decoder on the GPU at every hop length, at the shortest and at long frames, near both ends of the samples a pixel may
hold (the contexts, the window and the batches: tests/decoder_shapes.py).

Cases (audio_rate, n, lpm, width); H = rtty_hop(audio_rate), h = n / 2:
  ( 7900,  360,  90,  256)  H =  8; Lq is no whole number of samples, so line ends wander through hops and chunks (900 / 1700 Hz:
                            the rig's window is 2194 Hz wide)
  (12000, 2400, 120, 1024)  h = 1200: more than one chunk per frame
  (16000,  360, 240, 2048)  H = 32; 1.95 samples per pixel
  (48000,  512,  60,  768)  H = 64; 62.5 samples per pixel, the accepted shape nearest the bound of 64
  (12000,    4, 240,  256)  h = 2: batches that complete no hop, no pixel and no line
FREE mode everywhere; the 240 and 120 lines per minute cases at n >= 360 also run the short PSDR_FAX_AUTO sequence of
tests/test_gpu_fax_decoder.py.  Every case runs whole and split by decoder_shapes.split_of().

Expected, without a tolerance: the two runs' rows and NaN flags are the same bits, and every frame's record, the kept lines, their
meta and the total are tests/fax_model.py's records() on those rows and flags.  The conditions a run must meet to be worth comparing
are evaluated on the model's records."""
import functools

import numpy as np
import pytest

import decoder_shapes as S
import fax_model as M
from helpers import assert_same_bits, read_client
from test_gpu_fax_decoder import fax_raw, frames_of, rec_of, same_records, tx_seconds

pytestmark = pytest.mark.gpu

CASES = ((7900, 360, 90.0, 256, "free"), (12000, 2400, 120.0, 1024, "free"), (12000, 2400, 120.0, 1024, "auto"), (16000, 360, 240.0, 2048, "free"),
         (16000, 360, 240.0, 2048, "auto"), (48000, 512, 60.0, 768, "free"), (12000, 4, 240.0, 256, "free"))
FREE_LINES = 4.6  # lines of image a FREE case sends


def cfg_of(rate, lpm, width, kind):
    c = dict(mode=M.AUTO if kind == "auto" else M.FREE, lpm=lpm, width=width)
    if rate < 8000:
        c.update(black_hz=900.0, white_hz=1700.0)
    if kind == "auto":
        c.update(start_blocks=4, phase_lines=3)
    return c


def tx_of(rate, lpm, kind):
    """the sender's parts, and the NaN sample's time: inside an image line"""
    if kind == "auto":
        return dict(), 0.3 + 1.5 + 9.5 * 60.0 / lpm, tx_seconds(lpm)
    tx = dict(lead=0.0, start_s=0.0, phasing=0, lines=5, stop_s=0.0, tail=0.0)
    return tx, 1.5 * 60.0 / lpm, FREE_LINES * 60.0 / lpm


@functools.lru_cache(maxsize=1)  # (the whole and the split run of a case, one behind the other)
def raw_of(rate, n, lpm, width, kind):
    c = cfg_of(rate, lpm, width, kind)
    tx, nan_at, seconds = tx_of(rate, lpm, kind)
    return fax_raw(rate, n, frames_of(rate, n, seconds), lpm, black_hz=c.get("black_hz", 1500.0), white_hz=c.get("white_hz", 2300.0), nan_at=nan_at, **tx)


@functools.lru_cache(maxsize=None)
def run(rate, n, lpm, width, kind, whole):
    nf = frames_of(rate, n, tx_of(rate, lpm, kind)[2])
    batches = (nf,) if whole else S.split_of(nf, n // 2)
    A = S.open_ctx(rate, n, max(batches), raw_of(rate, n, lpm, width, kind))
    try:
        A.add("AM")
        g = A.add("USB")
        g.set_fax_decoder(True, **cfg_of(rate, lpm, width, kind))
        A.ctx.set_profiling(1)
        a, t = [], []
        for F in batches:
            A.batch(F)
            a.append(read_client(g, "USB", F)), t.append(g.read_fax(F))
        return S.cat(a), S.cat(t), g.read_fax_lines(), A.ctx.kernel_stats(), batches
    finally:
        A.close()


@pytest.mark.parametrize("rate,n,lpm,width,kind", CASES)
def test_records_and_lines_are_the_models_at_every_hop_pixel_and_frame_length(rate, n, lpm, width, kind):
    h, H = n // 2, M.hop_of(rate)
    cfg = cfg_of(rate, lpm, width, kind)
    (rows, _, nan), _, _, _, _ = run(rate, n, lpm, width, kind, True)
    assert nan.any()
    want, wlines, wmeta = M.records(rows, nan, h, rate, **cfg)
    for whole in (True, False):
        (r, _, f), t, (lines, meta, total), stats, batches = run(rate, n, lpm, width, kind, whole)
        assert_same_bits((r, f), (rows, nan), "the rows of the two runs", ("audio", "nan"))
        got = rec_of(t)
        ms, cnt = stats["audio_fax"]
        print(f"rate {rate} n {n} lpm {lpm} width {width} {kind} batches {batches[:12]}: {total} lines, states {sorted(set(got['state']))}; {cnt} launches, "
              f"{1e3 * ms / max(cnt, 1):.1f} us each")
        same_records(got, want, (rate, n, lpm, width, kind, batches[:12]))
        assert total == len(wlines) == got["nlines"][-1] and cnt == len(batches)
        assert lines.tobytes() == wlines.tobytes() and meta.tobytes() == wmeta.tobytes()
    # what the split run must be to be worth comparing, on the model's records and the rule's integers
    Lq = M.lq_of(lpm, 0.0, rate)
    edges = S.bounds(batches, h).astype(np.int64)
    q = 65536 * edges + Lq
    assert len(wlines) >= 3, "fewer than 3 kept lines"
    if h % H:
        assert np.any(edges % H), "no batch boundary inside a hop"
    if kind == "free":  # (the origin stays 0: line and column of a stream position are the header's formulas)
        assert np.any(q % Lq >= 65536), "no batch boundary inside a line"
        col = (q % Lq) * width // Lq
        col_before = ((q - 65536) % Lq) * width // Lq
        assert np.any(col == col_before), "no batch boundary inside a pixel"
        first, last = np.flatnonzero(nan)[[0, -1]]
        assert (65536 * first * h) // Lq == (65536 * (last + 1) * h - 1) // Lq and (65536 * first * h) % Lq > 0, "no flagged frame inside a line"
    else:
        st = want["state"]
        assert [int(s) for i, s in enumerate(st) if i == 0 or s != st[i - 1]] == [M.IDLE, M.PHASING, M.IMAGE, M.IDLE] and want["image"][-1] == 1
    if h < H:
        assert 0 in S.batch_units(batches, h, H), "no batch completes no hop"

"""What the GPU tests of the ingest-ring blanker share (tests/test_gpu_blanker.py at the smallest shapes, tests/
test_gpu_blanker_shapes.py at the others): one context with a ring, the stream fed call by call and held against
tests/nb_model.py byte for byte, and the twin context that never heard of the blanker.  Without a Stream (nb_model.stream) the
shape and the stream are those of nb_model.fixture()."""
import ctypes as C

import numpy as np

import nb_model as M


class Rig:
    """one context with a ring of NHALVES halves; feed() writes the halves a call needs, then processes"""

    def __init__(self, fmt, is_real, st=None):
        from phantomsdr_amd import Context
        self.fmt, self.is_real = fmt, is_real
        self.nhalves, max_batch, N = (st.nhalves, st.max_batch, st.N) if st else (M.NHALVES, M.MAX_BATCH, M.shape(is_real))
        self.ctx = Context(N, is_real, 3, input_format=fmt, max_batch=max_batch, max_clients=1)
        self.hb = self.ctx.half_frame_bytes()
        self.ctx.ring_create(self.nhalves)
        self.pinned = [self.ctx.pinned_array(self.hb) for _ in range(self.nhalves)]
        self.written = -1  # the highest half written so far

    def close(self):
        self.ctx.close()

    def read_frames(self, first, n, keep=None):
        """-> {frame: (spectrum, pyramid)} as bytes, of the last call's frames (those of `keep` if given)"""
        return {first + f: (self.ctx.read_spectrum(f).view(np.uint8).copy(), self.ctx.read_quantized(f).copy())
                for f in range(n) if keep is None or first + f in keep}

    def call(self, halves, first, n):
        """-> (spectra, pyramids) of the call's frames, as bytes"""
        self.feed(halves, first, n)
        return ([self.ctx.read_spectrum(f).view(np.uint8).copy() for f in range(n)], [self.ctx.read_quantized(f).copy() for f in range(n)])

    def feed(self, halves, first, n):
        for h in range(max(first, self.written + 1), first + n + 1):
            self.ctx.ring_wait(h)  # (the pinned buffer of the slot is free again)
            self.ctx.synchronize()
            self.pinned[h % self.nhalves][:] = halves[h].view(np.uint8)
            self.ctx.ring_write_async(h, self.pinned[h % self.nhalves])
            self.written = h
        self.ctx.process_ring(first, n)

    def ring_half(self, h):
        return self.ctx.ring_read(h, M.DTYPE[self.fmt])

    def mirror(self):
        ptrs = (C.c_void_p * 6)()
        assert self.ctx.lib.psdr_debug_blanker_ptrs(self.ctx.h, ptrs) == 0
        out = np.empty(self.hb, np.uint8)
        self.ctx.d2h(out, C.c_void_p(ptrs[5]))
        return out.view(M.DTYPE[self.fmt])

    def blanker_ptrs(self):
        ptrs = (C.c_void_p * 6)()
        assert self.ctx.lib.psdr_debug_blanker_ptrs(self.ctx.h, ptrs) == 0
        return [ptrs[k] for k in range(5)]


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def run_blanked(fmt, is_real, guard, calls, db=M.THRESHOLD_DB, planted=True, st=None, keep=None):
    """the stream through a context with the blanker on, call by call against the model: ring bytes, counts, levels.
    -> (frames' spectra and pyramids, the model-blanked stream, counts).  st: a Stream in place of the fixture (calls that move
    forward only); keep: the frames whose spectra and pyramids are read, all of them if None"""
    if st is None:
        halves, _ = M.fixture(fmt, is_real, guard, planted=planted)
        model, nb = [h.copy() for h in halves], M.Blanker(fmt, is_real, db, guard)
    else:
        halves, (model, seen), done = st.halves, M.run_model(st, calls, db, guard), set()
    rig = Rig(fmt, is_real, st)
    frames, counts = {}, {}
    try:
        rig.ctx.ring_set_blanker(True, db, guard)
        for first, n in calls:
            if st is None:
                want = nb.process(model, first, n)
            else:
                want = {h: seen[h] for h in range(first, first + n + 1) if h not in done}  # (the model of the whole stream is shared)
                done.update(want)
            rig.feed(halves, first, n)
            frames.update(rig.read_frames(first, n, keep))
            for h in range(first, first + n + 1):
                assert same(rig.ring_half(h), model[h]), (first, n, h)
                got = rig.ctx.ring_read_blanker(h)
                if h in want:
                    assert got is not None and got[0] == want[h][0] and same(got[1], want[h][1]), (h, got, want[h])
                    counts[h] = got[0]
                else:
                    assert got is None, (h, got)  # blanked by an earlier call: PSDR_ERR_NO_DATA
                if h % rig.nhalves == 0:
                    assert same(rig.mirror(), model[h]), (first, n, h)  # both copies of the slot-0 half
            assert rig.ctx.ring_read_blanker(first + n + 1) is None
    finally:
        rig.close()
    return frames, model, counts


def run_plain(fmt, is_real, halves, calls, st=None, keep=None):
    """a context that never heard of the blanker, fed `halves`"""
    rig = Rig(fmt, is_real, st)
    frames = {}
    try:
        for first, n in calls:
            rig.feed(halves, first, n)
            frames.update(rig.read_frames(first, n, keep))
            for h in range(first, first + n + 1):
                assert same(rig.ring_half(h), halves[h])
        assert not any(rig.blanker_ptrs())  # assertion 8: no blanker allocation
    finally:
        rig.close()
    return frames

"""What a context shows through the ABI against the plan it was created from (phantomsdr_amd/csrc/createplan.h, asked through
tests/create_plan_table.py): the smallest context of each branch of shape_plan with max_batch = 2 - IQ 2^12 (natural order), IQ
2^20 (tile-major, the family that accepts bands), real 2^13 (three-pass), real 2^21 (fused, octets).  Nothing is transformed:
the frame-to-frame distances of the device pointers are the plan's strides, the sizes are the plan's, a band layout gives the
regions band_plan names, and a rejected config comes back with create_check's code and text."""
import ctypes as C

import pytest

import create_plan_table as T

pytestmark = pytest.mark.gpu

F = 2
BITS = {"u8": 8, "s16": 16, "f32": 32}
CONTEXTS = {"iq12": (1 << 12, 0, "u8"), "iq20": (1 << 20, 0, "s16"), "real13": (1 << 13, 1, "f32"), "real21": (1 << 21, 1, "s16")}
NBANDS, HALO = 2, 360


@pytest.mark.parametrize("name", CONTEXTS)
def test_context_shows_what_the_plan_says(name):
    from phantomsdr_amd import Context
    N, is_real, fmt = CONTEXTS[name]
    plan = T.plan(N, is_real, levels=5, audio=360, batch=F, clients=2)
    s = plan["shape"]
    ctx = Context(N, is_real, 5, audio_fft_size=360, input_format=fmt, max_batch=F, max_clients=2)
    try:
        L, p, q, sz = ctx.lib, [C.c_void_p(), C.c_void_p()], [C.c_void_p(), C.c_void_p()], C.c_size_t()
        assert ctx.half_frame_bytes() == (N // 2) * (1 if is_real else 2) * BITS[fmt] // 8
        for f in range(F):
            assert L.psdr_spectrum_device_ptr(ctx.h, f, C.byref(p[f]), C.byref(sz)) == 0
            assert sz.value == (N // 2 + 1 if is_real else N)
            assert L.psdr_quantized_device_ptr(ctx.h, f, C.byref(q[f]), C.byref(sz)) == 0
            assert sz.value == int(s["q_len"])
        assert p[1].value - p[0].value == 8 * int(s["spec_stride"]) and q[1].value - q[0].value == int(s["q_stride"])
        if name != "iq20":
            assert L.psdr_set_band_layout(ctx.h, NBANDS, HALO) == -6
            return
        (b,) = T.blocks(T.run(T.program(), "%s\n%s\nband %d %d\n" % (T.env(), T.cfg(N, 0, levels=5, audio=360, batch=F, clients=2), NBANDS, HALO)))
        band, lay = b["band"][0], b["lay"][1]
        assert L.psdr_set_band_layout(ctx.h, NBANDS, HALO) == 0
        fs, fb, nb, reg = C.c_size_t(), C.c_uint32(), C.c_uint32(), [C.c_void_p(), C.c_void_p()]
        for g in range(NBANDS):
            assert L.psdr_band_region(ctx.h, g, C.byref(reg[g]), C.byref(fs), C.byref(fb), C.byref(nb)) == 0
            assert fs.value == nb.value == int(band["frame_stride"]) and fb.value == g * int(band["Lb"]) * int(s["M1"])
        assert reg[1].value - reg[0].value == 8 * int(band["region"]) == 8 * int(lay["band_stride"]) == 8 * F * int(band["frame_stride"])
    finally:
        ctx.close()


def test_rejected_configs_answer_with_create_checks_code_and_text():
    from phantomsdr_amd import Context, PsdrError
    cases = [dict(N=2048, kw={}), dict(N=4096, kw=dict(audio_fft_size=362)), dict(N=4096, kw=dict(max_batch=0, waterfall_size=-1))]
    for c in cases:
        kw = c["kw"]
        line = T.cfg(c["N"], 0, levels=1, audio=kw.get("audio_fft_size", 0), batch=kw.get("max_batch", 1), wf_size=kw.get("waterfall_size", 0))
        (b,) = T.blocks(T.run(T.program(), line + "\n"))
        want = b["check"][0]
        assert int(want["code"]) < 0 and want["msg"]
        with pytest.raises(PsdrError) as e:
            Context(c["N"], 0, 1, **kw).close()
        assert e.value.code == int(want["code"]) and str(e.value).endswith(": " + want["msg"])

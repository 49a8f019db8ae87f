"""k_audio_fax's budget: like the other audio-row kernels it must fit beside a pass's work-group - at most 80 VGPRs
(tests/test_cw_code_object.py), no scratch, no AGPRs - and inside the 15 KiB of LDS an FFT pass leaves free on a CU.
Read from the gfx950 code object of the built library: kernel metadata only."""
import codeobj


def test_k_audio_fax_fits_beside_a_pass():
    md = {k: v for k, v in codeobj.kernel_metadata().items() if "k_audio_fax" in k}
    assert len(md) >= 1, sorted(md)
    for name, m in md.items():
        print(name, m)
        assert m["vgpr"] <= 80 and m["scratch"] == 0 and m["agpr"] == 0 and m["lds"] <= 15 * 1024, (name, m)

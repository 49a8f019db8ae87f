"""k_audio_filter's budget: like the column tail and the chain kernel it must fit beside a pass's work-group - at most
80 VGPRs (what cfg2's second pass leaves per SIMD lane), no scratch, no AGPRs, one wave per work-group.  Read from
the gfx950 code object of the built library."""
import codeobj


def test_k_audio_filter_fits_beside_a_pass():
    md = {k: v for k, v in codeobj.kernel_metadata().items() if "k_audio_filter" in k}
    assert len(md) == 2, sorted(md)  # the 16-byte and the 8-byte form
    for name, m in md.items():
        print(name, m)
        assert m["vgpr"] <= 80 and m["scratch"] == 0 and m["agpr"] == 0 and m["wg"] == 64 and m["lds"] == 0, (name, m)

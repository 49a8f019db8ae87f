"""The band scan's kernels run on the side stream beside the FFT passes' work-groups: no scratch, no AGPRs, few
enough registers that they never cost a pass an occupancy step (at most 64 VGPRs), and no LDS but k_scan_mark's block
scan (4 KiB, one work-group of 1024).  Read from the gfx950 code object of the built library: kernel metadata only.  The numbers
found are the ones written into DESIGN 3.19."""
import codeobj

DESIGN = {  # kernel -> (vgpr, lds, work-group)
    "k_scan_trace<16>": (38, 0, 256), "k_scan_trace<8>": (44, 0, 256), "k_scan_trace<4>": (25, 0, 256), "k_scan_trace<2>": (14, 0, 256),
    "k_scan_trace<1>": (10, 0, 256), "k_scan_floor": (11, 0, 256), "k_scan_hot": (10, 0, 256), "k_scan_mark": (20, 4096, 1024),
    "k_scan_emit": (16, 0, 256),
}


def test_scan_kernels_fit_beside_a_pass():
    md = {k: v for k, v in codeobj.kernel_metadata().items() if "k_scan_" in k}
    assert len(md) == len(DESIGN), sorted(md)  # five forms of the trace, four kernels of the evaluation
    for name, m in md.items():
        print(name, m)
        assert m["scratch"] == 0 and m["agpr"] == 0 and m["vgpr"] <= 64, (name, m)
        key = [k for k in DESIGN if k + "(" in name]
        assert len(key) == 1, name
        assert (m["vgpr"], m["lds"], m["wg"]) == DESIGN[key[0]], (name, m, "DESIGN.md 3.19 says otherwise")

// pass1.hip - launchers of the first FFT pass (fft_pass.h: convert + Hann + column transform + inter-pass twiddle)
#include "ctx.h"
#include "fft_pass.h"

namespace psdr {

constexpr size_t P1_LDS_MAX = 160 * 1024 - 256;  // dynamic LDS of a pass-1 work-group (the kernel's own words beside it)

template <typename K>
static int launch_pass1_k(psdr_ctx *c, K kern, int L, int T, size_t lds, const Pass1Args &a, unsigned blocks) {
    if (lds > P1_LDS_MAX)  // (a dispatch asking for more faults the queue)
        return fail(PSDR_ERR_UNSUPPORTED, "pass 1 L=%d T=%d M2=%d needs %zu bytes of LDS", L, T, a.M2, lds);
    // (per context = per device: the attribute is a property of the function ON a device)
    if (c->lds_attr_done.insert((const void *)kern).second)
        HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P1_LDS_MAX));
    ProfScope ps(c, K_PASS1, c->stream);
    // persistent: as many work-groups per CU as their LDS admits (a 128 KiB tile: one)
    const unsigned grid = persistent_grid(c, blocks, lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(L * T / 32), lds, c->stream, a);
    HIPCHK(hipGetLastError());
    return PSDR_OK;
}
template <int L, int T, int SB, bool PAIR = false, int CP = 8>
static int launch_pass1_t(psdr_ctx *c, const Pass1Args &a, unsigned blocks) {
    // tile + W_L (= first twiddle factor) + second twiddle factor (M2 entries)
    const size_t lds = (size_t)L * T * sizeof(cf) + (size_t)L * sizeof(cf) + (size_t)a.M2 * sizeof(cf);
    return launch_pass1_k(c, k_fft_pass1<L, T, SB, PAIR, CP>, L, T, lds, a, blocks);
}
// 2048 x 2048 (2^22 IQ, 2^23 real): tile, stage table and the 2048-entry second factor are 160 KiB - that factor comes from L2
template <int SB>
static int launch_pass1_l2tb(psdr_ctx *c, const Pass1Args &a, unsigned blocks) {
    const size_t lds = (size_t)2048 * 8 * sizeof(cf) + (size_t)2048 * sizeof(cf);
    return launch_pass1_k(c, k_fft_pass1_l2tb<2048, 8, SB>, 2048, 8, lds, a, blocks);
}

#define P1CASE(L_, T_)                                                   \
    if (L == L_ && T == T_) {                                            \
        if (sb == 2) return launch_pass1_t<L_, T_, 2>(c, a, blocks);     \
        if (sb == 4) return launch_pass1_t<L_, T_, 4>(c, a, blocks);     \
        return launch_pass1_t<L_, T_, 8>(c, a, blocks);                  \
    }
#define P1PAIR(L_, T_)                                                         \
    if (L == L_ && T == T_) {                                                  \
        if (sb == 2) return launch_pass1_t<L_, T_, 2, true>(c, a, blocks);     \
        if (sb == 4) return launch_pass1_t<L_, T_, 4, true>(c, a, blocks);     \
        return launch_pass1_t<L_, T_, 8, true>(c, a, blocks);                  \
    }
// sb: bytes per complex sample slot of the raw image (2, 4, 8); pair: the real-input form feeding k_fft_pass2_real
int launch_pass1(psdr_ctx *c, int L, int T, int sb, const Pass1Args &a, unsigned blocks, bool pair) {
    if (pair) {
        if (L == 1024 && T == 16 && a.l2t2 == 3) {  // pass-2 tiles of 8 rows = four (row, mirror row) couples: 2048-point rows (1024 x 2048)
            if (sb == 2) return launch_pass1_t<1024, 16, 2, true, 4>(c, a, blocks);
            if (sb == 4) return launch_pass1_t<1024, 16, 4, true, 4>(c, a, blocks);
            return launch_pass1_t<1024, 16, 8, true, 4>(c, a, blocks);
        }
        P1PAIR(1024, 16)
        P1PAIR(2048, 8)
        return fail(PSDR_ERR_UNSUPPORTED, "no paired pass-1 kernel for L=%d T=%d", L, T);
    }
    P1CASE(64, 64)
    P1CASE(128, 64)
    P1CASE(128, 128)
    P1CASE(256, 64)
    P1CASE(512, 32)
    P1CASE(1024, 16)
    P1CASE(1024, 8)
    if (L == 2048 && T == 8 && a.M2 == 2048) {
        if (sb == 2) return launch_pass1_l2tb<2>(c, a, blocks);
        if (sb == 4) return launch_pass1_l2tb<4>(c, a, blocks);
        return launch_pass1_l2tb<8>(c, a, blocks);
    }
    P1CASE(2048, 8)
    return fail(PSDR_ERR_UNSUPPORTED, "no pass-1 kernel for L=%d T=%d", L, T);
}

}  // namespace psdr

/* Stand-alone check of the oracle's post-chain pieces at the signal edges, for a host sanitizer build:
 *   cc -O1 -g -fsanitize=undefined,float-cast-overflow -fno-sanitize-recover=all -fopenmp edge_check.c psdr_oracle.c -lm -ldl -lpthread
 * (make -C oracle edge_check runs it).  orc_float_to_int16 over +-0, denormals, every boundary of the conversion with its
 * float neighbours, the last values inside int32 and far beyond it up to +-Inf; orc_agc_process through noise-like level,
 * digital silence (the gain climbs towards 2e9), a burst behind the silence, a reset in mid-silence and denormals.  Exit
 * status 0 and no report: nothing undefined was executed, and the conversion kept its contract. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "psdr_oracle.h"

static int contract(float x) {
    float t = fmaf(x, 16384.0f, 32768.5f);
    if (t >= 65536.0f) return 32767;
    if (t < 0.0f) return -32768;
    return (int)t - 32768;
}

int main(void) {
    static const double at[] = {-1.0, -0.5, 0.0, 0.5, 1.0, 32768.0, 65534.5, 65535.0, 65535.5, 65536.0, 65536.5};
    static const float mags[] = {0.0f, 1.4e-45f, 1e-39f, 1.1754942e-38f, 1.1754944e-38f, 1e-30f, 1e-10f, 1e-5f, 6.1e-5f, 1e-3f, 0.1f, 1.0f, 1.99993f,
                                 2.0f, 3.0f, 10.0f, 1e3f, 1e5f, 131069.98f, 131070.0f, 131072.0f, 131073.98f, 131074.0f, 131080.0f, 2e5f, 1e6f,
                                 1e10f, 1e20f, 3.4e38f, INFINITY};
    float x[256];
    int32_t out[256];
    size_t n = 0;
    for (size_t k = 0; k < sizeof(at) / sizeof(at[0]); k++) {
        float v = (float)((at[k] - 32768.5) / 16384.0);
        x[n++] = nextafterf(v, -INFINITY);
        x[n++] = v;
        x[n++] = nextafterf(v, INFINITY);
    }
    for (size_t k = 0; k < sizeof(mags) / sizeof(mags[0]); k++) {
        x[n++] = mags[k];
        x[n++] = -mags[k];
    }
    orc_float_to_int16(x, out, 16384.0f, n);
    int bad = 0;
    for (size_t i = 0; i < n; i++)
        if (out[i] != contract(x[i])) {
            printf("orc_float_to_int16(%a) = %d, the contract says %d\n", x[i], out[i], contract(x[i]));
            bad++;
        }
    /* the AGC at 12 kHz, blocks of 180: level 4e-3, silence, level 4e-4, long silence with a reset, a burst, denormals, recovery */
    static const struct { int blocks; float amp; } script[] = {{18, 4e-3f}, {8, 0.f}, {3, 4e-4f}, {22, 0.f}, {3, 4.f}, {18, 4e-39f}, {6, 4e-3f}};
    orc_agc *a = orc_agc_create(0.2f, 50.0f, 300.0f, 200.0f, 12000.0f);
    float blk[180], peak = 0.f;
    long t = 0;
    int it = 0;
    for (size_t s = 0; s < sizeof(script) / sizeof(script[0]); s++)
        for (int b = 0; b < script[s].blocks; b++, it++) {
            if (it == 31) orc_agc_reset(a);
            for (int i = 0; i < 180; i++, t++) blk[i] = script[s].amp * cosf(0.62831853f * (float)(t % 10) + 0.3f);
            orc_agc_process(a, blk, 180);
            for (int i = 0; i < 180; i++) {
                if (!isfinite(blk[i])) bad++;
                if (fabsf(blk[i]) > peak) peak = fabsf(blk[i]);
            }
            orc_float_to_int16(blk, out, 16384.0f, 180);
            for (int i = 0; i < 180; i++) bad += out[i] != contract(blk[i]);
        }
    orc_agc_destroy(a);
    if (!(peak * 16384.0f > 2147483648.0f)) {
        printf("the AGC's output never left int32 (peak %g): the script did not reach its regime\n", peak);
        bad++;
    }
    printf("%zu conversions, %d AGC blocks, largest AGC output %g: %s\n", n, it, peak, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

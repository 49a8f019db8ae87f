// Runs the AGC profile's host side (phantomsdr_amd/csrc/agcplan.h, and postplan.h's coefficient function) over a script from
// stdin.  Plain host C++: tests/test_agc_profile_host.py builds and runs it, tests/test_gpu_agc_profile.py uses its `run` as the
// model of what the chain's kernels compute where the oracle has no counterpart (cap, manual gain, a change in mid-stream).
// Four slots, 0 and 1 with a client.  The script, one operation per line:
//   coeff MS RATE               pc_agc_coeff: the bits of the f32
//   plan RATE N                 pc_resolve for the rate and the audio FFT size: desired, attack, release as bits, and L
//   preset KIND                 agc_preset: ok and the six fields, then what agc_profile_check_values says of them at 12000
//   set I RATE null | DESIRED ATTACK RELEASE MAX_GAIN MANUAL MANUAL_GAIN
//                               psdr_client_set_agc_profile: agc_profile_check, then agc_profile_apply when it passes; prints the
//                               verdict and the slot's entry behind the call, as bits
//   batch SEQ                   agc_profile_plan for a batch in which slots 0 and 1 were demodulated: `any` and the table's `on`
//   run IN OUT                  the recurrence, sample by sample, over one client's stream.  IN (binary, native endianness): int32
//                               rate, L, nseg; f32 gain; int32 n0 (samples pushed since the last reset, at most L: the window starts
//                               with that many ZEROS - the model is only started from an empty or a full window of them); then
//                               nseg segments of 8 doubles: count, reset, on, desired, attack_ms, release_ms, max_gain, manual,
//                               and a ninth, manual_gain; then f32 x[sum of counts].  A segment with reset = 1 starts with
//                               AGC::reset; on = 0: the context's AGC (0.2, 50, 300).  OUT: f32 y[..] (the AGC's output),
//                               f32 g[..] (the gain behind each sample)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "agcplan.h"

using namespace psdr;

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static const char *verdict_name(AgcVerdict v) {
    switch (v) {
    case AP_OK: return "OK";
    case AP_BAD_ID: return "BAD_ID";
    case AP_NONFINITE: return "NONFINITE";
    case AP_BAD_DESIRED: return "BAD_DESIRED";
    case AP_BAD_TIME: return "BAD_TIME";
    case AP_BAD_CAP: return "BAD_CAP";
    case AP_BAD_MANUAL: return "BAD_MANUAL";
    case AP_BAD_MANUAL_GAIN: return "BAD_MANUAL_GAIN";
    case AP_NO_RATE: return "NO_RATE";
    case AP_ATTACK_SLOWER: return "ATTACK_SLOWER";
    }
    return "?";
}
static void print_entry(const AgcEntry &e) {
    printf("entry=%u:%u:%u:%u:%u:%d:%d", bits_of(e.desired), bits_of(e.att), bits_of(e.rel), bits_of(e.cap), bits_of(e.manual_gain), e.on, e.manual);
}

// The recurrence as postchain.h states it, sample by sample: the window is the last L samples, the output the oldest of them
// times the gain, zeros until the window is full.  peak by the plain maximum over the window.
struct Model {
    int L = 0;
    std::vector<float> win;  // the last min(n0, L) samples, oldest first
    float gain = 0.f;
    void reset() {
        gain = 0.f;
        win.clear();
    }
    float step(const AgcEntry &e, float x, float *g_out) {
        win.push_back(x);
        if ((int)win.size() > L) win.erase(win.begin());
        float y = 0.f;
        if ((int)win.size() == L) {
            float peak = 0.f;
            for (float v : win) peak = fmaxf(peak, fabsf(v));
            const float w = agc_want(e, peak);
            gain = fmaf(w < gain ? e.att : e.rel, w - gain, gain);
            y = win.front() * gain;
        }
        *g_out = gain;
        return y;
    }
};

static int run(const char *in, const char *out) {
    FILE *f = fopen(in, "rb");
    if (!f) return 1;
    int32_t head[3], n0 = 0;
    float g0 = 0.f;
    if (fread(head, 4, 3, f) != 3 || fread(&g0, 4, 1, f) != 1 || fread(&n0, 4, 1, f) != 1) return 1;
    const int rate = head[0], L = head[1], nseg = head[2];
    std::vector<double> seg((size_t)nseg * 9);
    if (fread(seg.data(), 8, seg.size(), f) != seg.size()) return 1;
    size_t total = 0;
    for (int s = 0; s < nseg; s++) total += (size_t)seg[9 * s];
    std::vector<float> x(total), y(total), g(total);
    if (total && fread(x.data(), 4, total, f) != total) return 1;
    fclose(f);
    Model m;
    m.L = L;
    m.gain = g0;
    m.win.assign((size_t)std::min(n0, (int32_t)L), 0.f);
    size_t t = 0;
    for (int s = 0; s < nseg; s++) {
        const double *q = &seg[9 * s];
        psdr_agc_profile p{};
        p.desired = q[3], p.attack_ms = q[4], p.release_ms = q[5], p.max_gain = q[6], p.manual = (int32_t)q[7], p.manual_gain = q[8];
        AgcEntry e;
        if (q[2] != 0) {
            if (agc_profile_check_values(p, rate) != AP_OK) return 2;
            e = agc_entry(p, rate);
        } else {
            e = agc_entry_none();
            e.desired = 0.2f, e.att = pc_agc_coeff(50.0f, (float)rate), e.rel = pc_agc_coeff(300.0f, (float)rate);
        }
        if (q[1] != 0) m.reset();
        for (size_t k = 0; k < (size_t)q[0]; k++, t++) y[t] = m.step(e, x[t], &g[t]);
    }
    FILE *o = fopen(out, "wb");
    if (!o) return 1;
    fwrite(y.data(), 4, total, o);
    fwrite(g.data(), 4, total, o);
    fclose(o);
    printf("run samples=%zu\n", total);
    return 0;
}

int main() {
    AudioSlot slots[4];
    slots[0].active = slots[1].active = true;
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        char op[32] = "", a1[400] = "", a2[400] = "";
        double v[8] = {};
        int i = 0, rate = 0;
        if (sscanf(line, "%31s", op) != 1) continue;
        if (!strcmp(op, "coeff") && sscanf(line, "%*s %lf %lf", &v[0], &v[1]) == 2) {
            printf("coeff bits=%u\n", bits_of(pc_agc_coeff((float)v[0], (float)v[1])));
        } else if (!strcmp(op, "plan") && sscanf(line, "%*s %d %d", &rate, &i) == 2) {
            PcFacts f;
            f.audio_rate = rate, f.n = i, f.slots = 4, f.max_batch = 1;
            const PcPlan p = pc_resolve(f, PcKnobs());
            printf("plan verdict=%d desired=%u attack=%u release=%u L=%d att_faster=%d\n", (int)p.verdict, bits_of(p.desired), bits_of(p.attack), bits_of(p.release), p.L,
                   (int)p.att_faster);
        } else if (!strcmp(op, "preset") && sscanf(line, "%*s %d", &i) == 1) {
            psdr_agc_profile p{};
            p.desired = -1;
            const bool ok = agc_preset(i, &p);
            printf("preset ok=%d desired=%.17g attack_ms=%.17g release_ms=%.17g max_gain=%.17g manual=%d manual_gain=%.17g check=%s\n", (int)ok, p.desired, p.attack_ms,
                   p.release_ms, p.max_gain, (int)p.manual, p.manual_gain, ok ? verdict_name(agc_profile_check_values(p, 12000)) : "-");
        } else if (!strcmp(op, "set") && sscanf(line, "%*s %d %d %399s", &i, &rate, a1) == 3) {
            psdr_agc_profile p{};
            const bool null = !strcmp(a1, "null");
            if (!null) {
                char w[6][64];
                if (sscanf(line, "%*s %*d %*d %63s %63s %63s %63s %63s %63s", w[0], w[1], w[2], w[3], w[4], w[5]) != 6) return 3;
                p.desired = strtod(w[0], nullptr), p.attack_ms = strtod(w[1], nullptr), p.release_ms = strtod(w[2], nullptr), p.max_gain = strtod(w[3], nullptr);
                p.manual = (int32_t)strtol(w[4], nullptr, 10), p.manual_gain = strtod(w[5], nullptr);
            }
            const AgcVerdict verdict = agc_profile_check(slots, 4, i, null ? nullptr : &p, rate);
            if (verdict == AP_OK) agc_profile_apply(slots[i], null ? nullptr : &p, rate);
            printf("set verdict=%s ", verdict_name(verdict));
            print_entry(slots[i >= 0 && i < 4 ? i : 0].agc);
            printf("\n");
        } else if (!strcmp(op, "batch") && sscanf(line, "%*s %d", &i) == 1) {
            slots[0].last_seq = slots[1].last_seq = (uint64_t)i;
            AgcEntry tab[4];
            const AgcPlan p = agc_profile_plan(slots, 4, (uint64_t)i, tab);
            printf("batch any=%d on=%d%d%d%d\n", (int)p.any, tab[0].on, tab[1].on, tab[2].on, tab[3].on);
        } else if (!strcmp(op, "run") && sscanf(line, "%*s %399s %399s", a1, a2) == 2) {
            const int rc = run(a1, a2);
            if (rc) {
                fprintf(stderr, "run failed: %d\n", rc);
                return rc;
            }
        } else {
            fprintf(stderr, "bad line: %s", line);
            return 4;
        }
    }
    return 0;
}

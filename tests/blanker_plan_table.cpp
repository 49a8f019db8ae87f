// Runs the impulse blanker's host side (phantomsdr_amd/csrc/blankerplan.h) over a script from stdin.  Plain host C++:
// tests/test_blanker_host.py builds and runs it.  The power, maximum and exceed functions are the text the kernels of
// blanker.h run.  The script, one operation per line:
//   check ON DB GUARD           nb_check: prints the verdict (DB through strtod: "nan" and "inf" are values)
//   db V                        nb_factor(V) as the bits of the f32
//   on                          psdr_ring_set_blanker(on = 1) on a blanker that is off: the reference starts afresh
//   reset                       a new context: the state as constructed
//   plan FIRST NFRAMES NHALVES RCAP
//                               nb_plan on the carried state, which moves on: one `plan` line
//   chunk FMT REAL W0 W1 W2 W3  a 16-byte chunk as four words: nb_chunk_powers, nb_chunk_max and, sample by sample from the
//                               chunk's bytes, nb_sample_power - all as f32 bits
//   cmp P T M                   (f32 bits) nb_exceed(P, T), nb_threshold_valid(T), nb_max(M, P)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "blankerplan.h"

using namespace psdr;

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static float float_of(uint32_t u) {
    float v;
    memcpy(&v, &u, 4);
    return v;
}

int main() {
    NbState st;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        if (op == "check") {
            int on = 0, guard = 0;
            std::string db;
            if (!(in >> on >> db >> guard)) return 2;
            const NbVerdict v = nb_check(on, strtod(db.c_str(), nullptr), guard);
            printf("check verdict=%s\n", v == NB_OK ? "OK" : (v == NB_BAD_DB ? "BAD_DB" : "BAD_GUARD"));
        } else if (op == "db") {
            double v = 0;
            if (!(in >> v)) return 2;
            printf("db v=%.17g bits=%u\n", v, bits_of(nb_factor(v)));
        } else if (op == "on") {
            st.fresh = true;
        } else if (op == "reset") {
            st = NbState();
        } else if (op == "plan") {
            unsigned long long first = 0;
            int nframes = 0, nhalves = 0, rcap = 0;
            if (!(in >> first >> nframes >> nhalves >> rcap) || nframes < 1 || nhalves < 2 || rcap < nframes + 2) return 2;
            const NbPlan p = nb_plan(st, first, nframes, nhalves, rcap);
            st = p.after;
            printf("plan nnew=%d first_new=%llu slot0=%d mirror=%d own=%d r0=%d next=%llu rpos=%d prev=", p.nnew, (unsigned long long)p.first_new, p.slot0, p.mirror,
                   (int)p.own, p.r0, (unsigned long long)st.next, st.rpos);
            for (int j = 0; j < p.nnew; j++) printf("%s%d", j ? "," : "", nb_prev_pos(p, j, rcap));
            printf("\n");
        } else if (op == "chunk") {
            int fmt = 0, real = 0;
            uint32_t w[4];
            if (!(in >> fmt >> real >> w[0] >> w[1] >> w[2] >> w[3]) || fmt < 0 || fmt > 5) return 2;
            float P[16];
            const int n = nb_chunk_powers(w, fmt, real != 0, P);
            unsigned char bytes[16];
            memcpy(bytes, w, 16);
            printf("chunk n=%d max=%u p=", n, bits_of(nb_chunk_max(w, fmt, real != 0)));
            for (int i = 0; i < n; i++) printf("%s%u", i ? "," : "", bits_of(P[i]));
            printf(" s=");
            const int sb = nb_sample_bytes(fmt, real != 0);
            for (int i = 0; i < n; i++) printf("%s%u", i ? "," : "", bits_of(nb_sample_power(bytes + i * sb, fmt, real != 0)));
            printf(" zero=%u sb=%d\n", nb_zero_word(fmt), sb);
        } else if (op == "cmp") {
            uint32_t p = 0, t = 0, m = 0;
            if (!(in >> p >> t >> m)) return 2;
            printf("cmp exceed=%d valid=%d max=%u\n", (int)nb_exceed(float_of(p), float_of(t)), (int)nb_threshold_valid(float_of(t)), bits_of(nb_max(float_of(m), float_of(p))));
        } else {
            return 2;
        }
    }
    return 0;
}

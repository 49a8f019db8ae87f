// Runs the audio filter's host side (phantomsdr_amd/csrc/audiofilterplan.h) over a script from stdin.  Plain host C++:
// tests/test_audio_filter_host.py builds and runs it.  The slots, their setters and the printed demodulation plan are those of
// tests/demod_plan_table.cpp, whose text is included (its main() under another name); behind every `batch` this program runs
// audio_filter_plan() as demod.hip does and prints what it yields.  The script, one operation per line:
//   case NAME | size S n nframes | add I | remove I | pause I | resume I | kind I MODE FINE SIDEBAND | window I L MID R | post on|off
//                               as in demod_plan_table.cpp
//   filter I N B0 B1 B2 A1 A2 ..  psdr_client_set_audio_filter with N sections of five coefficients (or the word `null` behind N:
//                               a null pointer): audio_filter_check, then audio_filter_apply; prints the verdict (I may be any integer)
//   dump                        the filter fields of every slot
//   batch                       demod_plan (printed as demod_plan_table.cpp prints it), then audio_filter_plan: one `af` line
//   design KIND RATE F0 Q       psdr_audio_filter_design: the verdict and the five doubles
//   table B0 B1 B2 A1 A2        af_section: the f32 coefficients and the 6 x 4 powers, as the bits of the f32
//   run IN OUT                  the blocked evaluation of one client's stream, batch by batch from zero state.  IN (binary, native
//                               endianness): int32 nsec, h, nb; int32 frames[nb]; double sections[nsec][5]; int32 flags[F]; f32
//                               rows[F * h] as bits (F = the sum of frames).  OUT: f32 rows[F * h], then f32 state[nb][4] behind each batch
#define main demod_plan_table_main
#include "demod_plan_table.cpp"
#undef main

#include "audiofilterplan.h"

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static const char *verdict_name(AfVerdict v) {
    switch (v) {
    case AF_OK: return "OK";
    case AF_BAD_ID: return "BAD_ID";
    case AF_BAD_COUNT: return "BAD_COUNT";
    case AF_NULL: return "NULL";
    case AF_NONFINITE: return "NONFINITE";
    case AF_UNSTABLE: return "UNSTABLE";
    case AF_POLE: return "POLE";
    }
    return "?";
}
static const char *design_name(AfDesignVerdict v) {
    switch (v) {
    case AD_OK: return "OK";
    case AD_NULL: return "NULL";
    case AD_BAD_KIND: return "BAD_KIND";
    case AD_BAD_RATE: return "BAD_RATE";
    case AD_BAD_F0: return "BAD_F0";
    case AD_BAD_Q: return "BAD_Q";
    case AD_REFUSED: return "REFUSED";
    }
    return "?";
}
static void print_section(const AfSection &s) {
    printf("%u:%u:%u:%u:%u", bits_of(s.b0), bits_of(s.b1), bits_of(s.b2), bits_of(s.a1), bits_of(s.a2));
    for (int k = 0; k < AF_LEVELS; k++)
        for (int i = 0; i < 4; i++) printf(":%u", bits_of(s.P[k][i]));
}
static void dump(const Ctx &c) {
    for (size_t i = 0; i < c.S; i++) {
        const AudioSlot &s = c.slots[i];
        printf("afs slot=%zu active=%d n=%d fresh=%d sec0=", i, (int)s.active, s.af_n, (int)s.af_fresh);
        print_section(s.af_sec[0]);
        printf(" sec1=");
        print_section(s.af_sec[1]);
        printf("\n");
    }
}
// behind demod_plan, as demod_impl calls it (the context's first filter client allocates the table: `have`)
static void filter_batch(Ctx &c, uint64_t seq_before, bool have) {
    if (c.seq == seq_before) {  // (a refused batch: nothing moved)
        printf("af refused=1\n");
        return;
    }
    std::vector<AfEntry> table(c.S);
    AfPlan p;
    if (have) p = audio_filter_plan(c.slots.data(), c.S, c.seq, table.data());
    printf("af have=%d n=%d any=%d zero=", (int)have, p.n, (int)p.any());
    for (size_t j = 0; j < p.zero.size(); j++) printf("%s%zu", j ? "," : "", p.zero[j]);
    printf(" list=");
    for (int j = 0; j < p.n; j++) printf("%s%d:%d:%u:%u", j ? "," : "", table[j].slot, table[j].nsec, bits_of(table[j].sec[0].b0), bits_of(table[j].sec[1].b0));
    printf("\n");
}
template <class T>
static void rd(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) exit(3);
}
static int run_file(const std::string &in, const std::string &out) {
    FILE *f = fopen(in.c_str(), "rb");
    if (!f) return 3;
    int32_t head[3];
    rd(f, head, 3);
    const int nsec = head[0], h = head[1], nb = head[2];
    if (nsec < 1 || nsec > PSDR_AUDIO_FILTER_SECTIONS || h < 1 || nb < 1) return 3;
    std::vector<int32_t> frames(nb);
    rd(f, frames.data(), nb);
    size_t F = 0;
    for (int32_t v : frames) {
        if (v < 1) return 3;
        F += (size_t)v;
    }
    psdr_biquad sec[PSDR_AUDIO_FILTER_SECTIONS] = {};
    for (int s = 0; s < nsec; s++) rd(f, &sec[s].b0, 5);
    std::vector<int32_t> flags(F);
    std::vector<float> rows(F * h), states;
    rd(f, flags.data(), F);
    rd(f, rows.data(), F * h);
    fclose(f);
    if (audio_filter_check_sections(nsec, sec) != AF_OK) return 4;
    AfEntry e{};
    e.nsec = nsec;
    for (int s = 0; s < nsec; s++) e.sec[s] = af_section(sec[s]);
    float state[2 * PSDR_AUDIO_FILTER_SECTIONS] = {0, 0, 0, 0};
    size_t at = 0;
    for (int b = 0; b < nb; b++) {
        af_stream(e, rows.data() + at * h, flags.data() + at, h, frames[b], state);
        at += (size_t)frames[b];
        states.insert(states.end(), state, state + 4);
    }
    FILE *g = fopen(out.c_str(), "wb");
    if (!g) return 3;
    if (fwrite(rows.data(), 4, rows.size(), g) != rows.size() || fwrite(states.data(), 4, states.size(), g) != states.size()) return 3;
    fclose(g);
    printf("run frames=%zu h=%d nb=%d nsec=%d\n", F, h, nb, nsec);
    return 0;
}

int main() {
    Ctx c;
    bool have = false;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, w;
        if (!(in >> op)) continue;
        if (op == "case") {
            in >> w;
            c.resize(8, 360, 5);
            have = false;
            printf("case name=%s\n", w.c_str());
        } else if (op == "size") {
            size_t S = 0;
            int n = 0, nframes = 0;
            if (!(in >> S >> n >> nframes) || S == 0) return 2;
            c.resize(S, n, nframes);
            have = false;
        } else if (op == "batch") {
            const uint64_t before = c.seq;
            batch(c);
            filter_batch(c, before, have);
        } else if (op == "post") {
            in >> w;
            c.f.post_on = w == "on";
        } else if (op == "dump") {
            dump(c);
        } else if (op == "design") {
            int kind = 0;
            std::string a[3];  // (strtod: "nan" and "inf" are values here)
            if (!(in >> kind >> a[0] >> a[1] >> a[2])) return 2;
            psdr_biquad b{};
            const AfDesignVerdict v = audio_filter_design(kind, strtod(a[0].c_str(), nullptr), strtod(a[1].c_str(), nullptr), strtod(a[2].c_str(), nullptr), &b);
            printf("design verdict=%s b0=%.17g b1=%.17g b2=%.17g a1=%.17g a2=%.17g\n", design_name(v), b.b0, b.b1, b.b2, b.a1, b.a2);
        } else if (op == "table") {
            psdr_biquad b{};
            if (!(in >> b.b0 >> b.b1 >> b.b2 >> b.a1 >> b.a2)) return 2;
            printf("table sec=");
            print_section(af_section(b));
            printf("\n");
        } else if (op == "run") {
            std::string fin, fout;
            if (!(in >> fin >> fout)) return 2;
            const int rc = run_file(fin, fout);
            if (rc) return rc;
        } else if (op == "filter") {
            int id = 0, n = 0;
            if (!(in >> id >> n)) return 2;
            std::vector<psdr_biquad> sec;
            bool null = false;
            while (in >> w) {
                if (w == "null") {
                    null = true;
                    break;
                }
                double v[5] = {strtod(w.c_str(), nullptr), 0, 0, 0, 0};
                for (int k = 1; k < 5; k++) {
                    if (!(in >> w)) return 2;
                    v[k] = strtod(w.c_str(), nullptr);
                }
                sec.push_back(psdr_biquad{v[0], v[1], v[2], v[3], v[4]});
            }
            if (!null && n > 0 && n <= PSDR_AUDIO_FILTER_SECTIONS && (int)sec.size() < n) return 2;
            const psdr_biquad *ptr = null || sec.empty() ? nullptr : sec.data();
            const AfVerdict v = audio_filter_check(c.slots.data(), c.S, id, n, ptr);
            if (v == AF_OK) {
                if (n > 0) have = true;  // (first_use of the filter's state and table)
                audio_filter_apply(c.slots[id], n, ptr);
            }
            printf("set id=%d verdict=%s\n", id, verdict_name(v));
        } else {
            size_t i = 0;
            if (!(in >> i) || i >= c.S) return 2;
            AudioSlot &s = c.slots[i];
            if (op == "add") {
                op_add(c, i);
            } else if (op == "remove") {
                s.active = false;
            } else if (op == "pause" || op == "resume") {
                s.paused = op == "pause";
            } else if (op == "kind") {
                int mode = 0, fine = 0, sb = 0;
                if (!(in >> mode >> fine >> sb)) return 2;
                op_kind(c, i, mode, fine, sb);
            } else if (op == "window") {
                if (!(in >> s.l >> s.mid >> s.r)) return 2;
            } else {
                return 2;
            }
        }
    }
    return 0;
}

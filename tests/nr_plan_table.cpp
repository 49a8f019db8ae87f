// Runs the noise reduction's host side (phantomsdr_amd/csrc/nrplan.h) over a script from stdin.  Plain host C++:
// tests/test_nr_host.py builds and runs it.  The slots, their setters and the printed demodulation plan are those of
// tests/demod_plan_table.cpp, whose text is included (its main() under another name); behind every `batch` this program runs
// nr_plan() as demod.hip does and prints what it yields.  The script, one operation per line:
//   case NAME | size S n nframes | add I | remove I | pause I | resume I | kind I MODE FINE SIDEBAND | window I L MID R | post on|off
//                               as in demod_plan_table.cpp
//   rate R                      the context's audio_rate (12000 at every `case`)
//   nr I ON DEPTH BETA          psdr_client_set_noise_reduction: nr_check, then nr_apply; prints the verdict (I may be any integer)
//   dump                        the noise reduction fields of every slot
//   batch                       demod_plan (printed as demod_plan_table.cpp prints it), then nr_plan: one `nrp` line
//   preset K                    psdr_noise_reduction_preset
//   tables OUT                  NrTables as the device gets it (binary)
//   run IN OUT                  nr_stream over one client's stream, batch by batch from zero state.  IN (binary, native endianness):
//                               int32 h, nb, rate; double depth_db, beta; int32 frames[nb]; int32 flags[F]; f32 rows[F * h] as bits
//                               (F = the sum of frames).  OUT: f32 rows[F * h]; NrState[nb] behind each batch; then the applied
//                               gains of every finished block, 129 f32 each
#define main demod_plan_table_main
#include "demod_plan_table.cpp"
#undef main

#include "nrplan.h"

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static const char *verdict_name(NrVerdict v) {
    switch (v) {
    case NR_OK: return "OK";
    case NR_BAD_ID: return "BAD_ID";
    case NR_INACTIVE: return "INACTIVE";
    case NR_IQ: return "IQ";
    case NR_NONFINITE: return "NONFINITE";
    case NR_BAD_DEPTH: return "BAD_DEPTH";
    case NR_BAD_BETA: return "BAD_BETA";
    case NR_NO_RATE: return "NO_RATE";
    }
    return "?";
}
static void dump(const Ctx &c) {
    for (size_t i = 0; i < c.S; i++) {
        const AudioSlot &s = c.slots[i];
        printf("nrs slot=%zu active=%d on=%d fresh=%d g_min=%u beta=%u\n", i, (int)s.active, s.nr_on, (int)s.nr_fresh, bits_of(s.nr_g_min), bits_of(s.nr_beta));
    }
}
// behind demod_plan, as demod_impl calls it (the context's first such client allocates state and tables: `have`)
static void nr_batch(Ctx &c, uint64_t seq_before, bool have, int rate) {
    if (c.seq == seq_before) {  // (a refused batch: nothing moved)
        printf("nrp refused=1\n");
        return;
    }
    std::vector<NrEntry> table(c.S);
    NrPlan p;
    if (have) p = nr_plan(c.slots.data(), c.S, c.seq, table.data(), nr_a_up(rate));
    printf("nrp have=%d n=%d any=%d zero=", (int)have, p.n, (int)p.any());
    for (size_t j = 0; j < p.zero.size(); j++) printf("%s%zu", j ? "," : "", p.zero[j]);
    printf(" list=");
    for (int j = 0; j < p.n; j++) printf("%s%d:%u:%u:%u", j ? "," : "", table[j].slot, bits_of(table[j].g_min), bits_of(table[j].beta), bits_of(table[j].a_up));
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
    double par[2];
    rd(f, head, 3);
    rd(f, par, 2);
    const int h = head[0], nb = head[1], rate = head[2];
    if (h < 1 || nb < 1 || rate < 1) return 3;
    std::vector<int32_t> frames(nb);
    rd(f, frames.data(), nb);
    size_t F = 0;
    for (int32_t v : frames) {
        if (v < 1) return 3;
        F += (size_t)v;
    }
    std::vector<int32_t> flags(F);
    std::vector<float> rows(F * h), gains;
    rd(f, flags.data(), F);
    rd(f, rows.data(), F * h);
    fclose(f);
    AudioSlot slot;
    slot.active = true;
    if (nr_check(&slot, 1, 0, 1, par[0], par[1], rate) != NR_OK) return 4;
    nr_apply(slot, 1, par[0], par[1]);
    const NrEntry e{0, slot.nr_g_min, slot.nr_beta, nr_a_up(rate)};
    static NrTables t;
    nr_tables(t);
    std::vector<NrState> states;
    NrState st{};
    size_t at = 0;
    for (int b = 0; b < nb; b++) {
        nr_stream(t, e, rows.data() + at * h, flags.data() + at, h, frames[b], st, &gains);
        at += (size_t)frames[b];
        states.push_back(st);
    }
    FILE *g = fopen(out.c_str(), "wb");
    if (!g) return 3;
    if (fwrite(rows.data(), 4, rows.size(), g) != rows.size() || fwrite(states.data(), sizeof(NrState), states.size(), g) != states.size() ||
        (!gains.empty() && fwrite(gains.data(), 4, gains.size(), g) != gains.size()))
        return 3;
    fclose(g);
    printf("run frames=%zu h=%d nb=%d blocks=%zu g_min=%u a_up=%u\n", F, h, nb, gains.size() / NR_BINS, bits_of(e.g_min), bits_of(e.a_up));
    return 0;
}

int main() {
    Ctx c;
    bool have = false;
    int rate = 12000;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, w;
        if (!(in >> op)) continue;
        if (op == "case") {
            in >> w;
            c.resize(8, 360, 5);
            have = false, rate = 12000;
            printf("case name=%s\n", w.c_str());
        } else if (op == "size") {
            size_t S = 0;
            int n = 0, nframes = 0;
            if (!(in >> S >> n >> nframes) || S == 0) return 2;
            c.resize(S, n, nframes);
            have = false;
        } else if (op == "rate") {
            if (!(in >> rate)) return 2;
        } else if (op == "batch") {
            const uint64_t before = c.seq;
            batch(c);
            nr_batch(c, before, have, rate);
        } else if (op == "post") {
            in >> w;
            c.f.post_on = w == "on";
        } else if (op == "dump") {
            dump(c);
        } else if (op == "preset") {
            int k = 0;
            if (!(in >> k)) return 2;
            double d = -1, b = -1;
            const bool ok = nr_preset(k, &d, &b);
            printf("preset kind=%d ok=%d depth=%.17g beta=%.17g\n", k, (int)ok, d, b);
        } else if (op == "tables") {
            if (!(in >> w)) return 2;
            static NrTables t;
            nr_tables(t);
            FILE *g = fopen(w.c_str(), "wb");
            if (!g || fwrite(&t, sizeof(t), 1, g) != 1) return 3;
            fclose(g);
            printf("tables bytes=%zu\n", sizeof(t));
        } else if (op == "run") {
            std::string fin, fout;
            if (!(in >> fin >> fout)) return 2;
            const int rc = run_file(fin, fout);
            if (rc) return rc;
        } else if (op == "nr") {
            int id = 0, on = 0;
            std::string a[2];  // (strtod: "nan" and "inf" are values here)
            if (!(in >> id >> on >> a[0] >> a[1])) return 2;
            const double depth = strtod(a[0].c_str(), nullptr), beta = strtod(a[1].c_str(), nullptr);
            const NrVerdict v = nr_check(c.slots.data(), c.S, id, on, depth, beta, rate);
            if (v == NR_OK) {
                if (on) have = true;  // (first_use of the state and the tables)
                nr_apply(c.slots[id], on, depth, beta);
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

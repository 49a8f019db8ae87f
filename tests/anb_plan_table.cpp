// Runs the audio blanker's host side (phantomsdr_amd/csrc/anbplan.h) over a script from stdin.  Plain host C++:
// tests/test_anb_host.py builds and runs it.  The slots, their setters and the printed demodulation plan are those of
// tests/demod_plan_table.cpp, whose text is included (its main() under another name); behind every `batch` this program runs
// anb_plan() as demod.hip does and prints what it yields.  The script, one operation per line:
//   case NAME | size S n nframes | add I | remove I | pause I | resume I | kind I MODE FINE SIDEBAND | window I L MID R | post on|off
//                               as in demod_plan_table.cpp
//   anb I ON THRESHOLD WIDTH    psdr_client_set_audio_blanker: anb_check, then anb_apply; prints the verdict (I may be any integer)
//   dump                        the blanker fields of every slot
//   batch                       demod_plan (printed as demod_plan_table.cpp prints it), then anb_plan: one `anbp` line
//   preset K                    psdr_audio_blanker_preset
//   levinson R0 .. R10          anb_levinson on these eleven values: the order that stands and a[0..10]
//   run IN OUT                  anb_stream over one client's stream, batch by batch from zero state.  IN (binary, native endianness):
//                               int32 h, nb, width; double threshold; int32 frames[nb]; int32 flags[F]; f32 rows[F * h] as bits
//                               (F = the sum of frames).  OUT: f32 rows[F * h]; AnbState[nb] behind each batch; int64 nblocks,
//                               ncentres; int32 order[nblocks]; f32 level[nblocks]; f32 m[nblocks * 256]; int64 centres[ncentres]
#define main demod_plan_table_main
#include "demod_plan_table.cpp"
#undef main

#include "anbplan.h"

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static const char *verdict_name(AnbVerdict v) {
    switch (v) {
    case ANB_OK: return "OK";
    case ANB_BAD_ID: return "BAD_ID";
    case ANB_INACTIVE: return "INACTIVE";
    case ANB_IQ: return "IQ";
    case ANB_NONFINITE: return "NONFINITE";
    case ANB_BAD_THRESHOLD: return "BAD_THRESHOLD";
    case ANB_BAD_WIDTH: return "BAD_WIDTH";
    }
    return "?";
}
static void dump(const Ctx &c) {
    for (size_t i = 0; i < c.S; i++) {
        const AudioSlot &s = c.slots[i];
        printf("anbs slot=%zu active=%d on=%d fresh=%d threshold=%u width=%d\n", i, (int)s.active, s.anb_on, (int)s.anb_fresh, bits_of(s.anb_threshold), s.anb_width);
    }
}
// behind demod_plan, as demod_impl calls it (the context's first such client allocates the state: `have`)
static void anb_batch(Ctx &c, uint64_t seq_before, bool have) {
    if (c.seq == seq_before) {  // (a refused batch: nothing moved)
        printf("anbp refused=1\n");
        return;
    }
    std::vector<AnbEntry> table(c.S);
    AnbPlan p;
    if (have) p = anb_plan(c.slots.data(), c.S, c.seq, table.data());
    printf("anbp have=%d n=%d any=%d zero=", (int)have, p.n, (int)p.any());
    for (size_t j = 0; j < p.zero.size(); j++) printf("%s%zu", j ? "," : "", p.zero[j]);
    printf(" list=");
    for (int j = 0; j < p.n; j++) printf("%s%d:%u:%d", j ? "," : "", table[j].slot, bits_of(table[j].threshold), table[j].width);
    printf("\n");
}
template <class T>
static void rd(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) exit(3);
}
template <class T>
static bool wr(FILE *f, const T *p, size_t n) {
    return !n || fwrite(p, sizeof(T), n, f) == n;
}
static int run_file(const std::string &in, const std::string &out) {
    FILE *f = fopen(in.c_str(), "rb");
    if (!f) return 3;
    int32_t head[3];
    double thr;
    rd(f, head, 3);
    rd(f, &thr, 1);
    const int h = head[0], nb = head[1], width = head[2];
    if (h < 1 || nb < 1) return 3;
    std::vector<int32_t> frames(nb);
    rd(f, frames.data(), nb);
    size_t F = 0;
    for (int32_t v : frames) {
        if (v < 1) return 3;
        F += (size_t)v;
    }
    std::vector<int32_t> flags(F);
    std::vector<float> rows(F * h);
    rd(f, flags.data(), F);
    rd(f, rows.data(), F * h);
    fclose(f);
    AudioSlot slot;
    slot.active = true;
    if (anb_check(&slot, 1, 0, 1, thr, width) != ANB_OK) return 4;
    anb_apply(slot, 1, thr, width);
    const AnbEntry e{0, slot.anb_threshold, slot.anb_width, 0};
    std::vector<AnbState> states;
    AnbState st{};
    AnbTrace tr;
    size_t at = 0;
    for (int b = 0; b < nb; b++) {
        anb_stream(e, rows.data() + at * h, flags.data() + at, h, frames[b], st, &tr);
        at += (size_t)frames[b];
        states.push_back(st);
    }
    FILE *g = fopen(out.c_str(), "wb");
    if (!g) return 3;
    const int64_t counts[2] = {(int64_t)tr.orders.size(), (int64_t)tr.centres.size()};
    if (!wr(g, rows.data(), rows.size()) || !wr(g, states.data(), states.size()) || !wr(g, counts, 2) || !wr(g, tr.orders.data(), tr.orders.size()) ||
        !wr(g, tr.levels.data(), tr.levels.size()) || !wr(g, tr.m.data(), tr.m.size()) || !wr(g, tr.centres.data(), tr.centres.size()))
        return 3;
    fclose(g);
    printf("run frames=%zu h=%d nb=%d blocks=%zu centres=%zu threshold=%u width=%d\n", F, h, nb, tr.orders.size(), tr.centres.size(), bits_of(e.threshold), e.width);
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
            anb_batch(c, before, have);
        } else if (op == "post") {
            in >> w;
            c.f.post_on = w == "on";
        } else if (op == "dump") {
            dump(c);
        } else if (op == "preset") {
            int k = 0;
            if (!(in >> k)) return 2;
            double t = -1;
            int wd = -1;
            const bool ok = anb_preset(k, &t, &wd);
            printf("preset kind=%d ok=%d threshold=%.17g width=%d\n", k, (int)ok, t, wd);
        } else if (op == "levinson") {
            float R[ANB_P + 1], a[ANB_P + 1];
            for (int i = 0; i <= ANB_P; i++) {
                if (!(in >> w)) return 2;
                R[i] = strtof(w.c_str(), nullptr);
            }
            const int order = anb_levinson(R, a);
            printf("levinson order=%d a=", order);
            for (int i = 0; i <= ANB_P; i++) printf("%s%.9g", i ? "," : "", a[i]);
            printf("\n");
        } else if (op == "run") {
            std::string fin, fout;
            if (!(in >> fin >> fout)) return 2;
            const int rc = run_file(fin, fout);
            if (rc) return rc;
        } else if (op == "anb") {
            int id = 0, on = 0, width = 0;
            std::string a;  // (strtod: "nan" and "inf" are values here)
            if (!(in >> id >> on >> a >> width)) return 2;
            const double thr = strtod(a.c_str(), nullptr);
            const AnbVerdict v = anb_check(c.slots.data(), c.S, id, on, thr, width);
            if (v == ANB_OK) {
                if (on) have = true;  // (first_use of the state)
                anb_apply(c.slots[id], on, thr, width);
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

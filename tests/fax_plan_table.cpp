// Runs the radiofax decoder's host side (phantomsdr_amd/csrc/faxplan.h) over a script from stdin.  Plain host C++:
// tests/test_fax_host.py builds and runs it.  The slots, their setters and the printed demodulation plan are those of
// tests/demod_plan_table.cpp, whose text is included (its main() under another name); behind every `batch` this program runs
// fax_plan() as demod.hip does and prints what it yields.  The script, one operation per line:
//   case NAME | size S n nframes | add I | remove I | pause I | resume I | kind I MODE FINE SIDEBAND | window I L MID R
//                               as in demod_plan_table.cpp
//   rate R                      the context's audio_rate (12000 at every `case`)
//   fax I ON MODE BLACK WHITE LPM WIDTH SLANT PHASE_COL RATIO START_BLOCKS PHASE_LINES MAX_LINES
//                               psdr_client_set_fax_decoder (ON = 0: a null config): fax_check, then fax_apply with a largest batch
//                               of 5 frames of 180 samples; prints the verdict (I may be any integer)
//   dump                        the fax decoder fields of every slot
//   batch                       demod_plan (printed as demod_plan_table.cpp prints it), then fax_plan: one `fxp` line
//   defaults RATE               psdr_fax_defaults
//   run IN OUT                  fax_stream over one client's stream, batch by batch from zero state.  IN (binary, native endianness):
//                               int32 h, nb, rate, maxb; int32 mode, width, phase_col, start_blocks, phase_lines, max_lines;
//                               double black, white, lpm, slant, ratio; int32 frames[nb]; int32 flags[F]; f32 rows[F * h] as bits
//                               (F = the sum of frames; maxb: the frames of the context's largest batch).  OUT: FaxRec[F];
//                               FaxState[nb] behind each batch; int32 R; uint32 meta[R]; uint8 ring[R * width]
//   angle IN OUT                fax_angle over pairs: IN f32 (re, im)[n] to the file's end, OUT f32 a[n]
#define main demod_plan_table_main
#include "demod_plan_table.cpp"
#undef main

#include "faxplan.h"

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static const char *verdict_name(FaxVerdict v) {
    static const char *names[] = {"OK",        "BAD_ID",        "INACTIVE",  "IQ",        "BAD_MODE",        "BAD_TONES",     "BAD_LPM",  "BAD_WIDTH", "BAD_SLANT",
                                  "BAD_PHASE_COL", "BAD_RATIO", "BAD_START", "BAD_PHASE_LINES", "BAD_MAX_LINES", "BAD_RATE", "BAD_BAND",  "BAD_PIXEL"};
    return names[(int)v];
}
static void dump(const Ctx &c) {
    for (size_t i = 0; i < c.S; i++) {
        const AudioSlot &s = c.slots[i];
        const FaxEntry &e = s.fax;
        printf("fxs slot=%zu active=%d on=%d fresh=%d b_on=%d mode=%d width=%d K=%d D=%d NB=%d wp=%d R=%d Lq=%llu origin0=%llu inc=%u tinc0=%u s=%u ratio=%u shift=%u nbh=%u\n", i,
               (int)s.active, s.fax_on, (int)s.fax_fresh, (int)s.b_fax_on, e.mode, e.width, e.K, e.D, e.NB, e.wp, e.R, (unsigned long long)e.Lq, (unsigned long long)e.origin0,
               e.inc, e.tinc[0], bits_of(e.s), bits_of(e.ratio), bits_of(e.shift), bits_of(e.nbh));
    }
}
// behind demod_plan, as demod_impl calls it (the context's first such client allocates state and tables: `have`)
static void fax_batch(Ctx &c, uint64_t seq_before, bool have) {
    if (c.seq == seq_before) {  // (a refused batch: nothing moved)
        printf("fxp refused=1\n");
        return;
    }
    std::vector<FaxEntry> table(c.S);
    FaxPlan p;
    if (have) p = fax_plan(c.slots.data(), c.S, c.seq, table.data());
    printf("fxp have=%d n=%d any=%d zero=", (int)have, p.n, (int)p.any());
    for (size_t j = 0; j < p.zero.size(); j++) printf("%s%zu", j ? "," : "", p.zero[j]);
    printf(" list=");
    for (int j = 0; j < p.n; j++) printf("%s%d:%d:%d:%llu:%u", j ? "," : "", table[j].slot, table[j].mode, table[j].width, (unsigned long long)table[j].Lq, table[j].inc);
    printf("\n");
}
template <class T>
static void rd(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) exit(3);
}
static int run_file(const std::string &in, const std::string &out) {
    FILE *f = fopen(in.c_str(), "rb");
    if (!f) return 3;
    int32_t head[10];
    double par[5];
    rd(f, head, 10);
    rd(f, par, 5);
    const int h = head[0], nb = head[1], rate = head[2], maxb = head[3];
    if (h < 1 || nb < 1 || maxb < 1) return 3;
    std::vector<int32_t> frames(nb);
    rd(f, frames.data(), nb);
    size_t F = 0;
    for (int32_t v : frames) {
        if (v < 1 || v > maxb) return 3;
        F += (size_t)v;
    }
    std::vector<int32_t> flags(F);
    std::vector<float> rows(F * h);
    rd(f, flags.data(), F);
    rd(f, rows.data(), F * h);
    fclose(f);
    AudioSlot slot;
    slot.active = true;
    psdr_fax_config cfg;
    cfg.mode = head[4], cfg.width = head[5], cfg.phase_col = head[6], cfg.start_blocks = head[7], cfg.phase_lines = head[8], cfg.max_lines = head[9];
    cfg.black_hz = par[0], cfg.white_hz = par[1], cfg.lpm = par[2], cfg.slant_ppm = par[3], cfg.tone_ratio = par[4];
    const FaxVerdict v = fax_check(&slot, 1, 0, &cfg, rate);
    if (v != FAX_OK) {
        fprintf(stderr, "run: %s\n", verdict_name(v));
        return 4;
    }
    fax_apply(slot, &cfg, rate, (uint64_t)maxb * (uint64_t)h);
    const FaxEntry e = slot.fax;
    std::vector<FaxTables> t(1);
    fax_tables(t[0], (double)rate);
    std::vector<FaxRec> rec(F);
    std::vector<FaxState> states;
    std::vector<uint8_t> ring((size_t)e.R * e.width, 0);
    std::vector<uint32_t> meta(e.R, 0);
    FaxState st;
    memset(&st, 0, sizeof(st));
    size_t at = 0;
    for (int b = 0; b < nb; b++) {
        fax_stream(t[0], e, rows.data() + at * h, flags.data() + at, h, frames[b], st, ring.data(), meta.data(), rec.data() + at);
        at += (size_t)frames[b];
        states.push_back(st);
    }
    FILE *g = fopen(out.c_str(), "wb");
    if (!g) return 3;
    const int32_t R = e.R;
    if (fwrite(rec.data(), sizeof(FaxRec), F, g) != F || fwrite(states.data(), sizeof(FaxState), states.size(), g) != states.size() || fwrite(&R, 4, 1, g) != 1 ||
        fwrite(meta.data(), 4, meta.size(), g) != meta.size() || fwrite(ring.data(), 1, ring.size(), g) != ring.size())
        return 3;
    fclose(g);
    printf("run frames=%zu h=%d nb=%d H=%d K=%d D=%d NB=%d R=%d Lq=%llu\n", F, h, nb, t[0].H, e.K, e.D, e.NB, e.R, (unsigned long long)e.Lq);
    return 0;
}
static int angle_file(const std::string &in, const std::string &out) {
    FILE *f = fopen(in.c_str(), "rb");
    FILE *g = fopen(out.c_str(), "wb");
    if (!f || !g) return 3;
    float p[2];
    while (fread(p, 4, 2, f) == 2) {
        const float a = fax_angle(p[0], p[1]);
        if (fwrite(&a, 4, 1, g) != 1) return 3;
    }
    fclose(f);
    fclose(g);
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
            fax_batch(c, before, have);
        } else if (op == "dump") {
            dump(c);
        } else if (op == "defaults") {
            if (!(in >> w)) return 2;
            const double r = strtod(w.c_str(), nullptr);
            psdr_fax_config d;
            memset(&d, 0, sizeof(d));
            const bool ok = fax_defaults(r, &d);
            printf("defaults rate=%.17g ok=%d mode=%d black_hz=%.17g white_hz=%.17g lpm=%.17g width=%d slant_ppm=%.17g phase_col=%d tone_ratio=%.17g start_blocks=%d phase_lines=%d "
                   "max_lines=%d\n",
                   r, (int)ok, d.mode, d.black_hz, d.white_hz, d.lpm, d.width, d.slant_ppm, d.phase_col, d.tone_ratio, d.start_blocks, d.phase_lines, d.max_lines);
        } else if (op == "run" || op == "angle") {
            std::string fin, fout;
            if (!(in >> fin >> fout)) return 2;
            const int rc = op == "run" ? run_file(fin, fout) : angle_file(fin, fout);
            if (rc) return rc;
        } else if (op == "fax") {
            int id = 0, on = 0;
            psdr_fax_config cfg;
            std::string a[5];  // (strtod: "nan" and "inf" are values here)
            if (!(in >> id >> on >> cfg.mode >> a[0] >> a[1] >> a[2] >> cfg.width >> a[3] >> cfg.phase_col >> a[4] >> cfg.start_blocks >> cfg.phase_lines >> cfg.max_lines)) return 2;
            cfg.black_hz = strtod(a[0].c_str(), nullptr), cfg.white_hz = strtod(a[1].c_str(), nullptr), cfg.lpm = strtod(a[2].c_str(), nullptr);
            cfg.slant_ppm = strtod(a[3].c_str(), nullptr), cfg.tone_ratio = strtod(a[4].c_str(), nullptr);
            const FaxVerdict v = fax_check(c.slots.data(), c.S, id, on ? &cfg : nullptr, rate);
            if (v == FAX_OK) {
                if (on) have = true;  // (first_use of the state and the tables)
                fax_apply(c.slots[id], on ? &cfg : nullptr, rate, 5 * 180);
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

// Runs the RTTY decoder's host side (phantomsdr_amd/csrc/rttyplan.h) over a script from stdin.  Plain host C++:
// tests/test_rtty_host.py builds and runs it.  The slots, their setters and the printed demodulation plan are those of
// tests/demod_plan_table.cpp, whose text is included (its main() under another name); behind every `batch` this program runs
// rtty_plan() as demod.hip does and prints what it yields.  The script, one operation per line:
//   case NAME | size S n nframes | add I | remove I | pause I | resume I | kind I MODE FINE SIDEBAND | window I L MID R
//                               as in demod_plan_table.cpp
//   rate R                      the context's audio_rate (12000 at every `case`)
//   rtty I ON MARK SHIFT BAUD USOS SEARCH SNR   psdr_client_set_rtty_decoder (ON = 0: a null config): rtty_check, then rtty_apply;
//                               prints the verdict (I may be any integer)
//   dump                        the RTTY decoder fields of every slot
//   batch                       demod_plan (printed as demod_plan_table.cpp prints it), then rtty_plan: one `rtp` line
//   defaults RATE               psdr_rtty_defaults
//   tables RATE                 H and the code table, printed
//   run IN OUT                  rtty_stream over one client's stream, batch by batch from zero state.  IN (binary, native endianness):
//                               int32 h, nb, rate, usos; double mark, shift, baud, search, snr_db; int32 frames[nb]; int32 flags[F];
//                               f32 rows[F * h] as bits (F = the sum of frames).  OUT: RttyRec[F]; RttyState[nb] behind each batch;
//                               uint8 text[1024], the ring
#define main demod_plan_table_main
#include "demod_plan_table.cpp"
#undef main

#include "rttyplan.h"

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static const char *verdict_name(RttyVerdict v) {
    switch (v) {
    case RTTY_OK: return "OK";
    case RTTY_BAD_ID: return "BAD_ID";
    case RTTY_INACTIVE: return "INACTIVE";
    case RTTY_IQ: return "IQ";
    case RTTY_BAD_MARK: return "BAD_MARK";
    case RTTY_BAD_SHIFT: return "BAD_SHIFT";
    case RTTY_BAD_BAUD: return "BAD_BAUD";
    case RTTY_BAD_USOS: return "BAD_USOS";
    case RTTY_BAD_SEARCH: return "BAD_SEARCH";
    case RTTY_BAD_SNR: return "BAD_SNR";
    case RTTY_BAD_RATE: return "BAD_RATE";
    case RTTY_BAD_BAND: return "BAD_BAND";
    }
    return "?";
}
static void dump(const Ctx &c) {
    for (size_t i = 0; i < c.S; i++) {
        const AudioSlot &s = c.slots[i];
        printf("rts slot=%zu active=%d on=%d fresh=%d b_on=%d wn=%d u=%d usos=%d ratio=%u lscale=%u cand=%04x inc16=%u inc17=%u\n", i, (int)s.active, s.rtty_on,
               (int)s.rtty_fresh, (int)s.b_rtty_on, s.rtty_wn, s.rtty_u, s.rtty_usos, bits_of(s.rtty_ratio), bits_of(s.rtty_lscale), s.rtty_cand, s.rtty_inc[16],
               s.rtty_inc[17]);
    }
}
// behind demod_plan, as demod_impl calls it (the context's first such client allocates state and tables: `have`)
static void rtty_batch(Ctx &c, uint64_t seq_before, bool have) {
    if (c.seq == seq_before) {  // (a refused batch: nothing moved)
        printf("rtp refused=1\n");
        return;
    }
    std::vector<RttyEntry> table(c.S);
    RttyPlan p;
    if (have) p = rtty_plan(c.slots.data(), c.S, c.seq, table.data());
    printf("rtp have=%d n=%d any=%d zero=", (int)have, p.n, (int)p.any());
    for (size_t j = 0; j < p.zero.size(); j++) printf("%s%zu", j ? "," : "", p.zero[j]);
    printf(" list=");
    for (int j = 0; j < p.n; j++)
        printf("%s%d:%d:%d:%d:%u:%04x:%u", j ? "," : "", table[j].slot, table[j].wn, table[j].u, table[j].usos, bits_of(table[j].ratio), table[j].cand, table[j].inc[16]);
    printf("\n");
}
template <class T>
static void rd(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) exit(3);
}
static int run_file(const std::string &in, const std::string &out) {
    FILE *f = fopen(in.c_str(), "rb");
    if (!f) return 3;
    int32_t head[4];
    double par[5];
    rd(f, head, 4);
    rd(f, par, 5);
    const int h = head[0], nb = head[1], rate = head[2];
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
    psdr_rtty_config cfg;
    cfg.mark_hz = par[0], cfg.shift_hz = par[1], cfg.baud = par[2], cfg.usos = head[3], cfg.search_hz = par[3], cfg.snr_db = par[4];
    if (rtty_check(&slot, 1, 0, &cfg, rate) != RTTY_OK) return 4;
    rtty_apply(slot, &cfg, rate);
    RttyEntry e;
    rtty_entry(e, 0, slot);
    std::vector<RttyTables> t(1);
    rtty_tables(t[0], (double)rate);
    std::vector<RttyRec> rec(F);
    std::vector<RttyState> states;
    std::vector<uint8_t> text(RTTY_TEXT, 0);
    RttyState st;
    memset(&st, 0, sizeof(st));
    size_t at = 0;
    for (int b = 0; b < nb; b++) {
        rtty_stream(t[0], e, rows.data() + at * h, flags.data() + at, h, frames[b], st, text.data(), rec.data() + at);
        at += (size_t)frames[b];
        states.push_back(st);
    }
    FILE *g = fopen(out.c_str(), "wb");
    if (!g) return 3;
    if (fwrite(rec.data(), sizeof(RttyRec), F, g) != F || fwrite(states.data(), sizeof(RttyState), states.size(), g) != states.size() ||
        fwrite(text.data(), 1, RTTY_TEXT, g) != (size_t)RTTY_TEXT)
        return 3;
    fclose(g);
    printf("run frames=%zu h=%d nb=%d H=%d wn=%d u=%d ratio=%u\n", F, h, nb, t[0].H, e.wn, e.u, bits_of(e.ratio));
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
            rtty_batch(c, before, have);
        } else if (op == "dump") {
            dump(c);
        } else if (op == "defaults") {
            if (!(in >> w)) return 2;
            const double r = strtod(w.c_str(), nullptr);
            psdr_rtty_config d;
            memset(&d, 0, sizeof(d));
            const bool ok = rtty_defaults(r, &d);
            printf("defaults rate=%.17g ok=%d mark_hz=%.17g shift_hz=%.17g baud=%.17g usos=%d search_hz=%.17g snr_db=%.17g\n", r, (int)ok, d.mark_hz, d.shift_hz, d.baud, d.usos,
                   d.search_hz, d.snr_db);
        } else if (op == "tables") {
            double r = 0;
            if (!(in >> r)) return 2;
            std::vector<RttyTables> t(1);
            rtty_tables(t[0], r);
            printf("tables rate=%.17g H=%d wn45=%d wn75=%d u4545=%d baudot=", r, t[0].H, rtty_wn_of(45.0, r), rtty_wn_of(75.0, r), rtty_u_of(45.45, r));
            for (int s = 0; s < 2; s++)
                for (int j = 0; j < 32; j++) printf("%02x", t[0].baudot[s][j]);
            printf("\n");
        } else if (op == "run") {
            std::string fin, fout;
            if (!(in >> fin >> fout)) return 2;
            const int rc = run_file(fin, fout);
            if (rc) return rc;
        } else if (op == "rtty") {
            int id = 0, on = 0;
            psdr_rtty_config cfg;
            std::string a[5];  // (strtod: "nan" and "inf" are values here)
            if (!(in >> id >> on >> a[0] >> a[1] >> a[2] >> cfg.usos >> a[3] >> a[4])) return 2;
            cfg.mark_hz = strtod(a[0].c_str(), nullptr), cfg.shift_hz = strtod(a[1].c_str(), nullptr), cfg.baud = strtod(a[2].c_str(), nullptr);
            cfg.search_hz = strtod(a[3].c_str(), nullptr), cfg.snr_db = strtod(a[4].c_str(), nullptr);
            const RttyVerdict v = rtty_check(c.slots.data(), c.S, id, on ? &cfg : nullptr, rate);
            if (v == RTTY_OK) {
                if (on) have = true;  // (first_use of the state and the tables)
                rtty_apply(c.slots[id], on ? &cfg : nullptr, rate);
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

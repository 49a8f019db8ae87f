// Runs the PSK31 decoder's host side (phantomsdr_amd/csrc/pskplan.h) over a script from stdin.  Plain host C++:
// tests/test_psk_host.py builds and runs it.  The slots, their setters and the printed demodulation plan are those of
// tests/demod_plan_table.cpp, whose text is included (its main() under another name); behind every `batch` this program runs
// psk_plan() as demod.hip does and prints what it yields.  The script, one operation per line:
//   case NAME | size S n nframes | add I | remove I | pause I | resume I | kind I MODE FINE SIDEBAND | window I L MID R
//                               as in demod_plan_table.cpp
//   rate R                      the context's audio_rate (12000 at every `case`)
//   psk I ON CARRIER BAUD SEARCH QUALITY   psdr_client_set_psk_decoder (ON = 0: a null config): psk_check, then psk_apply; prints the
//                               verdict (I may be any integer)
//   dump                        the PSK decoder fields of every slot
//   batch                       demod_plan (printed as demod_plan_table.cpp prints it), then psk_plan: one `pkp` line
//   defaults RATE               psdr_psk_defaults
//   tables RATE                 H, the windows and the varicode table by character, printed
//   run IN OUT                  psk_stream over one client's stream, batch by batch from zero state.  IN (binary, native endianness):
//                               int32 h, nb, rate, pad; double carrier, baud, search, quality; int32 frames[nb]; int32 flags[F];
//                               f32 rows[F * h] as bits (F = the sum of frames).  OUT: PskRec[F]; PskState[nb] behind each batch;
//                               uint8 text[1024], the ring
#define main demod_plan_table_main
#include "demod_plan_table.cpp"
#undef main

#include "pskplan.h"

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static const char *verdict_name(PskVerdict v) {
    switch (v) {
    case PSK_OK: return "OK";
    case PSK_BAD_ID: return "BAD_ID";
    case PSK_INACTIVE: return "INACTIVE";
    case PSK_IQ: return "IQ";
    case PSK_BAD_CARRIER: return "BAD_CARRIER";
    case PSK_BAD_BAUD: return "BAD_BAUD";
    case PSK_BAD_SEARCH: return "BAD_SEARCH";
    case PSK_BAD_QUALITY: return "BAD_QUALITY";
    case PSK_BAD_RATE: return "BAD_RATE";
    case PSK_BAD_BAND: return "BAD_BAND";
    }
    return "?";
}
static void dump(const Ctx &c) {
    for (size_t i = 0; i < c.S; i++) {
        const AudioSlot &s = c.slots[i];
        printf("pks slot=%zu active=%d on=%d fresh=%d b_on=%d wn=%d u=%d quality=%u lscale=%u df=%u cand=%04x inc0=%u inc8=%u inc15=%u\n", i, (int)s.active, s.psk_on,
               (int)s.psk_fresh, (int)s.b_psk_on, s.psk_wn, s.psk_u, bits_of(s.psk_quality), bits_of(s.psk_lscale), bits_of(s.psk_df), s.psk_cand, s.psk_inc[0],
               s.psk_inc[8], s.psk_inc[15]);
    }
}
// behind demod_plan, as demod_impl calls it (the context's first such client allocates state and tables: `have`)
static void psk_batch(Ctx &c, uint64_t seq_before, bool have) {
    if (c.seq == seq_before) {  // (a refused batch: nothing moved)
        printf("pkp refused=1\n");
        return;
    }
    std::vector<PskEntry> table(c.S);
    PskPlan p;
    if (have) p = psk_plan(c.slots.data(), c.S, c.seq, table.data());
    printf("pkp have=%d n=%d any=%d zero=", (int)have, p.n, (int)p.any());
    for (size_t j = 0; j < p.zero.size(); j++) printf("%s%zu", j ? "," : "", p.zero[j]);
    printf(" list=");
    for (int j = 0; j < p.n; j++)
        printf("%s%d:%d:%d:%u:%04x:%u", j ? "," : "", table[j].slot, table[j].wn, table[j].u, bits_of(table[j].quality), table[j].cand, table[j].inc[8]);
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
    double par[4];
    rd(f, head, 4);
    rd(f, par, 4);
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
    psdr_psk_config cfg;
    cfg.carrier_hz = par[0], cfg.baud = par[1], cfg.search_hz = par[2], cfg.quality = par[3];
    if (psk_check(&slot, 1, 0, &cfg, rate) != PSK_OK) return 4;
    psk_apply(slot, &cfg, rate);
    PskEntry e;
    psk_entry(e, 0, slot);
    std::vector<PskTables> t(1);
    psk_tables(t[0], (double)rate);
    std::vector<PskRec> rec(F);
    std::vector<PskState> states;
    std::vector<uint8_t> text(PSK_TEXT, 0);
    PskState st;
    memset(&st, 0, sizeof(st));
    size_t at = 0;
    for (int b = 0; b < nb; b++) {
        psk_stream(t[0], e, rows.data() + at * h, flags.data() + at, h, frames[b], st, text.data(), rec.data() + at);
        at += (size_t)frames[b];
        states.push_back(st);
    }
    FILE *g = fopen(out.c_str(), "wb");
    if (!g) return 3;
    if (fwrite(rec.data(), sizeof(PskRec), F, g) != F || fwrite(states.data(), sizeof(PskState), states.size(), g) != states.size() ||
        fwrite(text.data(), 1, PSK_TEXT, g) != (size_t)PSK_TEXT)
        return 3;
    fclose(g);
    printf("run frames=%zu h=%d nb=%d H=%d wn=%d u=%d quality=%u\n", F, h, nb, t[0].H, e.wn, e.u, bits_of(e.quality));
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
            psk_batch(c, before, have);
        } else if (op == "dump") {
            dump(c);
        } else if (op == "defaults") {
            if (!(in >> w)) return 2;
            const double r = strtod(w.c_str(), nullptr);
            psdr_psk_config d;
            memset(&d, 0, sizeof(d));
            const bool ok = psk_defaults(r, &d);
            printf("defaults rate=%.17g ok=%d carrier_hz=%.17g baud=%.17g search_hz=%.17g quality=%.17g\n", r, (int)ok, d.carrier_hz, d.baud, d.search_hz, d.quality);
        } else if (op == "tables") {
            double r = 0;
            if (!(in >> r)) return 2;
            std::vector<PskTables> t(1);
            psk_tables(t[0], r);
            printf("tables rate=%.17g H=%d wn31=%d wn63=%d u31=%d u63=%d fill=%d varicode=", r, t[0].H, psk_wn_of(31.25, r), psk_wn_of(62.5, r), psk_u_of(31.25, r),
                   psk_u_of(62.5, r), PSK_FILL);
            for (int ch = 0; ch < 128; ch++) printf("%s%x", ch ? "," : "", (unsigned)PSK_VARICODE[ch]);
            int known = 0, wrong = 0;  // the table by code is the table by character, turned round
            for (int code = 0; code < 1024; code++)
                if (t[0].vari[code]) known++, wrong += PSK_VARICODE[t[0].vari[code] - 1] != code;
            printf(" known=%d wrong=%d\n", known, wrong);
        } else if (op == "run") {
            std::string fin, fout;
            if (!(in >> fin >> fout)) return 2;
            const int rc = run_file(fin, fout);
            if (rc) return rc;
        } else if (op == "psk") {
            int id = 0, on = 0;
            psdr_psk_config cfg;
            std::string a[4];  // (strtod: "nan" and "inf" are values here)
            if (!(in >> id >> on >> a[0] >> a[1] >> a[2] >> a[3])) return 2;
            cfg.carrier_hz = strtod(a[0].c_str(), nullptr), cfg.baud = strtod(a[1].c_str(), nullptr);
            cfg.search_hz = strtod(a[2].c_str(), nullptr), cfg.quality = strtod(a[3].c_str(), nullptr);
            const PskVerdict v = psk_check(c.slots.data(), c.S, id, on ? &cfg : nullptr, rate);
            if (v == PSK_OK) {
                if (on) have = true;  // (first_use of the state and the tables)
                psk_apply(c.slots[id], on ? &cfg : nullptr, rate);
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

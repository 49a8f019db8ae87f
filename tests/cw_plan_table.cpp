// Runs the CW decoder's host side (phantomsdr_amd/csrc/cwplan.h) over a script from stdin.  Plain host C++:
// tests/test_cw_host.py builds and runs it.  The slots, their setters and the printed demodulation plan are those of
// tests/demod_plan_table.cpp, whose text is included (its main() under another name); behind every `batch` this program runs
// cw_plan() as demod.hip does and prints what it yields.  The script, one operation per line:
//   case NAME | size S n nframes | add I | remove I | pause I | resume I | kind I MODE FINE SIDEBAND | window I L MID R
//                               as in demod_plan_table.cpp
//   rate R                      the context's audio_rate (12000 at every `case`)
//   cw I ON PITCH SEARCH WPM TRACK SNR   psdr_client_set_cw_decoder (ON = 0: a null config): cw_check, then cw_apply; prints the
//                               verdict (I may be any integer)
//   dump                        the CW decoder fields of every slot
//   batch                       demod_plan (printed as demod_plan_table.cpp prints it), then cw_plan: one `cwp` line
//   defaults RATE               psdr_cw_defaults
//   tables RATE                 H, umin, umax, lscale, the lanes' increments and the Morse table, printed
//   keying RATE WPM TRACK RAW   cw_key_step over a string of 0 / 1 raw keys from the start: the text and the dot length behind it
//   run IN OUT                  cw_stream over one client's stream, batch by batch from zero state.  IN (binary, native endianness):
//                               int32 h, nb, rate, track; double pitch, search, wpm, snr_db; int32 frames[nb]; int32 flags[F];
//                               f32 rows[F * h] as bits (F = the sum of frames).  OUT: CwRec[F]; CwState[nb] behind each batch;
//                               uint8 text[1024], the ring
#define main demod_plan_table_main
#include "demod_plan_table.cpp"
#undef main

#include "cwplan.h"

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static const char *verdict_name(CwVerdict v) {
    switch (v) {
    case CW_OK: return "OK";
    case CW_BAD_ID: return "BAD_ID";
    case CW_INACTIVE: return "INACTIVE";
    case CW_IQ: return "IQ";
    case CW_BAD_PITCH: return "BAD_PITCH";
    case CW_BAD_SEARCH: return "BAD_SEARCH";
    case CW_BAD_WPM: return "BAD_WPM";
    case CW_BAD_TRACK: return "BAD_TRACK";
    case CW_BAD_SNR: return "BAD_SNR";
    case CW_BAD_RATE: return "BAD_RATE";
    }
    return "?";
}
static void dump(const Ctx &c) {
    for (size_t i = 0; i < c.S; i++) {
        const AudioSlot &s = c.slots[i];
        printf("cws slot=%zu active=%d on=%d fresh=%d b_on=%d p0=%d u0=%d track=%d ratio=%u cand=%016" PRIx64 "\n", i, (int)s.active, s.cw_on, (int)s.cw_fresh, (int)s.b_cw_on,
               s.cw_p0, s.cw_u0, s.cw_track, bits_of(s.cw_ratio), s.cw_cand);
    }
}
// behind demod_plan, as demod_impl calls it (the context's first such client allocates state and tables: `have`)
static void cw_batch(Ctx &c, uint64_t seq_before, bool have) {
    if (c.seq == seq_before) {  // (a refused batch: nothing moved)
        printf("cwp refused=1\n");
        return;
    }
    std::vector<CwEntry> table(c.S);
    CwPlan p;
    if (have) p = cw_plan(c.slots.data(), c.S, c.seq, table.data());
    printf("cwp have=%d n=%d any=%d zero=", (int)have, p.n, (int)p.any());
    for (size_t j = 0; j < p.zero.size(); j++) printf("%s%zu", j ? "," : "", p.zero[j]);
    printf(" list=");
    for (int j = 0; j < p.n; j++)
        printf("%s%d:%d:%d:%d:%u:%016" PRIx64, j ? "," : "", table[j].slot, table[j].p0, table[j].u0, table[j].track, bits_of(table[j].ratio), table[j].cand);
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
    psdr_cw_config cfg;
    cfg.pitch_hz = par[0], cfg.search_hz = par[1], cfg.wpm = par[2], cfg.track_speed = head[3], cfg.snr_db = par[3];
    if (cw_check(&slot, 1, 0, &cfg, rate) != CW_OK) return 4;
    cw_apply(slot, &cfg, rate);
    const CwEntry e{0, slot.cw_p0, slot.cw_u0, slot.cw_track, slot.cw_ratio, 0, slot.cw_cand};
    std::vector<CwTables> t(1);
    cw_tables(t[0], (double)rate);
    std::vector<CwRec> rec(F);
    std::vector<CwState> states;
    std::vector<uint8_t> text(CW_TEXT, 0);
    CwState st;
    memset(&st, 0, sizeof(st));
    size_t at = 0;
    for (int b = 0; b < nb; b++) {
        cw_stream(t[0], e, rows.data() + at * h, flags.data() + at, h, frames[b], st, text.data(), rec.data() + at);
        at += (size_t)frames[b];
        states.push_back(st);
    }
    FILE *g = fopen(out.c_str(), "wb");
    if (!g) return 3;
    if (fwrite(rec.data(), sizeof(CwRec), F, g) != F || fwrite(states.data(), sizeof(CwState), states.size(), g) != states.size() ||
        fwrite(text.data(), 1, CW_TEXT, g) != (size_t)CW_TEXT)
        return 3;
    fclose(g);
    printf("run frames=%zu h=%d nb=%d H=%d p0=%d u0=%d ratio=%u\n", F, h, nb, t[0].H, e.p0, e.u0, bits_of(e.ratio));
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
            cw_batch(c, before, have);
        } else if (op == "dump") {
            dump(c);
        } else if (op == "defaults") {
            if (!(in >> w)) return 2;
            const double r = strtod(w.c_str(), nullptr);
            psdr_cw_config d;
            memset(&d, 0, sizeof(d));
            const bool ok = cw_defaults(r, &d);
            printf("defaults rate=%.17g ok=%d pitch_hz=%.17g search_hz=%.17g wpm=%.17g track_speed=%d snr_db=%.17g\n", r, (int)ok, d.pitch_hz, d.search_hz, d.wpm,
                   d.track_speed, d.snr_db);
        } else if (op == "tables") {
            double r = 0;
            if (!(in >> r)) return 2;
            std::vector<CwTables> t(1);
            cw_tables(t[0], r);
            printf("tables rate=%.17g H=%d umin=%d umax=%d lscale=%u u20=%d wpm20=%u inc=", r, t[0].H, t[0].umin, t[0].umax, bits_of(t[0].lscale), cw_u_of(20.0, r),
                   bits_of(t[0].wpm[cw_u_of(20.0, r)]));
            for (int k = 0; k < CW_LANES; k++) printf("%s%u", k ? "," : "", t[0].t.inc[k]);
            printf(" morse=");
            for (int j = 0; j < 256; j++) printf("%02x", t[0].morse[j]);
            printf("\n");
        } else if (op == "keying") {
            double r = 0, wpm = 0;
            int track = 0;
            if (!(in >> r >> wpm >> track >> w)) return 2;
            std::vector<CwTables> t(1);
            cw_tables(t[0], r);
            CwKey k;
            memset(&k, 0, sizeof(k));
            k.u = cw_u_of(wpm, r);
            std::string text;
            for (char ch : w) {
                for (uint32_t out = cw_key_step(k, ch == '1', track, t[0].umin, t[0].umax, t[0].morse); out; out >>= 8) text += (char)(out & 255);
            }
            printf("keying u=%d key=%d text=[%s]\n", k.u, k.key, text.c_str());
        } else if (op == "run") {
            std::string fin, fout;
            if (!(in >> fin >> fout)) return 2;
            const int rc = run_file(fin, fout);
            if (rc) return rc;
        } else if (op == "cw") {
            int id = 0, on = 0;
            psdr_cw_config cfg;
            std::string a[4];  // (strtod: "nan" and "inf" are values here)
            if (!(in >> id >> on >> a[0] >> a[1] >> a[2] >> cfg.track_speed >> a[3])) return 2;
            cfg.pitch_hz = strtod(a[0].c_str(), nullptr), cfg.search_hz = strtod(a[1].c_str(), nullptr);
            cfg.wpm = strtod(a[2].c_str(), nullptr), cfg.snr_db = strtod(a[3].c_str(), nullptr);
            const CwVerdict v = cw_check(c.slots.data(), c.S, id, on ? &cfg : nullptr, rate);
            if (v == CW_OK) {
                if (on) have = true;  // (first_use of the state and the tables)
                cw_apply(c.slots[id], on ? &cfg : nullptr, rate);
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

// Runs the tone decoder's host side (phantomsdr_amd/csrc/toneplan.h) over a script from stdin.  Plain host C++:
// tests/test_tone_host.py builds and runs it.  The slots, their setters and the printed demodulation plan are those of
// tests/demod_plan_table.cpp, whose text is included (its main() under another name); behind every `batch` this program runs
// tone_plan() as demod.hip does and prints what it yields.  The script, one operation per line:
//   case NAME | size S n nframes | add I | remove I | pause I | resume I | kind I MODE FINE SIDEBAND | window I L MID R | post on|off
//                               as in demod_plan_table.cpp
//   rate R                      the context's audio_rate (12000 at every `case`)
//   tone I ON WANT GATE SNR LEVEL ATTACK HANG   psdr_client_set_tone_decoder (ON = 0: a null config): tone_check, then tone_apply;
//                               prints the verdict (I may be any integer)
//   dump                        the tone decoder fields of every slot
//   batch                       demod_plan (printed as demod_plan_table.cpp prints it), then tone_plan: one `tonep` line
//   defaults RATE               psdr_tone_defaults
//   tables RATE OUT             ToneTables as the device gets it (binary)
//   gate ATTACK HANG HITS       tone_gate over a string of 0 / 1 decisions from (closed, 0): the gate and the tone behind each
//   frames POS0 H NFRAMES       the number of complete blocks at each frame's end, from tone_first_frame as tone_stream uses it
//   run IN OUT                  tone_stream over one client's stream, batch by batch from zero state.  IN (binary, native endianness):
//                               int32 h, nb, rate, want, gate, attack, hang; double snr_db, min_level; int32 frames[nb]; int32 flags[F];
//                               int32 prev_drop[F]; f32 rows[F * h] as bits (F = the sum of frames).  OUT: ToneRec[F]; int32 drop[F];
//                               ToneState[nb] behind each batch
#define main demod_plan_table_main
#include "demod_plan_table.cpp"
#undef main

#include "toneplan.h"

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static const char *verdict_name(ToneVerdict v) {
    switch (v) {
    case TONE_OK: return "OK";
    case TONE_BAD_ID: return "BAD_ID";
    case TONE_INACTIVE: return "INACTIVE";
    case TONE_IQ: return "IQ";
    case TONE_BAD_WANT: return "BAD_WANT";
    case TONE_BAD_GATE: return "BAD_GATE";
    case TONE_BAD_SNR: return "BAD_SNR";
    case TONE_BAD_LEVEL: return "BAD_LEVEL";
    case TONE_BAD_ATTACK: return "BAD_ATTACK";
    case TONE_BAD_HANG: return "BAD_HANG";
    case TONE_BAD_RATE: return "BAD_RATE";
    }
    return "?";
}
static void dump(const Ctx &c) {
    for (size_t i = 0; i < c.S; i++) {
        const AudioSlot &s = c.slots[i];
        printf("tones slot=%zu active=%d on=%d fresh=%d b_on=%d want=%d gate=%d attack=%d hang=%d ratio=%u min_level=%u\n", i, (int)s.active, s.tone_on, (int)s.tone_fresh,
               (int)s.b_tone_on, s.tone_want, s.tone_gate, s.tone_attack, s.tone_hang, bits_of(s.tone_ratio), bits_of(s.tone_min_level));
    }
}
// behind demod_plan, as demod_impl calls it (the context's first such client allocates state and tables: `have`)
static void tone_batch(Ctx &c, uint64_t seq_before, bool have) {
    if (c.seq == seq_before) {  // (a refused batch: nothing moved)
        printf("tonep refused=1\n");
        return;
    }
    std::vector<ToneEntry> table(c.S);
    TonePlan p;
    int nact = 0;
    for (size_t i = 0; i < c.S; i++) nact += c.slots[i].active && !c.slots[i].paused && c.slots[i].last_seq == c.seq;
    if (have) p = tone_plan(c.slots.data(), c.S, c.seq, c.f.post_on && nact > 0, table.data());
    printf("tonep have=%d n=%d ncopy=%d gated=%d any=%d zero=", (int)have, p.n, p.ncopy, (int)p.gated, (int)p.any());
    for (size_t j = 0; j < p.zero.size(); j++) printf("%s%zu", j ? "," : "", p.zero[j]);
    printf(" list=");
    for (int j = 0; j < p.n + p.ncopy; j++)
        printf("%s%d:%d:%d:%d:%d:%u:%u", j ? "," : "", table[j].slot, table[j].want, table[j].gate, table[j].attack, table[j].hang, bits_of(table[j].ratio),
               bits_of(table[j].min_level));
    printf("\n");
}
template <class T>
static void rd(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) exit(3);
}
static int run_file(const std::string &in, const std::string &out) {
    FILE *f = fopen(in.c_str(), "rb");
    if (!f) return 3;
    int32_t head[7];
    double par[2];
    rd(f, head, 7);
    rd(f, par, 2);
    const int h = head[0], nb = head[1], rate = head[2];
    if (h < 1 || nb < 1) return 3;
    std::vector<int32_t> frames(nb);
    rd(f, frames.data(), nb);
    size_t F = 0;
    for (int32_t v : frames) {
        if (v < 1) return 3;
        F += (size_t)v;
    }
    std::vector<int32_t> flags(F), prev(F), drop(F);
    std::vector<float> rows(F * h);
    rd(f, flags.data(), F);
    rd(f, prev.data(), F);
    rd(f, rows.data(), F * h);
    fclose(f);
    AudioSlot slot;
    slot.active = true;
    psdr_tone_config cfg;
    cfg.want = head[3], cfg.gate = head[4], cfg.attack_blocks = head[5], cfg.hang_blocks = head[6];
    cfg.snr_db = par[0], cfg.min_level = par[1];
    if (tone_check(&slot, 1, 0, &cfg, rate) != TONE_OK) return 4;
    tone_apply(slot, &cfg);
    const ToneEntry e{0, slot.tone_want, slot.tone_gate, slot.tone_attack, slot.tone_hang, slot.tone_ratio, slot.tone_min_level, 0};
    std::vector<ToneTables> t(1);
    tone_tables(t[0], (double)rate);
    std::vector<ToneC> hist((size_t)tone_ring(t[0].nb) * TONE_LANES, ToneC{0.f, 0.f});
    std::vector<ToneRec> rec(F);
    std::vector<ToneState> states;
    ToneState st;
    memset(&st, 0, sizeof(st));
    size_t at = 0;
    for (int b = 0; b < nb; b++) {
        tone_stream(t[0], e, rows.data() + at * h, flags.data() + at, h, frames[b], st, hist.data(), rec.data() + at, prev.data() + at, drop.data() + at);
        at += (size_t)frames[b];
        states.push_back(st);
    }
    FILE *g = fopen(out.c_str(), "wb");
    if (!g) return 3;
    if (fwrite(rec.data(), sizeof(ToneRec), F, g) != F || fwrite(drop.data(), 4, F, g) != F || fwrite(states.data(), sizeof(ToneState), states.size(), g) != states.size())
        return 3;
    fclose(g);
    printf("run frames=%zu h=%d nb=%d window=%d ratio=%u lscale=%u\n", F, h, nb, t[0].nb, bits_of(e.ratio), bits_of(t[0].lscale));
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
            tone_batch(c, before, have);
        } else if (op == "post") {
            in >> w;
            c.f.post_on = w == "on";
        } else if (op == "dump") {
            dump(c);
        } else if (op == "defaults") {
            double r = 0;
            if (!(in >> w)) return 2;
            r = strtod(w.c_str(), nullptr);
            psdr_tone_config d;
            memset(&d, 0, sizeof(d));
            const bool ok = tone_defaults(r, &d);
            printf("defaults rate=%.17g ok=%d want=%d gate=%d snr_db=%.17g min_level=%.17g attack=%d hang=%d\n", r, (int)ok, d.want, d.gate, d.snr_db, d.min_level,
                   d.attack_blocks, d.hang_blocks);
        } else if (op == "tables") {
            double r = 0;
            if (!(in >> r >> w)) return 2;
            std::vector<ToneTables> t(1);
            tone_tables(t[0], r);
            FILE *g = fopen(w.c_str(), "wb");
            if (!g || fwrite(t.data(), sizeof(ToneTables), 1, g) != 1) return 3;
            fclose(g);
            printf("tables bytes=%zu nb=%d\n", sizeof(ToneTables), t[0].nb);
        } else if (op == "gate") {
            ToneEntry e{0, -1, 1, 0, 0, 1.f, 0.f, 0};
            if (!(in >> e.attack >> e.hang >> w)) return 2;
            SquelchState g{0, 0};
            int tp1 = 0;
            float level = 0.f;
            printf("gate attack=%d hang=%d open=", e.attack, e.hang);
            std::string tones;
            for (char ch : w) {
                tone_gate(g, tp1, level, ch == '1', 7, 0.5f, e);
                printf("%d", g.open);
                tones += tp1 ? '7' : '-';
            }
            printf(" tone=%s cnt=%d\n", tones.c_str(), g.cnt);
        } else if (op == "frames") {
            uint64_t pos0 = 0;
            int h = 0, nframes = 0;
            if (!(in >> pos0 >> h >> nframes) || h < 1) return 2;
            const uint64_t b0 = pos0 / TONE_B, b1 = (pos0 + (uint64_t)nframes * h) / TONE_B;
            std::vector<long long> done(nframes, -1);
            for (uint64_t D = b0; D <= b1; D++)
                for (int f = tone_first_frame(D, pos0, h); f < std::min(nframes, tone_first_frame(D + 1, pos0, h)); f++) done[f] = (long long)D;
            printf("frames pos0=%" PRIu64 " h=%d done=", pos0, h);
            for (int f = 0; f < nframes; f++) printf("%s%lld", f ? "," : "", done[f]);
            printf("\n");
        } else if (op == "run") {
            std::string fin, fout;
            if (!(in >> fin >> fout)) return 2;
            const int rc = run_file(fin, fout);
            if (rc) return rc;
        } else if (op == "tone") {
            int id = 0, on = 0;
            psdr_tone_config cfg;
            std::string a[2];  // (strtod: "nan" and "inf" are values here)
            if (!(in >> id >> on >> cfg.want >> cfg.gate >> a[0] >> a[1] >> cfg.attack_blocks >> cfg.hang_blocks)) return 2;
            cfg.snr_db = strtod(a[0].c_str(), nullptr), cfg.min_level = strtod(a[1].c_str(), nullptr);
            const ToneVerdict v = tone_check(c.slots.data(), c.S, id, on ? &cfg : nullptr, rate);
            if (v == TONE_OK) {
                if (on) have = true;  // (first_use of the state and the tables)
                tone_apply(c.slots[id], on ? &cfg : nullptr);
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

// Runs the squelch's host side (phantomsdr_amd/csrc/squelchplan.h) over a script from stdin.  Plain host C++:
// tests/test_squelch_host.py builds and runs it.  The slots, their setters and the printed demodulation plan are those of
// tests/demod_plan_table.cpp, whose text is included (its main() under another name); behind every `batch` this program runs
// squelch_plan() as demod.hip does and prints what it yields.  The script, one operation per line:
//   case NAME | size S n nframes | add I | remove I | pause I | resume I | kind I MODE FINE SIDEBAND | window I L MID R | post on|off
//                               as in demod_plan_table.cpp
//   squelch I ON OPEN_DB CLOSE_DB ATTACK HANG
//                               psdr_client_set_squelch: squelch_check, then squelch_apply; prints the verdict (I may be any integer)
//   dump                        the squelch fields of every slot
//   batch                       demod_plan (printed as demod_plan_table.cpp prints it), then squelch_plan: one `sq` line
//   db V                        squelch_threshold(V) as the bits of the f32
//   steps TOPEN TCLOSE ATTACK HANG N P_0 .. P_N-1
//                               thresholds and pwr values as f32 bits.  For EVERY split of the N frames into consecutive batches
//                               (mask: bit b set = a batch ends behind frame b): the state carried from (closed, 0) through the
//                               batches, each walked as k_squelch walks it - chunks of 64 frames, two comparison masks,
//                               squelch_walk - and, beside it, frame by frame through squelch_frame
//   run TOPEN TCLOSE ATTACK HANG N NB LEN_1 .. LEN_NB P_0 .. P_N-1
//                               the same for ONE split, the batches' lengths given (any N: batches longer than a chunk)
#define main demod_plan_table_main
#include "demod_plan_table.cpp"
#undef main

#include "squelchplan.h"

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
static const char *verdict_name(SquelchVerdict v) {
    switch (v) {
    case SQ_OK: return "OK";
    case SQ_BAD_ID: return "BAD_ID";
    case SQ_BAD_DB: return "BAD_DB";
    case SQ_CLOSE_ABOVE_OPEN: return "CLOSE_ABOVE_OPEN";
    case SQ_BAD_ATTACK: return "BAD_ATTACK";
    case SQ_BAD_HANG: return "BAD_HANG";
    }
    return "?";
}
static void dump(const Ctx &c) {
    for (size_t i = 0; i < c.S; i++) {
        const AudioSlot &s = c.slots[i];
        printf("sqs slot=%zu active=%d on=%d topen=%u tclose=%u attack=%d hang=%d b_on=%d fresh=%d\n", i, (int)s.active, s.sq_on, bits_of(s.sq_t_open),
               bits_of(s.sq_t_close), s.sq_attack, s.sq_hang, (int)s.b_sq_on, (int)s.sq_fresh);
    }
}
// behind demod_plan, as demod_impl calls it: the chain runs behind a batch with an audio client when it is on
static void squelch_batch(Ctx &c, uint64_t seq_before) {
    if (c.seq == seq_before) {  // (a refused batch: nothing moved)
        printf("sq refused=1\n");
        return;
    }
    bool audio = false;
    for (const AudioSlot &s : c.slots) audio |= s.active && !s.paused && s.last_seq == c.seq && s.b_mode != PSDR_IQ;
    std::vector<SquelchEntry> table(c.S);
    const SquelchPlan p = squelch_plan(c.slots.data(), c.S, c.seq, c.f.post_on && audio, table.data());
    printf("sq nsq=%d ncopy=%d lo=%d n=%d any=%d zero=", p.nsq, p.ncopy, p.lo, p.n, (int)p.any());
    for (size_t j = 0; j < p.zero.size(); j++) printf("%s%zu", j ? "," : "", p.zero[j]);
    printf(" list=");
    for (int j = 0; j < p.nsq + p.ncopy; j++)
        printf("%s%d:%d:%d:%d:%u:%u", j ? "," : "", table[j].slot, table[j].attack, table[j].hang, table[j].pad, bits_of(table[j].t_open), bits_of(table[j].t_close));
    printf("\n");
}
// the frames pw walked as the batches that end behind the frames `ends` (ascending, the last one = the last frame)
static void walk(const std::vector<float> &pw, const SquelchEntry &e, const std::vector<int> &ends, uint32_t mask) {
    SquelchState st{0, 0}, sf{0, 0};
    std::string flags, flags_f;
    for (float v : pw) flags_f += squelch_frame(sf, v, e) ? '1' : '0';
    int f0 = 0;
    for (int f : ends) {
        // one batch [f0, f]: chunks of 64 frames
        for (int c0 = f0; c0 <= f; c0 += 64) {
            const int cnt = std::min(64, f + 1 - c0);
            unsigned long long ge_open = 0, ge_close = 0;
            for (int j = 0; j < cnt; j++) {
                if (squelch_ge(pw[c0 + j], e.t_open)) ge_open |= 1ull << j;
                if (squelch_ge(pw[c0 + j], e.t_close)) ge_close |= 1ull << j;
            }
            const unsigned long long heard = squelch_walk(st, ge_open, ge_close, cnt, e.attack, e.hang);
            for (int j = 0; j < cnt; j++) flags += (heard >> j) & 1ull ? '1' : '0';
        }
        f0 = f + 1;
    }
    printf("st mask=%u flags=%s open=%d cnt=%d frame_flags=%s frame_open=%d frame_cnt=%d\n", mask, flags.c_str(), st.open, st.cnt, flags_f.c_str(), sf.open, sf.cnt);
}
// every: `steps` (N <= 20, every split); else `run`: ONE split, the batch lengths in front of the values
static void steps(std::istringstream &in, bool every) {
    uint32_t to = 0, tc = 0;
    int attack = 0, hang = 0, n = 0;
    if (!(in >> to >> tc >> attack >> hang >> n) || n < 1 || (every && n > 20)) exit(2);
    std::vector<int> ends;
    if (!every) {
        int nb = 0, at = 0;
        if (!(in >> nb) || nb < 1) exit(2);
        for (int b = 0; b < nb; b++) {
            int len = 0;
            if (!(in >> len) || len < 1) exit(2);
            ends.push_back((at += len) - 1);
        }
        if (at != n) exit(2);
    }
    std::vector<float> pw(n);
    for (float &v : pw) {
        uint32_t u = 0;
        if (!(in >> u)) exit(2);
        v = float_of(u);
    }
    const SquelchEntry e{0, attack, hang, 0, float_of(to), float_of(tc)};
    if (!every) return walk(pw, e, ends, 0);
    for (uint32_t mask = 0; mask < (1u << (n - 1)); mask++) {
        ends.clear();
        for (int f = 0; f < n; f++)
            if (f + 1 == n || ((mask >> f) & 1u)) ends.push_back(f);
        walk(pw, e, ends, mask);
    }
}

int main() {
    Ctx c;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, w;
        if (!(in >> op)) continue;
        if (op == "case") {
            in >> w;
            c.resize(8, 360, 5);
            printf("case name=%s\n", w.c_str());
        } else if (op == "size") {
            size_t S = 0;
            int n = 0, nframes = 0;
            if (!(in >> S >> n >> nframes) || S == 0) return 2;
            c.resize(S, n, nframes);
        } else if (op == "batch") {
            const uint64_t before = c.seq;
            batch(c);
            squelch_batch(c, before);
        } else if (op == "post") {
            in >> w;
            c.f.post_on = w == "on";
        } else if (op == "dump") {
            dump(c);
        } else if (op == "db") {
            double v = 0;
            if (!(in >> v)) return 2;
            printf("db v=%.17g bits=%u\n", v, bits_of(squelch_threshold(v)));
        } else if (op == "steps" || op == "run") {
            steps(in, op == "steps");
        } else if (op == "squelch") {
            int id = 0, on = 0, attack = 0, hang = 0;
            std::string od, cd;  // (strtod: "nan" and "inf" are values here)
            if (!(in >> id >> on >> od >> cd >> attack >> hang)) return 2;
            const double open_db = strtod(od.c_str(), nullptr), close_db = strtod(cd.c_str(), nullptr);
            const SquelchVerdict v = squelch_check(c.slots.data(), c.S, id, on, open_db, close_db, attack, hang);
            if (v == SQ_OK) squelch_apply(c.slots[id], on, open_db, close_db, attack, hang);
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

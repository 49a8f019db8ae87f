// Runs the noise floor's host side (phantomsdr_amd/csrc/noiseplan.h) over a script from stdin.  Plain host C++:
// tests/test_noise_host.py builds and runs it, tests/test_gpu_noise_floor.py feeds it the GPU's own spectrum bins.  The slots,
// their setters and the printed demodulation plan are those of tests/demod_plan_table.cpp, whose text is included (its main()
// under another name); behind every `batch` this program runs noise_plan() and squelch_plan() as demod.hip does and prints what
// they yield.  The script, one operation per line:
//   case NAME | size S n nframes | add I | remove I | pause I | resume I | kind I MODE FINE SIDEBAND | window I L MID R | post on|off
//   notch I INDEX FIRST END     as in demod_plan_table.cpp
//   rate R                      the context's audio_rate (a new case starts from 12000)
//   noise I ON                  psdr_client_set_noise_floor: noise_floor_check, then noise_floor_apply; prints the verdict
//   ref I REF                   psdr_client_set_squelch_reference: squelch_reference_check, then squelch_reference_apply
//   squelch I ON OPEN_DB CLOSE_DB ATTACK HANG
//                               psdr_client_set_squelch (squelchplan.h)
//   dump                        the noise-floor fields of every slot
//   batch                       demod_plan (printed as demod_plan_table.cpp prints it), then one `nf` and one `sq` line
//   select LEN K S_0 .. S_LEN-1 noise_select_host over sums given as f32 bits: the selected value's bits
//   ring N E_0 .. E_N-1         N evaluations (f32 bits) pushed into a state that starts from zero: behind each one the
//                               estimate's bits, fill and pos
//   frames LEN PERIOD NF NB LEN_1 .. LEN_NB  RE IM RE IM ...
//                               NF frames of a window of LEN bins as f32 bits, frame-major (re, im of bin 0 of frame 0 first),
//                               walked from a zero state as the NB batches of the given lengths: the W of every frame, the
//                               frames' power sums in bin order (what pwr is up to the demodulator's own order), the state behind
//   relwalk TOPEN TCLOSE ATTACK HANG N P_0 .. P_N-1 W_0 .. W_N-1
//                               the relative squelch from (closed, 0): squelch_frame_relative per frame, all values f32 bits
#define main demod_plan_table_main
#include "demod_plan_table.cpp"
#undef main

#include "noiseplan.h"
#include "squelchplan.h"

static uint32_t bits_of(float v) { return noise_bits(v); }
static float float_of(uint32_t u) { return noise_float(u); }

static int g_rate = 12000;

static void dump(const Ctx &c) {
    for (size_t i = 0; i < c.S; i++) {
        const AudioSlot &s = c.slots[i];
        printf("nfs slot=%zu active=%d on=%d b_on=%d fresh=%d nf_l=%d nf_r=%d ref=%d sq_on=%d sq_fresh=%d\n", i, (int)s.active, s.nf_on, (int)s.b_nf_on,
               (int)s.nf_fresh, s.nf_l, s.nf_r, s.sq_ref, s.sq_on, (int)s.sq_fresh);
    }
}
// behind demod_plan, as demod.hip's batch_plan calls them
static void noise_batch(Ctx &c, uint64_t seq_before) {
    if (c.seq == seq_before) {  // (a refused batch: nothing moved)
        printf("nf refused=1\n");
        return;
    }
    std::vector<NoiseEntry> table(c.S);
    const NoisePlan p = noise_plan(c.slots.data(), c.S, c.seq, table.data());
    int lo = 0, n = 0;
    noise_fetch_span(c.slots.data(), c.S, c.seq, &lo, &n);
    printf("nf n=%d lo=%d nspan=%d any=%d fetch_lo=%d fetch_n=%d zero=", p.n, p.lo, p.nspan, (int)p.any(), lo, n);
    for (size_t j = 0; j < p.zero.size(); j++) printf("%s%zu", j ? "," : "", p.zero[j]);
    printf(" list=");
    for (int j = 0; j < p.n; j++) printf("%s%d:%d:%d:%d", j ? "," : "", table[j].slot, table[j].l, table[j].r, table[j].pad);
    printf("\n");
    bool audio = false;
    for (const AudioSlot &s : c.slots) audio |= s.active && !s.paused && s.last_seq == c.seq && s.b_mode != PSDR_IQ;
    std::vector<SquelchEntry> sq(c.S);
    const SquelchPlan q = squelch_plan(c.slots.data(), c.S, c.seq, c.f.post_on && audio, sq.data());
    printf("sq nsq=%d ncopy=%d any_ref=%d list=", q.nsq, q.ncopy, (int)q.any_ref);
    for (int j = 0; j < q.nsq + q.ncopy; j++) printf("%s%d:%d", j ? "," : "", sq[j].slot, sq[j].pad);
    printf("\n");
}
static bool read_bits(std::istringstream &in, std::vector<float> &v) {
    for (float &x : v) {
        uint32_t u = 0;
        if (!(in >> u)) return false;
        x = float_of(u);
    }
    return true;
}
static void print_state(const NoiseState &st) {
    printf(" fill=%d pos=%d cnt=%d ring=", st.fill, st.pos, st.cnt);
    for (int i = 0; i < NOISE_RING; i++) printf("%s%u", i ? "," : "", bits_of(st.ring[i]));
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
            g_rate = 12000;
            printf("case name=%s\n", w.c_str());
        } else if (op == "size") {
            size_t S = 0;
            int n = 0, nframes = 0;
            if (!(in >> S >> n >> nframes) || S == 0) return 2;
            c.resize(S, n, nframes);
        } else if (op == "rate") {
            if (!(in >> g_rate)) return 2;
        } else if (op == "batch") {
            const uint64_t before = c.seq;
            batch(c);
            noise_batch(c, before);
        } else if (op == "post") {
            in >> w;
            c.f.post_on = w == "on";
        } else if (op == "dump") {
            dump(c);
        } else if (op == "noise") {
            int id = 0, on = 0;
            if (!(in >> id >> on)) return 2;
            const NoiseVerdict v = noise_floor_check(c.slots.data(), c.S, id, on, g_rate);
            if (v == NF_OK) noise_floor_apply(c.slots[id], on);
            const char *names[] = {"OK", "BAD_ID", "NO_RATE", "IN_USE"};
            printf("set id=%d verdict=%s period=%d\n", id, names[v], noise_period(g_rate > 0 ? g_rate : 1, c.f.n));
        } else if (op == "ref") {
            int id = 0, ref = 0;
            if (!(in >> id >> ref)) return 2;
            const SqRefVerdict v = squelch_reference_check(c.slots.data(), c.S, id, ref);
            if (v == SR_OK) squelch_reference_apply(c.slots[id], ref);
            const char *names[] = {"OK", "BAD_ID", "BAD_VALUE", "NOISE_OFF"};
            printf("set id=%d verdict=%s\n", id, names[v]);
        } else if (op == "squelch") {
            int id = 0, on = 0, attack = 0, hang = 0;
            double open_db = 0, close_db = 0;
            if (!(in >> id >> on >> open_db >> close_db >> attack >> hang)) return 2;
            const SquelchVerdict v = squelch_check(c.slots.data(), c.S, id, on, open_db, close_db, attack, hang);
            if (v == SQ_OK) squelch_apply(c.slots[id], on, open_db, close_db, attack, hang);
            printf("set id=%d verdict=%s\n", id, v == SQ_OK ? "OK" : "REFUSED");
        } else if (op == "select") {
            int len = 0, k = 0;
            if (!(in >> len >> k) || len < 1 || k < 0 || k >= len) return 2;
            std::vector<float> sums(len);
            if (!read_bits(in, sums)) return 2;
            printf("sel len=%d k=%d rank=%d bits=%u\n", len, k, noise_rank(len), bits_of(noise_select_host(sums.data(), len, k)));
        } else if (op == "ring") {
            int n = 0;
            if (!(in >> n) || n < 0) return 2;
            std::vector<float> e(n);
            if (!read_bits(in, e)) return 2;
            NoiseState st{};
            printf("est at=0 bits=%u", bits_of(noise_estimate(st)));
            print_state(st);
            printf("\n");
            for (int j = 0; j < n; j++) {
                noise_push(st, e[j]);
                printf("est at=%d bits=%u", j + 1, bits_of(noise_estimate(st)));
                print_state(st);
                printf("\n");
            }
        } else if (op == "frames") {
            int len = 0, period = 0, nf = 0, nb = 0;
            if (!(in >> len >> period >> nf >> nb) || period < 1 || nf < 1 || nb < 1) return 2;
            std::vector<int> lens(nb);
            int total = 0;
            for (int &b : lens) {
                if (!(in >> b) || b < 1) return 2;
                total += b;
            }
            if (total != nf) return 2;
            const int bins = len > 0 ? len : 0;
            std::vector<float> x((size_t)2 * bins * nf);
            if (!read_bits(in, x)) return 2;
            NoiseState st{};
            std::vector<float> acc(bins > 0 ? bins : 1, 0.f), W(nf);
            int f0 = 0;
            for (int b : lens) {
                noise_batch_host(st, acc.data(), len, period, b, [&](int t, int f) {
                    const float *v = &x[((size_t)(f0 + f) * bins + t) * 2];
                    return noise_bin_power(v[0], v[1]);
                }, W.data() + f0);
                f0 += b;
            }
            printf("W len=%d period=%d bits=", len, period);
            for (int f = 0; f < nf; f++) printf("%s%u", f ? "," : "", bits_of(W[f]));
            printf(" pwr=");
            for (int f = 0; f < nf; f++) {
                float p = 0.f;
                for (int t = 0; t < bins; t++) p += noise_bin_power(x[((size_t)f * bins + t) * 2], x[((size_t)f * bins + t) * 2 + 1]);
                printf("%s%u", f ? "," : "", bits_of(p));
            }
            print_state(st);
            printf(" acc=");
            for (int t = 0; t < bins; t++) printf("%s%u", t ? "," : "", bits_of(acc[t]));
            printf("\n");
        } else if (op == "relwalk") {
            uint32_t to = 0, tc = 0;
            int attack = 0, hang = 0, n = 0;
            if (!(in >> to >> tc >> attack >> hang >> n) || n < 1) return 2;
            std::vector<float> p(n), wv(n);
            if (!read_bits(in, p) || !read_bits(in, wv)) return 2;
            const SquelchEntry e{0, attack, hang, 1, float_of(to), float_of(tc)};
            SquelchState st{0, 0};
            std::string flags;
            for (int f = 0; f < n; f++) flags += squelch_frame_relative(st, p[f], wv[f], e) ? '1' : '0';
            printf("rel flags=%s open=%d cnt=%d\n", flags.c_str(), st.open, st.cnt);
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
            } else if (op == "notch") {
                int k = 0;
                if (!(in >> k) || k < 0 || k >= PSDR_NOTCH_MANUAL || !(in >> s.notch[2 * k] >> s.notch[2 * k + 1])) return 2;
            } else {
                return 2;
            }
        }
    }
    return 0;
}

// Runs the forward path's planners (phantomsdr_amd/csrc/forwardplan.h) over a script from stdin.  Plain host C++:
// tests/forward_plan_table.py builds and runs it, tests/test_forward_plan.py writes the scripts.  One operation per line:
//   seg G CUS ENV LO HI         for every batch size LO..HI one `seg` line: seg_len, seg_handoff, seg_count, a hash of the
//                               table seg_table fills, and whether the table keeps the plan's invariants (inv, below)
//   segtab G CUS ENV NF         the table itself: a `segtab` line, then `T` and five numbers per entry - frame, first tile,
//                               tiles, the segment above, carry-in through memory
//   cap G CUS ENV MAXB          seg_cap, and the largest seg_count over 1..MAXB counted here
//   tails R LEVELS LT LOG2M2 M2 REAL_FUSED MAPPED L2GPT PAIR
//                               tails_plan: kind:lvl_in:len_in:src:dst:mapped per step
//   wfreset W                   W waterfall slots as constructed, the carry's state as constructed
//   wffacts R LEVELS TILED_LT TILE_CH SKIP
//   wfslot I ACTIVE LEVEL L R DET
//   wfbatch FIRST NF            wf_plan on the carried state, which moves on as psdr_waterfall_batch moves it
//   wflayout TILED_LT LEVELS R Q_LEN Q_STRIDE QT_STRIDE
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "forwardplan.h"

using namespace psdr;

// FNV-1a over the entries' words
static uint64_t fnv(const std::vector<SegEntry> &tab) {
    uint64_t h = 1469598103934665603ull;
    for (const SegEntry &e : tab)
        for (unsigned v : {e.x, e.y, e.z, e.w}) h = (h ^ v) * 1099511628211ull;
    return h;
}

// every tile of every frame in exactly one segment; the segment above is of the same frame and ends one tile above (the top
// segment's: the one that holds tile 0); the segments without a carry-in come first; a carry-in through memory comes from
// exactly nframes entries earlier; hand-off: G/4 x 3, G/8 ... 1, 1 tiles, level-major
static bool seg_invariants(int G, int nf, const std::vector<SegEntry> &tab, bool handoff) {
    std::vector<unsigned char> seen((size_t)G * nf, 0);
    bool mem_seen = false;
    for (size_t sg = 0; sg < tab.size(); sg++) {
        const SegEntry &e = tab[sg];
        const int g0 = (int)(e.y & 0xFFFFu), ln = (int)(e.y >> 16);
        if ((int)e.x >= nf || ln < 1 || g0 >= G || g0 - ln + 1 < 0 || e.z >= tab.size()) return false;
        for (int g = g0 - ln + 1; g <= g0; g++)
            if (seen[(size_t)e.x * G + g]++) return false;
        const SegEntry &a = tab[e.z];
        const int ga = (int)(a.y & 0xFFFFu), la = (int)(a.y >> 16);
        const bool mem = (e.w & SEG_CARRY_MEM) != 0;
        if (a.x != e.x || (e.w & ~SEG_CARRY_MEM)) return false;
        if (g0 == G - 1 ? (ga - la + 1 != 0 || mem) : (ga - la + 1 != g0 + 1)) return false;
        if (mem && (sg < (size_t)nf || e.z != sg - (size_t)nf)) return false;
        if (!mem && mem_seen) return false;
        mem_seen |= mem;
    }
    for (unsigned char s : seen)
        if (s != 1) return false;
    if (!handoff) return !mem_seen;
    int levels = 2;
    for (int g = G; g > 1; g >>= 1) levels++;  // log2 G + 2
    if (tab.size() != (size_t)levels * nf) return false;
    for (int lv = 0; lv < levels; lv++) {
        const int want = lv < 3 ? G / 4 : std::max(G >> lv, 1);
        for (int f = 0; f < nf; f++) {
            const SegEntry &e = tab[(size_t)lv * nf + f];
            if ((int)e.x != f || (int)(e.y >> 16) != want || ((e.w & SEG_CARRY_MEM) != 0) != (lv > 0)) return false;
        }
    }
    return true;
}

int main() {
    std::vector<WfSlot> slots;
    std::vector<WfClient> h_wf;
    std::vector<int> h_sent;
    WfFacts wf;
    WfCarry carry;
    std::vector<SegEntry> tab;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        if (op == "seg" || op == "segtab") {
            SegFacts s;
            int lo = 0, hi = 0;
            if (!(in >> s.G >> s.num_cus >> s.seg_len_env >> lo) || s.G < 1 || lo < 1) return 2;
            hi = lo;
            if (op == "seg" && !(in >> hi)) return 2;
            for (int nf = lo; nf <= hi; nf++) {
                const unsigned n = seg_count(s, nf);
                tab.assign(n, SegEntry{~0u, ~0u, ~0u, ~0u});
                seg_table(s, nf, tab.data());
                const bool ho = seg_handoff(s, nf);
                if (op == "seg") {
                    printf("seg G=%d cus=%d env=%d nf=%d len=%d handoff=%d count=%u fnv=%016llx inv=%d\n", s.G, s.num_cus, s.seg_len_env, nf, seg_len(s, nf),
                           (int)ho, n, (unsigned long long)fnv(tab), (int)seg_invariants(s.G, nf, tab, ho));
                } else {
                    printf("segtab G=%d cus=%d env=%d nf=%d handoff=%d count=%u\nT", s.G, s.num_cus, s.seg_len_env, nf, (int)ho, n);
                    for (const SegEntry &e : tab) printf(" %u %u %u %u %u", e.x, e.y & 0xFFFFu, e.y >> 16, e.z, e.w);
                    printf("\n");
                }
            }
        } else if (op == "cap") {
            SegFacts s;
            int maxb = 0;
            if (!(in >> s.G >> s.num_cus >> s.seg_len_env >> maxb) || maxb < 1) return 2;
            unsigned brute = 0;
            for (int nf = 1; nf <= maxb; nf++) brute = std::max(brute, seg_count(s, nf));
            printf("cap G=%d cus=%d env=%d maxb=%d cap=%u brute=%u\n", s.G, s.num_cus, s.seg_len_env, maxb, seg_cap(s, maxb), brute);
        } else if (op == "tails") {
            TailFacts f;
            unsigned long long R = 0;
            int fused = 0;
            if (!(in >> R >> f.levels >> f.LT >> f.log2M2 >> f.M2 >> fused >> f.mapped >> f.l2gpt >> f.pair)) return 2;
            f.R = (size_t)R;
            f.real_fused = fused != 0;
            const TailPlan p = tails_plan(f);
            static const char *kinds[] = {"COL_64", "COL_128", "COL_256", "COL_256_PAIRED", "GENERIC"};
            printf("tails R=%llu levels=%d LT=%d n=%d steps=", R, f.levels, f.LT, p.n);
            for (int i = 0; i < p.n; i++)
                printf("%s%s:%d:%zu:%d:%d:%d", i ? "," : "", kinds[p.step[i].kind], p.step[i].lvl_in, p.step[i].len_in, p.step[i].src, p.step[i].dst,
                       (int)p.step[i].mapped);
            printf("\n");
        } else if (op == "wfreset") {
            int W = 0;
            if (!(in >> W) || W < 1) return 2;
            slots.assign((size_t)W, WfSlot());
            h_wf.assign((size_t)W, WfClient());
            carry = WfCarry();
        } else if (op == "wffacts") {
            unsigned long long R = 0;
            if (!(in >> R >> wf.levels >> wf.tiled_lt >> wf.tile_ch >> wf.skip_num) || wf.skip_num < 1) return 2;
            wf.R = (size_t)R;
        } else if (op == "wfslot") {
            int i = 0, active = 0;
            if (!(in >> i) || i < 0 || i >= (int)slots.size()) return 2;
            WfSlot &s = slots[(size_t)i];
            if (!(in >> active >> s.level >> s.l >> s.r >> s.det)) return 2;
            s.active = active != 0;
        } else if (op == "wfbatch") {
            unsigned long long first = 0;
            int nf = 0;
            if (!(in >> first >> nf) || nf < 1 || slots.empty()) return 2;
            h_sent.assign((size_t)nf, -1);
            const WfPlan p = wf_plan(slots.data(), slots.size(), wf, carry, first, nf, h_wf.data(), h_sent.data());
            carry = p.after;
            printf("wf first=%llu nf=%d nsent=%d total=%zu maxid=%d gather=%d hold=%d any_sample=%d carry_in=%d f0=%d accumulate=%d run=%d next=%llu carry_n=%d sent=", first,
                   nf, p.nsent, p.total, p.maxid, (int)p.gather, (int)p.hold, (int)p.any_sample, p.carry_n, p.f0, p.accumulate, (int)carry.run,
                   (unsigned long long)carry.next, carry.carry_n);
            for (int i = 0; i < p.nsent; i++) printf("%s%d", i ? "," : "", h_sent[(size_t)i]);
            printf(" clients=");
            for (size_t i = 0; i < slots.size(); i++)
                printf("%s%d:%d:%d:%d:%zu:%zu:%d:%d", i ? "," : "", h_wf[i].active, h_wf[i].level, h_wf[i].l, h_wf[i].r, h_wf[i].qoff, h_wf[i].out_off, h_wf[i].det,
                       h_wf[i].vec);
            printf(" slots=");
            for (size_t i = 0; i < slots.size(); i++)
                printf("%s%zu:%d:%d:%d:%d:%d", i ? "," : "", slots[i].out_off, slots[i].nsent, slots[i].b_level, slots[i].b_l, slots[i].b_r, slots[i].b_det);
            printf("\n");
        } else if (op == "wflayout") {
            int tiled_lt = 0, levels = 0;
            unsigned long long R = 0, q_len = 0, q_stride = 0, qt_stride = 0;
            if (!(in >> tiled_lt >> levels >> R >> q_len >> q_stride >> qt_stride)) return 2;
            const WfCarryLayout l = wf_carry_layout(tiled_lt, levels, (size_t)R, (size_t)q_len, (size_t)q_stride, (size_t)qt_stride);
            printf("wflayout ok=%d lenA=%zu qB0=%zu lenB=%zu\n", (int)l.ok, l.lenA, l.qB0, l.lenB);
        } else {
            return 2;
        }
    }
    return 0;
}

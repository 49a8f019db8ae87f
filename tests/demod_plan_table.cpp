// Runs the demodulation batch's planner (phantomsdr_amd/csrc/demodplan.h demod_plan) over a script of slot operations and
// batches from stdin and prints, per batch, the slots before, the plan, the ring slot's lists and the slots after, one line
// of key=value pairs each.  Plain host C++: tests/test_demod_plan.py builds and runs it.  The script, one operation per line:
//   case NAME                   a new context: S = 8, n = 360, nframes = 5, post chain off, no detector state, no band
//   size S n nframes            ... of another shape (the slots start over)
//   add I | remove I | pause I | resume I
//   kind I MODE FINE SIDEBAND   psdr_client_set_fine_tune, _set_sam_sideband, _set_audio_demodulation
//   window I L MID R            psdr_client_set_audio_range
//   notch I INDEX FIRST END     a manual notch's interval
//   auto I 0|1                  psdr_client_set_auto_notch (the first one allocates the detector's state: tab on)
//   post on|off | tab on|off | band none | band FIRST COUNT
//   batch
//   seeded SEED BATCHES         BATCHES batches with random operations between them, from an LCG
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "demodplan.h"

using namespace psdr;

struct Ctx {
    size_t S = 8;
    std::vector<AudioSlot> slots = std::vector<AudioSlot>(8);
    DemodFacts f;
    uint64_t seq = 0, births = 0;
    unsigned char *ring = nullptr;
    Ctx() { resize(8, 360, 5); }
    ~Ctx() { free(ring); }
    void resize(size_t S_, int n, int nframes) {
        S = S_;
        slots.assign(S, AudioSlot());
        f = DemodFacts();
        f.n = n, f.nframes = nframes;
        seq = births = 0;
        free(ring);
        ring = (unsigned char *)malloc(client_ring_bytes(S));
        if (!ring) abort();
    }
};

static void print_slots(const Ctx &c, const char *tag) {
    for (size_t i = 0; i < c.S; i++) {
        const AudioSlot &s = c.slots[i];
        printf("%s slot=%zu active=%d paused=%d l=%d r=%d mid=%.17g mode=%d cur=%d agc=%d seq=%" PRIu64 " b_l=%d b_r=%d b_mid=%.17g b_mode=%d born=%" PRIu64
               " fine=%d phi=%u b_tuned=%d sb=%d b_sb=%d notch=%d,%d,%d,%d b_notch=%d,%d,%d,%d auto=%d b_auto=%d fresh=%d\n",
               tag, i, (int)s.active, (int)s.paused, s.l, s.r, s.mid, s.mode, s.state_cur, s.agc_reset, s.last_seq, s.b_l, s.b_r, s.b_mid, s.b_mode, s.born,
               s.fine, s.ft_phi, (int)s.b_tuned, s.sam_sb, s.b_sam_sb, s.notch[0], s.notch[1], s.notch[2], s.notch[3], s.b_notch[0], s.b_notch[1],
               s.b_notch[2], s.b_notch[3], s.auto_notch, (int)s.b_auto, (int)s.auto_fresh);
    }
}
static void print_params(const char *tag, int k, const ClientParams &q) {
    printf("%s k=%d l=%d r=%d m=%d mode=%d slot=%d cur=%d agc=%d paused=%d", tag, k, q.l, q.r, q.m_floor, q.mode, q.slot, q.state_cur, q.agc_reset, q.paused);
}
static void print_zero(const char *name, const std::vector<size_t> &v) {
    printf(" %s=", name);
    for (size_t j = 0; j < v.size(); j++) printf("%s%zu", j ? "," : "", v[j]);
}

static void batch(Ctx &c) {
    printf("batch seq=%" PRIu64 " S=%zu n=%d nframes=%d post=%d tab=%d band=%d,%u,%u\n", c.seq, c.S, c.f.n, c.f.nframes, (int)c.f.post_on,
           (int)c.f.have_notch_tab, (int)c.f.has_band, c.f.band_first, c.f.band_count);
    print_slots(c, "pre");
    memset(c.ring, 0xCD, client_ring_bytes(c.S));  // (what the planner does not write is not printed)
    const DemodPlan p = demod_plan(c.slots.data(), c.S, c.seq, c.f, c.ring);
    printf("plan verdict=%s bad=%d,%d,%d seq=%" PRIu64 " nold=%d nsam=%d ntssb=%d ntiq=%d nsb=%d niq=%d nact=%d npaused=%d ndet=%d iq_off=%d any_manual=%d "
           "iq_notched=%d idle=%d ring_bytes=%zu\n",
           p.verdict == DP_OK ? "OK" : "BAND_OUTSIDE", p.bad_slot, p.bad_l, p.bad_r, c.seq, p.nold, p.nsam, p.ntssb, p.ntiq, p.nsb, p.niq, p.nact, p.npaused,
           p.ndet, p.iq_off, (int)p.any_manual, (int)p.iq_notched, (int)p.idle(), client_ring_bytes(c.S));
    if (p.verdict == DP_OK) {
        printf("off plain=%zu,%zu sam=%zu,%zu iq=%zu,%zu tssb=%zu,%zu tiq=%zu,%zu sb=%zu,%zu det=%zu,%zu slot_ci=%zu notch=%zu\n", p.plain.clients, p.plain.side,
               p.sam.clients, p.sam.side, p.iq.clients, p.iq.side, p.tssb.clients, p.tssb.side, p.tiq.clients, p.tiq.side, p.sb.clients, p.sb.side,
               p.det.clients, p.det.side, p.slot_ci, p.notch);
        printf("copies n=%d list=", p.ncopies);
        for (int j = 0; j < p.ncopies; j++) printf("%s%zu:%zu", j ? "," : "", p.copies[j].off, p.copies[j].bytes);
        printf("\nzero");
        print_zero("car", p.car_zero), print_zero("ft", p.ft_zero), print_zero("sb", p.sb_zero), print_zero("det", p.det_zero);
        printf("\n");
        const ClientParams *cl = (const ClientParams *)c.ring;
        const int listed = p.niq > 0 ? p.iq_off + p.niq : p.nact + p.npaused;
        for (int k = 0; k < listed; k++) print_params("cl", k, cl[k]), printf("\n");
        if (c.f.post_on) {
            const int *ci = (const int *)(c.ring + p.slot_ci);
            printf("ci list=");
            for (size_t i = 0; i < c.S; i++) printf("%s%d", i ? "," : "", ci[i]);
            printf("\n");
        }
        const ClientParams *ftc = (const ClientParams *)(c.ring + p.tssb.clients);
        const FtClient *ftp = (const FtClient *)(c.ring + p.tssb.side);
        for (int k = 0; k < p.ntssb + p.ntiq; k++) print_params("ft", k, ftc[k]), printf(" phi0=%u step=%u wl=%d wr=%d\n", ftp[k].phi0, ftp[k].step, ftp[k].l, ftp[k].r);
        const ClientParams *sbc = (const ClientParams *)(c.ring + p.sb.clients);
        const SbClient *sbp = (const SbClient *)(c.ring + p.sb.side);
        for (int k = 0; k < p.nsb; k++) print_params("sbl", k, sbc[k]), printf(" wl=%d wr=%d side=%d pad=%d\n", sbp[k].l, sbp[k].r, sbp[k].side, sbp[k].pad);
        if (p.any_manual) {
            const int *nt = (const int *)(c.ring + p.notch);
            for (size_t i = 0; i < c.S; i++) printf("nt slot=%zu v=%d,%d,%d,%d\n", i, nt[4 * i], nt[4 * i + 1], nt[4 * i + 2], nt[4 * i + 3]);
        }
        const ClientParams *det = (const ClientParams *)(c.ring + p.det.clients);
        for (int k = 0; k < p.ndet; k++) print_params("det", k, det[k]), printf("\n");
    }
    print_slots(c, "post");
}

// the setters of demod.hip, as far as they touch a slot
static void op_add(Ctx &c, size_t i) {
    c.slots[i] = AudioSlot();
    c.slots[i].active = true;
    c.slots[i].born = ++c.births;
}
static void op_kind(Ctx &c, size_t i, int mode, int fine, int sb) {
    AudioSlot &s = c.slots[i];
    s.fine = fine ? 1 : 0;
    s.sam_sb = sb;
    s.mode = mode;
    if (s.agc_reset == 0) s.agc_reset = 1;
}
static void op_auto(Ctx &c, size_t i, int on) {
    AudioSlot &s = c.slots[i];
    if (on) c.f.have_notch_tab = true;
    if (on && !s.auto_notch) s.auto_fresh = true;
    s.auto_notch = on ? 1 : 0;
}

static void seeded(Ctx &c, uint32_t seed, int batches) {
    uint32_t x = seed;
    auto rnd = [&](uint32_t m) {
        x = x * 1664525u + 1013904223u;
        return (x >> 8) % m;
    };
    for (int b = 0; b < batches; b++) {
        const int nops = (int)rnd(5);
        for (int o = 0; o < nops; o++) {
            const size_t i = rnd((uint32_t)c.S);
            AudioSlot &s = c.slots[i];
            const uint32_t what = rnd(16);
            if (!s.active) {
                if (what < 12) op_add(c, i), op_kind(c, i, (int)rnd(6), (int)rnd(2), (int)rnd(3));
                continue;
            }
            if (what < 4) {
                op_kind(c, i, (int)rnd(6), (int)rnd(2), (int)rnd(3));
            } else if (what < 8) {
                s.l = (int)rnd(100);
                s.r = s.l + (int)rnd(41);
                s.mid = s.l + (int)rnd(41) - 10 + rnd(1000) / 1000.0;
            } else if (what < 10) {
                s.paused = !s.paused;
            } else if (what == 10) {
                s.active = false;
            } else if (what == 11) {
                const int k = (int)rnd(2), first = (int)rnd(40);
                s.notch[2 * k] = first, s.notch[2 * k + 1] = first + (int)rnd(4);
            } else if (what == 12) {
                op_auto(c, i, (int)rnd(2));
            } else if (what == 13) {
                c.f.post_on = !c.f.post_on;
            } else if (what == 14) {
                c.f.has_band = rnd(2) != 0;
                c.f.band_first = rnd(8), c.f.band_count = 100 + rnd(40);  // (windows end at 139 at the most)
            }
        }
        batch(c);
    }
}

int main() {
    Ctx c;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, w;
        if (!(in >> op)) continue;
        size_t i = 0;
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
            batch(c);
        } else if (op == "seeded") {
            uint32_t seed = 0;
            int batches = 0;
            if (!(in >> seed >> batches)) return 2;
            seeded(c, seed, batches);
        } else if (op == "post" || op == "tab") {
            in >> w;
            (op == "post" ? c.f.post_on : c.f.have_notch_tab) = w == "on";
        } else if (op == "band") {
            in >> w;
            c.f.has_band = w != "none";
            if (c.f.has_band) {
                c.f.band_first = (uint32_t)strtoul(w.c_str(), nullptr, 0);
                if (!(in >> c.f.band_count)) return 2;
            }
        } else {
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
            } else if (op == "auto") {
                int on = 0;
                if (!(in >> on)) return 2;
                op_auto(c, i, on);
            } else {
                return 2;
            }
        }
    }
    return 0;
}

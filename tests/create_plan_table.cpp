// Runs the create-time planners (phantomsdr_amd/csrc/createplan.h) over a script from stdin.  Plain host C++:
// tests/create_plan_table.py builds and runs it, tests/test_create_plan.py writes the scripts.  One operation per line:
//   env SPLIT 3PASS SEGLEN LOG2M2 CUS
//                               the run-time knobs as facts (CreateEnv) for the configs that follow
//   cfg FFT REAL LEVELS BRIGHT ADD AUDIO RATE FMT BATCH CLIENTS WFCLIENTS SKIP WFSIZE
//                               create_check: a `check` line; an accepted config: the `idft` line of its audio size and, if that
//                               is accepted too, `shape`, `recmap`, `lay`, `seg`, `tail`, `buffers` and `twiddles`
//   band NB HALO                band_plan on the last accepted config's shape and its CURRENT layout: a `band` line; an accepted
//                               call makes its layout the current one, as psdr_set_band_layout does
//   perm STRIDE                 the shape's record map and the current layout: is pos() inside its buffer for every index, and
//                               one-to-one on every STRIDE-th (1: checked whole).  A banded layout: inside means in one of the
//                               nbands regions, less than a frame's stride from its start
//   idft N TAB                  idft_plan alone; TAB = 1: the stage table behind it, `S` and i j e1 per entry, stage-major
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "createplan.h"

using namespace psdr;

static void print_idft(const IdftPlan &p, bool with_table, bool dump) {
    static const char *kinds[] = {"none", "fixed360", "fixed720", "wave", "lds"};
    unsigned long long h = 1469598103934665603ull;  // FNV-1a over the entries' words
    std::vector<IdftEntry> tab;
    if (with_table && !p.st.code) {
        tab.resize((size_t)p.nstages * p.n);
        idft_stage_table(p, tab.data());
        for (const IdftEntry &e : tab)
            for (int v : {e.i, e.j, e.e1, e.pad}) h = (h ^ (unsigned)v) * 1099511628211ull;
    }
    printf("idft n=%d code=%d kind=%s nstages=%d radix=", p.n, p.st.code, kinds[p.kind], p.nstages);
    for (int i = 0; i < p.nstages; i++) printf("%s%d", i ? "," : "", p.radix[i]);
    printf(" lds_mode=%d idft_lds=%zu threads=%d tabfnv=%016llx msg=%s\n", p.lds_mode, p.idft_lds, p.idft_threads, with_table ? h : 0ull, p.st.msg.c_str());
    if (dump) {
        printf("S");
        for (const IdftEntry &e : tab) printf(" %d %d %d", e.i, e.j, e.e1);
        printf("\n");
    }
}
static void print_lay(const SpecLayout &l) {
    printf("lay mode=%d m1=%d l2m1=%d L=%d l2L=%d k0=%d l2Lb=%d Lw=%d c2_0=%d band_stride=%zu l2cp=%d\n", l.mode, l.m1, l.l2m1, l.L, l.l2L, l.k0, l.l2Lb, l.Lw,
           l.c2_0, l.band_stride, l.l2cp);
}
static void print_buf(const char *name, const Buf &b) { printf(" %s=%zu:%d", name, b.count, (int)(b.count && b.zero)); }
static void print_tw(const char *name, const Twiddles &t) {
    if (t.count)
        printf(" %s=%zu:%zu:%zu:%d", name, t.count, t.mult, t.period, t.sign);
    else
        printf(" %s=none", name);
}
// pos(i) < size for every i < count; distinct on every stride-th i
template <class Pos>
static void perm(const char *name, size_t count, size_t size, size_t stride, Pos pos) {
    std::vector<unsigned char> seen(size, 0);
    bool inside = true, distinct = true;
    for (size_t i = 0; i < count; i++) {
        const size_t p = pos(i);
        if (p >= size)
            inside = false;
        else if (i % stride == 0 && seen[p]++)
            distinct = false;
    }
    printf("perm what=%s count=%zu size=%zu stride=%zu inside=%d distinct=%d\n", name, count, size, stride, (int)inside, (int)distinct);
}

int main() {
    CreateEnv env;
    ShapePlan s;
    SpecLayout lay{};
    size_t spec_size = 0, band_frame = 0;  // bins of one frame's spectrum; banded: of all regions' first frames, and of one of them
    bool have = false;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        if (op == "env") {
            int split = 0, three = 0;
            env = CreateEnv();
            if (!(in >> split >> three >> env.seg_len >> env.log2M2 >> env.num_cus)) return 2;
            env.real_split_2048x1024 = split != 0, env.real_3pass = three != 0;
        } else if (op == "cfg") {
            psdr_config g{};
            g.struct_size = sizeof g;
            if (!(in >> g.fft_size >> g.is_real >> g.downsample_levels >> g.brightness_offset >> g.additional_size >> g.audio_fft_size >> g.audio_rate >>
                  g.input_format >> g.max_batch >> g.max_clients >> g.max_waterfall_clients >> g.skip_num >> g.waterfall_size))
                return 2;
            const PlanStatus st = create_check(g);
            printf("check code=%d msg=%s\n", st.code, st.msg.c_str());
            have = false;
            if (st.code) continue;
            const IdftPlan d = idft_plan(g.audio_fft_size);
            print_idft(d, g.audio_fft_size <= (1 << 20), false);
            if (d.st.code) continue;
            s = shape_plan(g, env);
            lay = s.lay, spec_size = s.spec_stride, band_frame = 0, have = true;
            printf("shape N=%zu M=%zu R=%zu real=%d l2M1=%d l2M2=%d M1=%d M2=%d T1=%d T2=%d size_log2=%d levels=%d maxb=%d n=%d spec_stride=%zu q_len=%zu "
                   "q_stride=%zu qt_stride=%zu p_stride=%zu fused=%d tile_ch=%d LT=%d tiled_lt=%d mwf=%d skip=%d l2UB=%d\n",
                   s.N, s.M, s.R, (int)s.is_real, s.log2M1, s.log2M2, s.M1, s.M2, s.T1, s.T2, s.size_log2, s.levels, s.max_batch, s.n, s.spec_stride, s.q_len,
                   s.q_stride, s.qt_stride, s.p_stride, (int)s.real_fused, s.tile_ch, s.LT, s.tiled_lt, s.min_waterfall_fft, s.skip_num, s.log2UB);
            printf("recmap l2tpr=%d l2gpt=%d l2rows=%d pair=%d mapped=%d\n", s.recmap.l2tpr, s.recmap.l2gpt, s.recmap.l2rows, s.recmap.pair, s.recmap.mapped);
            print_lay(s.lay);
            printf("seg G=%d cus=%d env=%d\n", s.seg.G, s.seg.num_cus, s.seg.seg_len_env);
            const TailFacts &t = s.tail;
            printf("tail R=%zu levels=%d LT=%d l2M2=%d M2=%d fused=%d mapped=%d l2gpt=%d pair=%d\n", t.R, t.levels, t.LT, t.log2M2, t.M2, (int)t.real_fused, t.mapped,
                   t.l2gpt, t.pair);
            const BufferPlan b = buffer_plan(s, g);
            printf("buffers seg_cap=%zu slots=%zu client_ring=%zu wslots=%zu wf_sent_off=%zu wf_ring=%zu", b.seg_cap, b.slots, b.client_ring, b.wslots, b.wf_sent_off,
                   b.wf_ring);
            print_buf("tickets", b.tickets), print_buf("Y", b.Y), print_buf("Z", b.Z), print_buf("seamP", b.seamP), print_buf("seamC", b.seamC);
            print_buf("segflag", b.segflag), print_buf("spec", b.spec), print_buf("q", b.q), print_buf("qt", b.qt), print_buf("pscr", b.pscr);
            print_buf("stage", b.stage), print_buf("h_out", b.h_out), print_buf("h_q", b.h_q), print_buf("ypost", b.ypost), print_buf("pwr", b.pwr);
            print_buf("audio", b.audio), print_buf("nan", b.nan), print_buf("real_prev", b.real_prev), print_buf("bb_tail", b.bb_tail);
            print_buf("bb_last", b.bb_last), print_buf("ssb_mark", b.ssb_mark), print_buf("gscratch", b.gscratch);
            printf("\n");
            const TwiddlePlan w = twiddle_plan(s);
            printf("twiddles");
            print_tw("Wl1", w.Wl1), print_tw("Wl2", w.Wl2), print_tw("TB", w.TB), print_tw("UA", w.UA), print_tw("UB", w.UB), print_tw("UG", w.UG), print_tw("Wn", w.Wn);
            printf("\n");
        } else if (op == "band") {
            int nb = 0;
            unsigned halo = 0;
            if (!(in >> nb >> halo) || !have) return 2;
            BandPlan b = band_plan(s, lay, nb, halo, s.max_batch);
            if (b.st.code) b.H = b.Lb = b.Lw = 0;  // (a rejected call has no geometry to show)
            printf("band nbands=%d halo=%u code=%d H=%d Lb=%d Lw=%d frame_stride=%zu region=%zu msg=%s\n", nb, halo, b.st.code, b.H, b.Lb, b.Lw, b.frame_stride, b.region,
                   b.st.msg.c_str());
            if (b.st.code) continue;
            print_lay(b.lay);
            lay = b.lay, spec_size = (size_t)nb * b.frame_stride, band_frame = b.frame_stride;
        } else if (op == "perm") {
            size_t stride = 0;
            if (!(in >> stride) || stride < 1 || !have) return 2;
            if (s.tiled_lt >= 0) perm("records", s.R / (size_t)s.tile_ch, s.R / (size_t)s.tile_ch, stride, [&](size_t g) { return s.recmap.pos(g); });
            perm("bins", s.R, spec_size, stride, [&](size_t k) {
                const size_t p = lay.pos((int)k);
                if (lay.mode != 3) return p;
                const size_t region = p / lay.band_stride, in_region = p % lay.band_stride;  // the regions' first frames, packed
                return in_region < band_frame ? region * band_frame + in_region : spec_size;
            });
        } else if (op == "idft") {
            int n = 0, tab = 0;
            if (!(in >> n >> tab)) return 2;
            print_idft(idft_plan(n), tab != 0, tab != 0);
        } else {
            return 2;
        }
    }
    return 0;
}

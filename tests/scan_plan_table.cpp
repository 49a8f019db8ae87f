// scan_plan_table.cpp - the band scan's host side (phantomsdr_amd/csrc/scanplan.h) as a program: built by tests/scan_model.py with
// the host compiler and driven over stdin, one command per line.  The steps it runs are the text the kernels of scan.hip run.
//   trace <in> <out>   in: int32 n, nframes, fresh, a; uint16 s[n]; int8 q[nframes][n]      out: uint16 s[n]
//   eval <in> <out>    in: int32 n, threshold, gap, min_width, cap; uint16 s[n]
//                      out: uint32 Q[G], F[G]; uint32 total, kept; psdr_signal list[kept]; int32 passed; psdr_signal out[min(passed, cap)]
//   check R levels level avg_shift threshold gap      -> verdict=<n> text=<...>
//   set                                               -> the run state as psdr_scan_set leaves it
//   step first nframes                                -> fresh=<0|1> next=<n> last=<n> evaluated=<0|1>
//   launch R levels tiled_lt tile_ch level            -> the launch plan's fields
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "scanplan.h"

using namespace psdr;

static std::vector<unsigned char> slurp(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) {
        fprintf(stderr, "cannot read %s\n", path.c_str());
        exit(2);
    }
    std::vector<unsigned char> b;
    unsigned char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + k);
    fclose(f);
    return b;
}
template <typename T>
static void put(FILE *f, const T *p, size_t count) {
    if (count && fwrite(p, sizeof(T), count, f) != count) {
        fprintf(stderr, "short write\n");
        exit(2);
    }
}

int main() {
    ScanState st;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "trace") {
            std::string src, dst;
            in >> src >> dst;
            const std::vector<unsigned char> b = slurp(src);
            const int32_t *h = (const int32_t *)b.data();
            const size_t n = (size_t)h[0];
            const int nframes = h[1], fresh = h[2], a = h[3];
            std::vector<uint16_t> s((const uint16_t *)(b.data() + 16), (const uint16_t *)(b.data() + 16) + n);
            std::vector<const int8_t *> fr((size_t)nframes);
            for (int f = 0; f < nframes; f++) fr[(size_t)f] = (const int8_t *)(b.data() + 16 + 2 * n + (size_t)f * n);
            scan_trace_host(s.data(), n, fr.data(), nframes, fresh != 0, a);
            FILE *o = fopen(dst.c_str(), "wb");
            put(o, s.data(), n);
            fclose(o);
            printf("trace n=%zu\n", n);
        } else if (cmd == "eval") {
            std::string src, dst;
            in >> src >> dst;
            const std::vector<unsigned char> b = slurp(src);
            const int32_t *h = (const int32_t *)b.data();
            const size_t n = (size_t)h[0];
            const int threshold = h[1], gap = h[2], min_width = h[3], cap = h[4];
            const uint16_t *s = (const uint16_t *)(b.data() + 20);
            const ScanEval e = scan_evaluate_host(s, n, threshold, gap);
            const uint32_t kept = (uint32_t)e.list.size();
            std::vector<psdr_signal> all(kept), some((size_t)cap);
            for (uint32_t i = 0; i < kept; i++) all[i] = scan_record(e.list[i], e.F.data());
            const int32_t passed = scan_filter(e.list.data(), (int)kept, e.F.data(), min_width, some.data(), cap);
            FILE *o = fopen(dst.c_str(), "wb");
            put(o, e.Q.data(), e.Q.size());
            put(o, e.F.data(), e.F.size());
            put(o, &e.total, 1);
            put(o, &kept, 1);
            put(o, all.data(), all.size());
            put(o, &passed, 1);
            put(o, some.data(), (size_t)(passed < cap ? passed : cap));
            fclose(o);
            printf("eval total=%u kept=%u passed=%d\n", e.total, kept, passed);
        } else if (cmd == "check") {
            size_t R;
            int levels;
            psdr_scan_config c;
            in >> R >> levels >> c.level >> c.avg_shift >> c.threshold >> c.gap;
            const ScanVerdict v = scan_check(R, levels, c);
            printf("check verdict=%d text=%s\n", (int)v, scan_text(v, R, levels, c).c_str());
        } else if (cmd == "set") {
            st = ScanState();
            printf("set run=%d evaluated=%d\n", st.run ? 1 : 0, st.evaluated ? 1 : 0);
        } else if (cmd == "step") {
            unsigned long long first;
            int nframes;
            in >> first >> nframes;
            const ScanStep p = scan_step_plan(st, first, nframes);
            st = p.after;
            printf("step fresh=%d next=%llu last=%llu evaluated=%d\n", p.fresh ? 1 : 0, (unsigned long long)st.next, (unsigned long long)st.last_frame,
                   st.evaluated ? 1 : 0);
        } else if (cmd == "launch") {
            ScanFacts f;
            int level;
            in >> f.R >> f.levels >> f.tiled_lt >> f.tile_ch >> level;
            const ScanLaunch l = scan_launch(f, level);
            printf("launch n=%zu G=%d words=%zu tiled=%d per=%d loff=%d qoff=%zu trace_blocks=%u floor_blocks=%u hot_blocks=%u emit_blocks=%u bytes=%zu\n", l.n,
                   l.G, l.words, l.tiled ? 1 : 0, l.per, l.loff, l.qoff, l.trace_blocks, l.floor_blocks, l.hot_blocks, l.emit_blocks, scan_bytes(f.R));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
        fflush(stdout);
    }
    return 0;
}

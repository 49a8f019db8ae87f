// Prints the post chain's plan (phantomsdr_amd/csrc/postplan.h) for every case on stdin, one line of key=value pairs each.
// A case: audio_rate n max_batch slots piped opt_agc opt_pcm16 opt_streams [KNOB=value ...], the knobs by the last word of
// their PSDR_PC_* names.  Plain host C++: tests/test_post_plan.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "postplan.h"

using namespace psdr;

int main() {
    static const char *const ma_names[] = {"MA2_CMW", "MA2", "MAD", "MA_POW2", "MA_DIV"};
    static const char *const agc_names[] = {"AGC_ONE_KERNEL", "AGC_FIVE"};
    static const char *const verdicts[] = {"OK", "RATE_TOO_SMALL", "RATE_UNSUPPORTED", "NO_FRAME"};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        PcFacts f;
        PcKnobs k;
        int piped = 0;
        if (!(in >> f.audio_rate >> f.n >> f.max_batch >> f.slots >> piped >> f.opt_pc_agc >> f.opt_pc_pcm16 >> f.opt_pc_streams)) continue;
        f.piped = piped != 0;
        std::string w;
        while (in >> w) {
            const size_t eq = w.find('=');
            if (eq == std::string::npos) return 2;
            const std::string name = w.substr(0, eq);
            const int v = (int)strtol(w.c_str() + eq + 1, nullptr, 0);
            int *dst = name == "LANES" ? &k.lanes : name == "RESERVE" ? &k.reserve : name == "OWN" ? &k.own : name == "FUSED" ? &k.fused
                     : name == "CMW" ? &k.cmw : name == "DIRECT" ? &k.direct : name == "STREAMS" ? &k.streams
                     : name == "SPLIT_PEAK" ? &k.split_peak : name == "PICK" ? &k.pick : name == "SKIP" ? &k.skip : nullptr;
            if (!dst) return 2;
            *dst = v;
        }
        const PcPlan p = pc_resolve(f, k);
        printf("verdict=%s D=%d L=%d h=%d vo=%d px=%zu pv=%zu nsub=%d sb=%d nch=%d h_magic=%u nblk=%zu agc_ok=%d groups=%u lanes=%d rgroups=%u "
               "reserve=%d own=%d rows4=%d ma=%s agc=%s ma_fused=%d direct=%d att_faster=%d pcm16=%d ma_lds=%zu gain_lds=%zu s_ma=%d s_gain=%d "
               "s_peak=%d split_peak=%d pick_streams=%d skip=%d\n",
               verdicts[p.verdict], p.D, p.L, p.h, p.vo, p.px, p.pv, p.nsub, p.sb, p.nch, p.h_magic, p.verdict == PC_OK ? pc_nblk(p.L, p.Tm) : (size_t)0,
               (int)p.agc_ok, p.groups, p.lanes, p.rgroups, p.reserve, (int)p.own, (int)p.rows4, ma_names[p.ma], agc_names[p.agc], (int)p.ma_fused,
               (int)p.direct, (int)p.att_faster, (int)p.pcm16, p.ma_lds, p.gain_lds, p.s_ma, p.s_gain, p.s_peak, (int)p.split_peak,
               (int)p.pick_streams, p.skip);
    }
    return 0;
}

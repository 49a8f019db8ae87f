// Runs the multi-GPU group's planner (phantomsdr_amd/csrc/groupplan.h) over a script from stdin.  Plain host C++:
// tests/group_plan_table.py builds and runs it, tests/test_group_plan.py writes the scripts.  One operation per line:
//   facts N SHARD FORCE PEER SERIAL TWICE R IS_REAL LAY_MODE MAX_BATCH HALF_FRAME_BYTES SPEC_STRIDE AUDIO_FFT_SIZE
//                        the facts of every line below (SHARD without the flag bits; TWICE: a device listed twice, -1 none)
//   check                group_check: code, which rule, what the message names
//   layout [STRIDE]      group_layout, and a fresh group state.  STRIDE: the regions a banded root would report (band b from
//                        b R/n on, STRIDE bins, frames STRIDE bins apart); without it a banded layout has no bands
//   place L NEXT_RR      group_rank_for
//   step FROM_RING F     group_step_plan on the layout and the state as the steps before left it: the set, link_bytes, which
//                        events time the exchange, the state afterwards (cur_set:copies_pending:xpending0:xpending1) and the
//                        operations in order, `;` between them, `/COMMIT` behind one that commits state:
//                        WAIT(stream,event) RECORD(event,stream) RING_WAIT(stream,halves) GROUP_START GROUP_END
//                        BCAST_RAW(rank,stream,bytes) BCAST_SPEC(rank,stream,floats) SEND_BAND(band,stream,floats)
//                        RECV_BAND(rank,stream,floats) PULL(rank,stream,bytes) PACK(band) TRANSFORM(rank) DEMOD_*(rank) WATERFALL(rank)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "groupplan.h"

using namespace psdr;

static std::string stream_of(const GroupOp &o) { return o.xs ? "XS" : "ST" + std::to_string(o.rank); }
static std::string event_of(const GroupOp &o) {
    static const char *names[] = {"EV_NONE", "EV0", "EV1", "EV_X", "EV_RANK", "EV_T0", "EV_T1", "EV_XDONE", "EV_PULL"};
    std::string s = names[o.ev];
    if (o.ev == EV_XDONE || o.ev == EV_PULL) s += "[" + std::to_string(o.ev_set) + "]";
    if (o.ev == EV_RANK || o.ev == EV_T0 || o.ev == EV_T1 || o.ev == EV_PULL) s += "[" + std::to_string(o.ev_rank) + "]";
    return s;
}
static std::string text_of(const GroupOp &o) {
    static const char *names[] = {"WAIT", "RECORD", "RING_WAIT", "GROUP_START", "GROUP_END", "BCAST_RAW", "BCAST_SPEC", "SEND_BAND", "RECV_BAND", "PULL", "PACK",
                                  "TRANSFORM", "DEMOD_OWN", "DEMOD_FROM_SPEC", "DEMOD_FROM_BAND", "DEMOD_FROM_BAND_REGION", "WATERFALL"};
    const std::string k = names[o.kind], r = std::to_string(o.rank), arg = std::to_string(o.arg);
    switch (o.kind) {
    case OP_WAIT: return k + "(" + stream_of(o) + "," + event_of(o) + ")";
    case OP_RECORD: return k + "(" + event_of(o) + "," + stream_of(o) + ")";
    case OP_RING_WAIT: return k + "(" + stream_of(o) + "," + arg + ")";
    case OP_GROUP_START:
    case OP_GROUP_END: return k;
    case OP_SEND_BAND: return k + "(" + std::to_string(o.band) + "," + stream_of(o) + "," + arg + ")";
    case OP_BCAST_RAW:
    case OP_BCAST_SPEC:
    case OP_RECV_BAND:
    case OP_PULL: return k + "(" + r + "," + stream_of(o) + "," + arg + ")";
    case OP_PACK: return k + "(" + std::to_string(o.band) + ")";
    default: return k + "(" + r + ")";
    }
}

int main() {
    GroupFacts f;
    GroupLayout L;
    GroupState st;
    bool have_facts = false, have_layout = false;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        if (op == "facts") {
            int force = 0, peer = 0, serial = 0, is_real = 0;
            unsigned long long R = 0, mb = 0, hb = 0, ss = 0;
            f = GroupFacts();
            if (!(in >> f.n >> f.shard >> force >> peer >> serial >> f.twice >> R >> is_real >> f.lay_mode >> mb >> hb >> ss >> f.audio_fft_size)) return 2;
            f.force_comm = force != 0, f.peer_copy = peer != 0, f.serial = serial != 0, f.is_real = is_real != 0;
            f.R = (size_t)R, f.max_batch = (size_t)mb, f.half_frame_bytes = (size_t)hb, f.spec_stride = (size_t)ss;
            have_facts = true, have_layout = false;
        } else if (op == "check") {
            if (!have_facts) return 2;
            const GroupCheck c = group_check(f);
            printf("check code=%d what=%d arg=%d\n", c.code, (int)c.what, c.arg);
        } else if (op == "layout") {
            if (!have_facts || group_check(f).code != PSDR_OK) return 2;  // (the layout of refused arguments is nobody's)
            unsigned long long stride = 0;
            GroupBands own;
            const bool regions = (bool)(in >> stride);
            for (int b = 0; b < f.n && regions; b++) own.first[b] = (uint32_t)((size_t)b * (f.R / (size_t)f.n)), own.bins[b] = (uint32_t)stride;
            own.stride = (size_t)stride;
            L = group_layout(f, regions ? &own : nullptr);
            st = GroupState();
            have_layout = true;
            printf("layout comm_on=%d peer_copy=%d self_loop=%d banded=%d overlap=%d halo=%u stride=%zu rbuf=", (int)L.comm_on, (int)L.peer_copy, (int)L.self_loop,
                   (int)L.banded, (int)L.overlap, L.halo, L.band.stride);
            for (int r = 0; r < f.n; r++) printf("%s%zu", r ? "," : "", L.rbuf_bytes[r]);
            printf(" sbuf=");
            for (int r = 0; r < f.n; r++) printf("%d", (int)L.sbuf[r]);
            printf(" first=");
            for (int r = 0; r < f.n; r++) printf("%s%u", r ? "," : "", L.band.first[r]);
            printf(" bins=");
            for (int r = 0; r < f.n; r++) printf("%s%u", r ? "," : "", L.band.bins[r]);
            printf("\n");
        } else if (op == "place") {
            int l = 0, rr = 0;
            if (!have_facts || !(in >> l >> rr) || f.n < 1 || f.R < (size_t)f.n) return 2;
            printf("place rank=%d\n", group_rank_for(f, l, rr));
        } else if (op == "step") {
            int from_ring = 0, F = 0;
            if (!have_layout || !(in >> from_ring >> F) || F < 1 || (size_t)F > L.max_batch) return 2;
            const GroupStepPlan p = group_step_plan(L, st, from_ring != 0, F);
            if (p.n >= GROUP_OPS_MAX) return 3;  // the list is full: an operation may be missing
            printf("step n=%d set=%d link_bytes=%zu stats=%d after=%d:%d:%d:%d ops=", p.n, p.set, p.link_bytes, (int)p.stats, p.after.cur_set,
                   (int)p.after.copies_pending, (int)p.after.xpending[0], (int)p.after.xpending[1]);
            for (int i = 0; i < p.n; i++) {
                printf("%s%s", i ? ";" : "", text_of(p.op[i]).c_str());
                if (p.op[i].commit) printf("/%u", p.op[i].commit);
            }
            printf("\n");
            st = p.after;
        } else {
            return 2;
        }
    }
    return 0;
}

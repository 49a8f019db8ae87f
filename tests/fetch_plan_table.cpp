// Runs the served end's planner (phantomsdr_amd/csrc/fetchplan.h) over a script from stdin.  Plain host C++:
// tests/fetch_plan_table.py builds and runs it, tests/test_fetch_plan.py writes the scripts.  One operation per line:
//   slots S                         S audio slots as constructed
//   slot I ACTIVE IN_BATCH MODE SQ  one of them at the time of the fetch
//   wfslots W                       W waterfall slots as constructed
//   wfslot I ACTIVE NSENT OUT_OFF L R
//   plan WHAT MB F H PCM16          a `plan` line: the three spans (lo:n), wf_bytes, iq_bytes, what the set records, which slots read
//                                   their squelch flags from the span (winsq), and the operations in order - copy:BUFFER:SOURCE
//                                   OFFSET:plain:BYTES:STREAM or copy:...:pitched:PITCH:WIDTH:ROWS:STREAM, record:EVENT:STREAM
//   oldest FILL INFLIGHT            the oldest set in flight
//   ring                            the ring as constructed
//   begin                           what psdr_fetch_begin does to it: the set it fills, whether it gave a fetch up
//   end                             ... psdr_fetch_end: the set and the number (from 1) of the fetch it delivers, or `none`
//   member WIN_SEQ WIN_BORN SET_SEQ BORN MODE WANT_IQ
//   row ID LO N MB FRAME            the row of [slot][max_batch], whether the span lo:n holds the slot, and its row there
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fetchplan.h"

using namespace psdr;

int main() {
    std::vector<FetchSlot> slots;
    std::vector<WfSlot> wslots;
    int fill = 0, inflight = 0, cur = -1, begun = 0;
    bool busy[PSDR_FETCH_SETS] = {};
    int holds[PSDR_FETCH_SETS] = {};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        if (op == "slots") {
            int S = 0;
            if (!(in >> S) || S < 1) return 2;
            slots.assign((size_t)S, FetchSlot());
        } else if (op == "slot") {
            int i = 0, active = 0, in_batch = 0, sq = 0;
            if (!(in >> i) || i < 0 || i >= (int)slots.size()) return 2;
            FetchSlot &s = slots[(size_t)i];
            if (!(in >> active >> in_batch >> s.mode >> sq)) return 2;
            s.active = active != 0, s.in_batch = in_batch != 0, s.sq_on = sq != 0;
        } else if (op == "wfslots") {
            int W = 0;
            if (!(in >> W) || W < 1) return 2;
            wslots.assign((size_t)W, WfSlot());
        } else if (op == "wfslot") {
            int i = 0, active = 0;
            unsigned long long off = 0;
            if (!(in >> i) || i < 0 || i >= (int)wslots.size()) return 2;
            WfSlot &w = wslots[(size_t)i];
            if (!(in >> active >> w.nsent >> off >> w.b_l >> w.b_r)) return 2;
            w.active = active != 0, w.out_off = (size_t)off;
        } else if (op == "plan") {
            FetchFacts f;
            unsigned long long mb = 0, F = 0, h = 0;
            int pcm16 = 0;
            if (!(in >> f.what >> mb >> F >> h >> pcm16) || slots.empty() || F < 1 || F > mb) return 2;
            f.S = slots.size(), f.mb = (size_t)mb, f.F = (size_t)F, f.h = (size_t)h, f.pcm16 = pcm16 != 0;
            const FetchPlan p = fetch_plan(f, slots.data(), wslots.data(), wslots.size());
            printf("plan what=%u S=%zu mb=%zu F=%zu h=%zu pcm16=%d iq=%d:%d car=%d:%d sq=%d:%d wf_bytes=%zu iq_bytes=%zu frames=%d seq=%d has_pcm=%d winsq=", f.what, f.S,
                   f.mb, f.F, f.h, pcm16, p.span[SPAN_IQ].lo, p.span[SPAN_IQ].n, p.span[SPAN_CAR].lo, p.span[SPAN_CAR].n, p.span[SPAN_SQ].lo, p.span[SPAN_SQ].n,
                   p.wf_bytes, p.iq_bytes, p.frames, (int)p.carries_seq, (int)p.has_pcm);
            for (const FetchSlot &s : slots) printf("%d", (int)fetch_in_span(f.what, s, SPAN_SQ));
            printf(" ops=");
            static const char *bufs[] = {"wf", "pwr", "nan", "audio", "iq", "car", "sq", "pcm"};
            static const char *evs[] = {"", "ev_wf", "ev_audio", "ev_pcm"};
            const char *sep = "";
            for (int i = 0; i <= p.n; i++) {
                if (i == p.n0) printf("%srecord:done:0", sep), sep = ",";
                if (i == p.n) break;
                const FetchCopy &k = p.copy[i];
                if (k.pitched)
                    printf("%scopy:%s:%zu:pitched:%zu:%zu:%zu:%d", sep, bufs[k.buf], k.src_off, k.pitch, k.width, k.rows, k.stream);
                else
                    printf("%scopy:%s:%zu:plain:%zu:%d", sep, bufs[k.buf], k.src_off, k.rows * k.pitch, k.stream);
                sep = ",";
                if (k.after != FE_NONE) printf(",record:%s:%d", evs[k.after], k.stream);
            }
            printf("\n");
        } else if (op == "oldest") {
            int fl = 0, nf = 0;
            if (!(in >> fl >> nf) || fl < 0 || fl >= PSDR_FETCH_SETS || nf < 0 || nf > PSDR_FETCH_SETS) return 2;
            printf("oldest fill=%d inflight=%d set=%d\n", fl, nf, ring_oldest(fl, nf));
        } else if (op == "ring") {
            fill = inflight = begun = 0, cur = -1;
            for (int k = 0; k < PSDR_FETCH_SETS; k++) busy[k] = false, holds[k] = 0;
        } else if (op == "begin") {
            const int k = fill;
            const bool gave_up = busy[k];
            if (busy[k]) busy[k] = false, inflight--;
            cur = ring_cur_after_begin(cur, fill);
            busy[k] = true, holds[k] = ++begun;
            fill = ring_next(fill), inflight++;
            printf("begin set=%d gave_up=%d cur=%d fill=%d inflight=%d\n", k, (int)gave_up, cur, fill, inflight);
        } else if (op == "end") {
            if (inflight <= 0) {
                printf("end none cur=%d fill=%d inflight=%d\n", cur, fill, inflight);
                continue;
            }
            const int k = ring_oldest(fill, inflight);
            if (!busy[k]) return 3;  // the ring is out of step
            busy[k] = false, inflight--, cur = k;
            printf("end set=%d fetch=%d cur=%d fill=%d inflight=%d\n", k, holds[k], cur, fill, inflight);
        } else if (op == "member") {
            FetchWin w;
            unsigned long long wseq = 0, wborn = 0, seq = 0, born = 0;
            int want_iq = 0;
            if (!(in >> wseq >> wborn >> seq >> born >> w.mode >> want_iq)) return 2;
            w.last_seq = wseq, w.born = wborn;
            printf("member part=%d kind=%d\n", (int)fetched_member(w, seq, born), (int)iq_kind_matches(w.mode, want_iq != 0));
        } else if (op == "row") {
            FetchSpan s;
            int id = 0, frame = 0;
            unsigned long long mb = 0;
            if (!(in >> id >> s.lo >> s.n >> mb >> frame)) return 2;
            printf("row id=%d frame=%d row=%zu held=%d", id, frame, fetch_row(id, (size_t)mb, frame), (int)s.holds(id));
            if (s.holds(id)) printf(" span_row=%zu", span_row(s, id, (size_t)mb, frame));
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}

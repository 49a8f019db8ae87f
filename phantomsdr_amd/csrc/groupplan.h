// groupplan.h - what a multi-GPU group (group.hip) decides on the host, resolved in pure functions of a few facts: whether its
// create arguments are acceptable, which transport it uses and what each rank gets for buffers, which rank serves a client, and -
// per step - the ordered list of operations: who waits for, records and copies what on which stream, who takes part in a
// collective and which demodulation entry each rank calls, with the state the step leaves behind.  Plain host C++17 (no HIP):
// group.hip validates, allocates and walks the list, tests/test_group_plan.py prints it and checks its ordering for n up to 16.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/psdr.h"

namespace psdr {

constexpr int GROUP_RANKS_MAX = 16;

// ---- facts: the create arguments, and what the root context says ---------------------------------------------------------------
struct GroupFacts {
    int n = 0, shard = 0;  // ranks; PSDR_SHARD_CLIENTS / _RAW / _BAND (the flag bits taken off)
    bool force_comm = false, peer_copy = false, serial = false;
    int twice = -1;        // a device that is listed twice, -1: none (group_listed_twice)
    size_t R = 0;          // bins of the spectrum
    bool is_real = false;
    int lay_mode = 0;      // SpecLayout::mode of the root
    size_t max_batch = 0, half_frame_bytes = 0, spec_stride = 0;
    int audio_fft_size = 0;
};
inline GroupFacts group_flags(int ndevices, int shard) {
    GroupFacts f;
    f.n = ndevices;
    f.force_comm = (shard & PSDR_SHARD_FORCE_COMM) != 0, f.peer_copy = (shard & PSDR_SHARD_PEER_COPY) != 0, f.serial = (shard & PSDR_SHARD_SERIAL) != 0;
    f.shard = shard & ~(PSDR_SHARD_FORCE_COMM | PSDR_SHARD_PEER_COPY | PSDR_SHARD_SERIAL);
    return f;
}
// (a list of a length group_check refuses is not read)
inline int group_listed_twice(const int *devices, int n) {
    for (int i = 0; i < n && n <= GROUP_RANKS_MAX; i++)
        for (int j = 0; j < i; j++)
            if (devices[i] == devices[j]) return devices[i];
    return -1;
}

// ---- the argument rules of psdr_group_create, in the order they are answered -------------------------------------------------------
enum GroupError { GROUP_OK, GROUP_BAD_COUNT, GROUP_BAD_SHARD, GROUP_EXCLUSIVE, GROUP_TWICE, GROUP_BAND_POW2 };
struct GroupCheck {
    int code = PSDR_OK;
    GroupError what = GROUP_OK;
    int arg = 0;  // what the message names: the count, the sharding or the device
};
inline GroupCheck group_check(const GroupFacts &f) {
    if (f.n < 1 || f.n > GROUP_RANKS_MAX) return {PSDR_ERR_INVALID, GROUP_BAD_COUNT, f.n};
    if (f.shard < PSDR_SHARD_CLIENTS || f.shard > PSDR_SHARD_BAND) return {PSDR_ERR_INVALID, GROUP_BAD_SHARD, f.shard};
    if (f.force_comm && f.peer_copy) return {PSDR_ERR_INVALID, GROUP_EXCLUSIVE, 0};
    if (!f.peer_copy && f.twice >= 0) return {PSDR_ERR_INVALID, GROUP_TWICE, f.twice};  // RCCL wants one rank per device
    if (f.shard == PSDR_SHARD_BAND && (f.n & (f.n - 1))) return {PSDR_ERR_INVALID, GROUP_BAND_POW2, f.n};
    return {};
}

// ---- layout: what psdr_group_create derives -------------------------------------------------------------------------------------------
// the bands of a band-sharded group: bins [first[b], first[b] + bins[b]) for rank b, frames `stride` bins apart
struct GroupBands {
    uint32_t first[GROUP_RANKS_MAX] = {0}, bins[GROUP_RANKS_MAX] = {0};
    size_t stride = 0;
};
struct GroupLayout {
    int n = 0, shard = 0;
    bool comm_on = false;    // RCCL collectives are issued (n > 1, or PSDR_SHARD_FORCE_COMM)
    bool peer_copy = false;  // the peers pull with device copies instead
    bool self_loop = false;  // one device with the collectives forced: rank 0 is its own peer (band: band 0 - the whole spectrum - is
                             // packed, sent to and received from oneself and demodulated from the received buffer)
    bool banded = false;     // band sharding: the root's second pass writes the band regions itself (no pack)
    bool overlap = false;    // the exchange of batch b beside the root's transform of batch b + 1, the root's result sets alternating
    uint32_t halo = 0;       // a window is at most audio_fft_size bins wide (src/signal.cpp:309-311)
    GroupBands band;
    size_t rbuf_bytes[GROUP_RANKS_MAX] = {0};  // per rank: its receive buffer (raw halves / band), 0: none
    bool sbuf[GROUP_RANKS_MAX] = {false};      // packed bands: the root's send buffer of band b exists
    size_t max_batch = 0, half_frame_bytes = 0, spec_stride = 0;
};
inline bool group_banded(const GroupFacts &f) { return f.shard == PSDR_SHARD_BAND && !f.is_real && f.lay_mode == 1 && f.n > 1; }
// `own`: the regions of a banded root (psdr_band_region: the context is their owner); packed bands are laid out here - linear
// buffers filled by psdr_pack_band, [b R/n, (b+1) R/n + 1 + halo), the same count on every rank
inline GroupLayout group_layout(const GroupFacts &f, const GroupBands *own = nullptr) {
    GroupLayout L;
    L.n = f.n, L.shard = f.shard;
    L.peer_copy = f.peer_copy && f.n > 1;
    L.comm_on = !f.peer_copy && (f.n > 1 || f.force_comm);
    L.self_loop = L.comm_on && f.n == 1;
    L.banded = group_banded(f);
    L.overlap = !f.serial && (L.comm_on || L.peer_copy) && (f.shard == PSDR_SHARD_CLIENTS || L.banded);
    L.max_batch = f.max_batch, L.half_frame_bytes = f.half_frame_bytes, L.spec_stride = f.spec_stride;
    size_t rbytes = 0;
    if (f.shard == PSDR_SHARD_RAW) rbytes = (f.max_batch + 1) * f.half_frame_bytes;
    if (f.shard == PSDR_SHARD_BAND) {
        L.halo = (uint32_t)std::max(f.audio_fft_size, 0);
        if (L.banded) {
            if (own) L.band = *own;
        } else {
            const size_t per = (f.R + (size_t)f.n - 1) / (size_t)f.n;
            L.band.stride = std::min(per + 1 + L.halo, f.R);
            for (int b = 0; b < f.n; b++) {
                L.band.first[b] = (uint32_t)((size_t)b * (f.R / (size_t)f.n)), L.band.bins[b] = (uint32_t)L.band.stride;
                L.sbuf[b] = b > 0 || L.self_loop;
            }
        }
        rbytes = f.max_batch * L.band.stride * 2 * sizeof(float);
    }
    // (the root receives only its own band on the self-loop; its raw broadcast is in place)
    for (int r = f.shard == PSDR_SHARD_BAND && L.self_loop ? 0 : 1; r < f.n; r++) L.rbuf_bytes[r] = rbytes;
    return L;
}

// ---- placement: the one rule of add and retune ----------------------------------------------------------------------------------
// band sharding: the band the window STARTS in (it may end in the halo); otherwise round robin (client i on rank i mod n, like
// assign_clients of distributed.py)
inline int band_of(size_t R, int n, int l) {
    const int b = (int)((size_t)std::max(l, 0) / (R / (size_t)n));
    return std::min(b, n - 1);
}
inline int group_rank_for(const GroupFacts &f, int l, int next_rr) { return f.shard == PSDR_SHARD_BAND ? band_of(f.R, f.n, l) : next_rr % f.n; }

// ---- one step ---------------------------------------------------------------------------------------------------------------------------
enum GroupOpKind {
    OP_WAIT, OP_RECORD,  // the stream waits for / records the event
    OP_RING_WAIT,        // raw from the ring: the written-events of the `arg` half-frames that are sent
    OP_GROUP_START, OP_GROUP_END,
    OP_BCAST_RAW, OP_BCAST_SPEC,  // the rank's side of a broadcast from rank 0: `arg` bytes / floats
    OP_SEND_BAND, OP_RECV_BAND,   // the root sends band `band`; rank `band` receives it: `arg` floats
    OP_PULL,                      // the rank copies `arg` bytes of its share from the root
    OP_PACK,                      // the root packs band `band` into its send buffer
    OP_TRANSFORM,                 // rank 0: the caller's halves or the ring; others: their receive buffer (raw sharding)
    OP_DEMOD_OWN, OP_DEMOD_FROM_SPEC, OP_DEMOD_FROM_BAND, OP_DEMOD_FROM_BAND_REGION,
    OP_WATERFALL
};
enum GroupEvent { EV_NONE, EV0, EV1, EV_X, EV_RANK, EV_T0, EV_T1, EV_XDONE, EV_PULL };  // EV_RANK, EV_T0, EV_T1: [r]; EV_XDONE: [s]; EV_PULL: [s][r]
// what a successfully issued operation commits to the group's state (a failed step leaves what was issued before it)
enum : unsigned { GC_COPIES_CLEAR = 1, GC_COPIES_SET = 2, GC_X_CLEAR = 4, GC_X_SET = 8, GC_TIMED = 16 };
struct GroupOp {
    GroupOpKind kind = OP_WAIT;
    int rank = 0;     // whose device, stream, context and communicator
    bool xs = false;  // on the root's exchange stream instead of the rank's own
    GroupEvent ev = EV_NONE;
    int ev_set = 0, ev_rank = 0;
    int band = 0;
    size_t arg = 0;
    unsigned commit = 0;
};
struct GroupState {
    int cur_set = 0;              // the root's result set BEFORE its transform of the step (the context's; it toggles under overlap)
    bool copies_pending = false;  // peer copy: EV_RANK[r] of the last step not yet waited for by the root
    bool xpending[2] = {false, false};  // overlap: the exchange of that set is in flight
};
enum GroupStats { STATS_NONE, STATS_EV01, STATS_T01 };  // psdr_group_link_stats: EV0 -> EV1 on the root, or the slowest peer's EV_T0 -> EV_T1
// (the longest list: 16 ranks, raw from the ring by peer copies - 15 + 1 + 76 + 15 + 16 + 16 + 1 operations)
constexpr int GROUP_OPS_MAX = 160;
struct GroupStepPlan {
    int n = 0;
    GroupOp op[GROUP_OPS_MAX];
    int set = 0;            // overlap: the result set this step's transform writes and its exchange reads
    size_t link_bytes = 0;  // bytes over ONE root -> peer link, once the exchange is issued (GC_TIMED)
    GroupStats stats = STATS_NONE;
    GroupState after;
    GroupOp &add(GroupOpKind kind, int rank, size_t arg = 0) {
        GroupOp &o = op[std::min(n, GROUP_OPS_MAX - 1)];
        n = std::min(n + 1, GROUP_OPS_MAX);
        o = GroupOp();
        o.kind = kind, o.rank = rank, o.arg = arg;
        return o;
    }
    GroupOp &sync(GroupOpKind kind, int rank, bool xs, GroupEvent ev, int ev_set = 0, int ev_rank = 0) {
        GroupOp &o = add(kind, rank);
        o.xs = xs, o.ev = ev, o.ev_set = ev_set, o.ev_rank = ev_rank;
        return o;
    }
};
inline void group_commit(GroupState &s, unsigned commit, int set) {
    if (commit & (GC_COPIES_CLEAR | GC_COPIES_SET)) s.copies_pending = (commit & GC_COPIES_SET) != 0;
    if (commit & (GC_X_CLEAR | GC_X_SET)) s.xpending[set] = (commit & GC_X_SET) != 0;
}
// the pull: peer r copies `bytes` of its share from the root on ITS OWN stream, behind the root's "data ready" event - n - 1
// independent copies, one per root -> peer link; `closing` is what the root waits for before it overwrites the source
inline void group_pull(GroupStepPlan &p, const GroupLayout &L, size_t bytes, GroupEvent closing, unsigned commit) {
    p.sync(OP_RECORD, 0, false, EV_X);
    for (int r = 1; r < L.n; r++) {
        p.sync(OP_WAIT, r, false, EV_X);
        p.sync(OP_RECORD, r, false, EV_T0, 0, r);
        p.add(OP_PULL, r, bytes);
        p.sync(OP_RECORD, r, false, EV_T1, 0, r);
        p.sync(OP_RECORD, r, false, closing, p.set, r).commit = r == L.n - 1 ? commit | GC_TIMED : 0u;
    }
}
// the bracket around the RCCL calls: serial on the root's stream; overlapped the root's side goes to the exchange stream, behind
// the transform (its own stream goes on with the demodulation and the next batch's transform into the other result set)
inline void group_bracket_begin(GroupStepPlan &p, const GroupLayout &L) {
    if (L.overlap) {
        p.sync(OP_RECORD, 0, false, EV_X);
        p.sync(OP_WAIT, 0, true, EV_X);
    }
    p.sync(OP_RECORD, 0, L.overlap, EV0);
    p.add(OP_GROUP_START, 0);
}
inline void group_bracket_end(GroupStepPlan &p, const GroupLayout &L) {
    p.add(OP_GROUP_END, 0);
    GroupOp &e1 = p.sync(OP_RECORD, 0, L.overlap, EV1);
    if (L.overlap)
        p.sync(OP_RECORD, 0, true, EV_XDONE, p.set).commit = GC_X_SET | GC_TIMED;
    else
        e1.commit = GC_TIMED;
}
inline void root_waits_for_ranks(GroupStepPlan &p, const GroupLayout &L) {
    for (int r = 1; r < L.n; r++) p.sync(OP_WAIT, 0, false, EV_RANK, 0, r).commit = r == L.n - 1 ? (unsigned)GC_COPIES_CLEAR : 0u;
}
inline GroupStepPlan group_step_plan(const GroupLayout &L, const GroupState &s, bool from_ring, int nframes) {
    GroupStepPlan p;
    const size_t F = (size_t)nframes;
    const bool exchange = L.comm_on || L.peer_copy;
    p.set = L.overlap ? s.cur_set ^ 1 : s.cur_set;
    p.stats = L.peer_copy ? STATS_T01 : L.comm_on ? STATS_EV01 : STATS_NONE;
    // what the root is about to overwrite was the source of an exchange: of this result set two steps ago (overlap), or of the
    // peers' copies of the previous step
    if (L.overlap && s.xpending[p.set]) {
        if (L.comm_on) p.sync(OP_WAIT, 0, false, EV_XDONE, p.set).commit = GC_X_CLEAR;
        for (int r = 1; r < L.n && L.peer_copy; r++) p.sync(OP_WAIT, 0, false, EV_PULL, p.set, r).commit = r == L.n - 1 ? (unsigned)GC_X_CLEAR : 0u;
    } else if (!L.overlap && s.copies_pending) {
        root_waits_for_ranks(p, L);
    }
    if (L.shard == PSDR_SHARD_RAW) {
        // the raw half-frames cross the links, every rank transforms them itself.  They are the caller's (or the ring's, whose slots
        // the root's first pass releases): the root's transform - and what the caller orders behind it - comes after the pulls
        const size_t bytes = (F + 1) * L.half_frame_bytes;
        if (from_ring) p.add(OP_RING_WAIT, 0, F + 1);
        if (L.comm_on) {
            group_bracket_begin(p, L);
            for (int r = 0; r < L.n; r++) p.add(OP_BCAST_RAW, r, bytes);  // (root: in place)
            group_bracket_end(p, L);
        } else if (L.peer_copy) {
            group_pull(p, L, bytes, EV_RANK, GC_COPIES_SET);
            root_waits_for_ranks(p, L);
        }
        if (exchange) p.link_bytes = bytes;
        for (int r = 0; r < L.n; r++) p.add(OP_TRANSFORM, r);
        for (int r = 0; r < L.n; r++) p.add(OP_DEMOD_OWN, r);
    } else {
        const bool band = L.shard == PSDR_SHARD_BAND;
        const size_t count = F * (band ? L.band.stride : L.spec_stride) * 2;  // floats: frames one stride apart
        p.add(OP_TRANSFORM, 0);
        for (int b = 1; b < L.n && band && !L.banded; b++) p.add(OP_PACK, 0).band = b;
        if (band && L.self_loop) p.add(OP_PACK, 0).band = 0;
        if (L.comm_on) {
            group_bracket_begin(p, L);
            for (int r = 0; r < L.n && !band; r++) p.add(OP_BCAST_SPEC, r, count).xs = r == 0 && L.overlap;
            for (int b = L.self_loop ? 0 : 1; b < L.n && band; b++) {
                GroupOp &snd = p.add(OP_SEND_BAND, 0, count);
                snd.band = b, snd.xs = L.overlap;
                p.add(OP_RECV_BAND, b, count).band = b;
            }
            group_bracket_end(p, L);
        } else if (L.peer_copy) {
            group_pull(p, L, count * sizeof(float), L.overlap ? EV_PULL : EV_RANK, L.overlap ? GC_X_SET : GC_COPIES_SET);
        }
        if (exchange) p.link_bytes = count * sizeof(float);
        // the root's own clients read its spectrum (self-loop: the band buffer that came back)
        p.add(band && L.self_loop ? OP_DEMOD_FROM_BAND : OP_DEMOD_OWN, 0);
        for (int r = 1; r < L.n; r++) p.add(!band ? OP_DEMOD_FROM_SPEC : L.banded ? OP_DEMOD_FROM_BAND_REGION : OP_DEMOD_FROM_BAND, r).band = r;
    }
    p.add(OP_WATERFALL, 0);  // waterfall clients stay on the root (they read only its pyramid)
    p.after = s;
    for (int i = 0; i < p.n; i++) group_commit(p.after, p.op[i].commit, p.set);
    p.after.cur_set = p.set;
    return p;
}

}  // namespace psdr

// group.hip - SURVEY 8e from C: ONE process drives n GPUs of a node.  GPU 0 ("root") owns the raw ring, the forward
// FFT and the waterfall clients; the audio clients are spread over all n contexts; one exchange per batch over xGMI,
// issued DIRECTLY through RCCL (librccl.so is dlopen()ed when a group of more than one device is created - a single-GPU
// user of libpsdr_hip.so never loads it):
//   PSDR_SHARD_CLIENTS  ncclBroadcast of the spectrum, F x 8 (N + A) bytes per batch (BASELINE.json configs[3]: the
//                       north star's shape; link-bound at ~9.5 GS/s by construction)
//   PSDR_SHARD_RAW      ncclBroadcast of the raw half-frames (4 x fewer bytes for cs16), every GPU runs the forward FFT
//   PSDR_SHARD_BAND     GPU b gets only band b of the spectrum (+ a halo of one maximal window): ncclSend / ncclRecv of
//                       R/n + halo bins per frame.  2^20- and 2^21-point IQ contexts: the root's second pass writes the
//                       band regions itself (psdr_set_band_layout) and the regions ARE the send buffers; otherwise
//                       psdr_pack_band fills them.
// | PSDR_SHARD_PEER_COPY: no RCCL - the peers pull their share from the root with hipMemcpyPeerAsync on their own
//                       streams (one copy per root->peer link, ordered by events).  A device may then be listed more than
//                       once (n ranks on fewer GPUs): the whole multi-rank logic - placement, band regions and halos,
//                       migration, fetch - runs on a one-GPU box, only the transport differs.
// What is DECIDED - the argument rules, transport and buffers per rank, a client's rank, and the ordered operations of a step
// with their streams and events - is groupplan.h (host-only, tests/test_group_plan.py).  This file carries it out: it creates
// what the layout names, walks a step's list (group_issue: one place per HIP / RCCL call) and keeps the client table.
// Everything of one rank - its kernels and its side of the collective - is enqueued in order on ONE stream per device
// (psdr_set_stream), so a step needs no host synchronisation; psdr_group_synchronize() drains all devices.
// Threads: client calls arrive on the server's websocket threads while the frame loop steps the group.  A client is named
// by a STABLE gid (an index into the group's table of (rank, slot)); every psdr_group_* call that touches the table, a
// stream or a client takes the group mutex, so a band migration can never interleave with a step's enqueue.
// The Python twin for one PROCESS per GPU (torch.distributed, what bench.py --gpus N runs) is phantomsdr_amd/distributed.py.
#include <dlfcn.h>

#include "ctx.h"
#include "groupplan.h"

namespace {

// the slice of RCCL's C API used here (rccl.h: ncclCommInitAll :236, ncclBroadcast :591, ncclSend :700, ncclRecv :722)
typedef void *ncclComm_t;
enum { ncclSuccess = 0 };
enum { ncclChar = 0, ncclFloat = 7 };
struct Rccl {
    void *h = nullptr;
    int (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Broadcast)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*Send)(const void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    int load() {
        if (h) return PSDR_OK;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"}) {
            h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (h) break;
        }
        if (!h) return fail(PSDR_ERR_UNSUPPORTED, "librccl.so could not be loaded (%s): a multi-GPU group needs RCCL", dlerror());
#define SYM(f)                                                                       \
    *(void **)(&f) = dlsym(h, "nccl" #f);                                            \
    if (!f) return fail(PSDR_ERR_UNSUPPORTED, "librccl.so does not export nccl" #f)
        SYM(CommInitAll);
        SYM(CommDestroy);
        SYM(GroupStart);
        SYM(GroupEnd);
        SYM(Broadcast);
        SYM(Send);
        SYM(Recv);
        SYM(GetErrorString);
#undef SYM
        return PSDR_OK;
    }
};
Rccl g_rccl;

#define NCCLCHK(expr)                                                                                          \
    do {                                                                                                       \
        int e_ = (expr);                                                                                       \
        if (e_ != ncclSuccess) return fail(PSDR_ERR_HIP, "%s failed: %s", #expr, g_rccl.GetErrorString(e_));  \
    } while (0)

// fails with `rc` and the message as it stands now: the clean-up in between must not overwrite it
template <typename Cleanup>
int fail_after(int rc, Cleanup cleanup) {
    const std::string msg = psdr_last_error();
    cleanup();
    return fail(rc, "%s", msg.c_str());
}
// `count` elements on `device`; `what`: the message, which names the bytes and may name the device
template <typename T>
int alloc_on(int device, DevBuf<T> &b, size_t count, const char *what) {
    if (hipSetDevice(device) == hipSuccess && !b.alloc(count)) return PSDR_OK;
    return fail(PSDR_ERR_NOMEM, what, count * sizeof(T), device);
}

}  // namespace

struct GroupClient {
    int rank = -1, id = -1;  // device rank and the slot of that rank's context; rank < 0: free entry
};
struct psdr_group {
    GroupFacts facts;               // the create arguments and the root's shape
    GroupLayout lay;                // transport, buffers per rank, bands (groupplan.h)
    int n = 0;
    std::mutex mtx;                 // the client table, next_rr, and every enqueue on the ranks' streams
    std::vector<GroupClient> clients;  // gid -> (rank, slot): the gid a caller holds never changes
    std::vector<Event> ev_rank;        // per rank, on its device: migration hand-over / peer copy done
    std::vector<Event> ev_t0, ev_t1;   // peer copy: the copy's own duration on the peer's stream
    Event ev_x;                        // the root's data of this step is ready (peer copy; overlapped exchange)
    // copies_pending, and - the exchange of batch b beside the root's transform of batch b + 1 (lay.overlap) - xpending: the
    // root alternates its two result sets (psdr_ctx::alt_sets) and issues ITS side of the collective on a stream of its own
    // (`xs`), behind ev_x; what it waits for - before it overwrites a set two steps later - is that set's exchange
    // (ev_xdone[set]; peer copies: ev_pull[set][r], recorded by the peers).  PSDR_SHARD_SERIAL switches it off (A/B, tests).
    GroupState state;
    Stream xs;
    Event ev_xdone[2];
    std::vector<Event> ev_pull[2];
    std::vector<int> dev;
    std::vector<psdr_ctx *> ctx;
    std::vector<Stream> st;         // the one stream per device everything of that rank is ordered on
    std::vector<ncclComm_t> comm;
    std::vector<DevBuf<unsigned char>> rbuf;  // per rank: receive buffer (raw halves / band region), nullptr where unused
    std::vector<DevBuf<cf>> sbuf;   // band sharding with the pack pass: the root's send buffers, one per band
    int next_rr = 0;                // round-robin cursor of psdr_group_client_add
    // link accounting
    double link_bytes = 0;          // bytes that crossed ONE link (root -> one peer) in the last step
    Event ev0, ev1;
    GroupStats stats = STATS_NONE;  // which events timed the last step's exchange
    uint64_t steps = 0;
};

// (callers hold g->mtx)
static int gid_split(psdr_group *g, int gid, int *rank, int *id) {
    if (gid < 0 || gid >= (int)g->clients.size() || g->clients[gid].rank < 0) return fail(PSDR_ERR_INVALID, "no client %d in this group", gid);
    *rank = g->clients[gid].rank;
    *id = g->clients[gid].id;
    return PSDR_OK;
}
static int gid_new(psdr_group *g, int rank, int id) {
    for (size_t i = 0; i < g->clients.size(); i++)
        if (g->clients[i].rank < 0) {
            g->clients[i] = GroupClient{rank, id};
            return (int)i;
        }
    g->clients.push_back(GroupClient{rank, id});
    return (int)g->clients.size() - 1;
}
// rank `to` copies on its own stream what rank `from` holds: inside one device, or across two
static hipError_t rank_copy(psdr_group *g, int to, void *d, int from, const void *s, size_t bytes) {
    return g->dev[from] == g->dev[to] ? hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, g->st[to])
                                      : hipMemcpyPeerAsync(d, g->dev[to], s, g->dev[from], bytes, g->st[to]);
}

extern "C" void psdr_group_destroy(psdr_group *g) {
    if (!g) return;
    for (int r = 0; r < (int)g->ctx.size(); r++) {
        if (r < (int)g->dev.size()) hipSetDevice(g->dev[r]);
        if (g->ctx[r]) {
            psdr_synchronize(g->ctx[r]);
            psdr_set_stream(g->ctx[r], nullptr);
        }
        if (r < (int)g->comm.size() && g->comm[r]) g_rccl.CommDestroy(g->comm[r]);
        if (g->ctx[r]) psdr_destroy(g->ctx[r]);
        if (r < (int)g->st.size()) g->st[r].reset();  // (behind the context that was ordered on it)
    }
    delete g;  // (the buffers, the events and the exchange stream go with their members)
}

extern "C" int psdr_group_create(const psdr_config *cfg, const int *devices, int ndevices, int shard, psdr_group **out) {
    if (!cfg || !devices || !out) return fail(PSDR_ERR_INVALID, "null argument");
    GroupFacts f = group_flags(ndevices, shard);
    f.twice = group_listed_twice(devices, ndevices);
    const GroupCheck chk = group_check(f);
    switch (chk.what) {
    case GROUP_BAD_COUNT: return fail(chk.code, "a group has 1..16 devices, not %d", chk.arg);
    case GROUP_BAD_SHARD: return fail(chk.code, "unknown sharding %d", chk.arg);
    case GROUP_EXCLUSIVE: return fail(chk.code, "PSDR_SHARD_FORCE_COMM (RCCL) and PSDR_SHARD_PEER_COPY (no RCCL) exclude each other");
    case GROUP_TWICE: return fail(chk.code, "device %d listed twice (RCCL wants one rank per device; PSDR_SHARD_PEER_COPY allows it)", chk.arg);
    case GROUP_BAND_POW2: return fail(chk.code, "band sharding: a power-of-two number of devices, not %d", chk.arg);
    case GROUP_OK: break;
    }
    psdr_group *g = new (std::nothrow) psdr_group();
    if (!g) return fail(PSDR_ERR_NOMEM, "out of memory");
    g->n = ndevices;
    g->dev.assign(devices, devices + ndevices);
    g->ctx.assign(ndevices, nullptr);
    g->st.resize(ndevices);
    g->comm.assign(ndevices, nullptr);
    g->rbuf.resize(ndevices);
    g->sbuf.resize(ndevices);
    g->ev_rank.resize(ndevices);
    g->ev_t0.resize(ndevices);
    g->ev_t1.resize(ndevices);
    auto bail = [&](int rc) { return fail_after(rc, [&] { psdr_group_destroy(g); }); };
    for (int r = 0; r < ndevices; r++) {
        psdr_config c = *cfg;
        c.device = devices[r];
        int rc = psdr_create(&c, &g->ctx[r]);
        if (rc) return bail(rc);
        if (hipSetDevice(devices[r]) != hipSuccess || g->st[r].create()) {
            fail(PSDR_ERR_HIP, "stream creation on device %d failed", devices[r]);
            return bail(PSDR_ERR_HIP);
        }
        rc = psdr_set_stream(g->ctx[r], g->st[r]);
        if (rc) return bail(rc);
        // (events belong to the device that is current when they are created)
        if (g->ev_rank[r].create() || g->ev_t0[r].create_timing() || g->ev_t1[r].create_timing()) {
            fail(PSDR_ERR_HIP, "event creation on device %d failed", devices[r]);
            return bail(PSDR_ERR_HIP);
        }
        if (f.peer_copy && r > 0 && devices[r] != devices[0]) {
            (void)hipDeviceEnablePeerAccess(devices[0], 0);  // (direct xGMI reads; without it the copy is staged)
            (void)hipGetLastError();
        }
    }
    psdr_ctx *c0 = g->ctx[0];
    f.R = c0->R, f.is_real = c0->is_real, f.lay_mode = c0->lay.mode;
    f.max_batch = (size_t)c0->max_batch, f.half_frame_bytes = psdr_half_frame_bytes(c0), f.spec_stride = c0->spec_stride;
    f.audio_fft_size = cfg->audio_fft_size;
    g->facts = f;
    g->lay = group_layout(f);
    const GroupLayout &L = g->lay;
    if (L.comm_on) {
        int rc = g_rccl.load();
        if (rc) return bail(rc);
        const int e = g_rccl.CommInitAll(g->comm.data(), ndevices, devices);
        if (e != ncclSuccess) {
            fail(PSDR_ERR_HIP, "ncclCommInitAll over %d devices failed: %s", ndevices, g_rccl.GetErrorString(e));
            return bail(PSDR_ERR_HIP);
        }
    }
    // ---- per-sharding buffers
    if (L.banded) {  // the root's second pass writes the regions: the context is their owner
        GroupBands own;
        int rc = psdr_set_band_layout(c0, ndevices, L.halo);
        for (int b = 0; b < ndevices && !rc; b++) {
            const float *p;
            rc = psdr_band_region(c0, b, &p, &own.stride, &own.first[b], &own.bins[b]);
        }
        if (rc) return bail(rc);
        g->lay = group_layout(f, &own);
    }
    for (int b = 0; b < ndevices; b++)
        if (L.sbuf[b] && alloc_on(devices[0], g->sbuf[b], f.max_batch * L.band.stride, "band send buffer of %zu bytes")) return bail(PSDR_ERR_NOMEM);
    for (int r = 0; r < ndevices; r++)
        if (L.rbuf_bytes[r] && alloc_on(devices[r], g->rbuf[r], L.rbuf_bytes[r],
                                        f.shard == PSDR_SHARD_RAW ? "raw receive buffer of %zu bytes on device %d" : "band receive buffer of %zu bytes on device %d"))
            return bail(PSDR_ERR_NOMEM);
    if (hipSetDevice(devices[0]) != hipSuccess || g->ev0.create_timing() || g->ev1.create_timing() || g->ev_x.create()) {
        fail(PSDR_ERR_HIP, "event creation failed");
        return bail(PSDR_ERR_HIP);
    }
    // the exchange beside the next transform: spectrum broadcast, and band regions the root's second pass writes itself
    if (L.overlap) {
        c0->alt_sets = true;
        bool ok = !g->xs.create();
        for (Event &e : g->ev_xdone) ok = ok && !e.create();
        for (auto &v : g->ev_pull) {
            v.resize(ndevices);
            for (int r = 1; r < ndevices && ok; r++) ok = hipSetDevice(devices[r]) == hipSuccess && !v[r].create();
        }
        if (!ok) {
            fail(PSDR_ERR_HIP, "exchange stream / events could not be created");
            return bail(PSDR_ERR_HIP);
        }
    }
    *out = g;
    return PSDR_OK;
}

extern "C" int psdr_group_size(const psdr_group *g) { return g ? g->n : 0; }
extern "C" psdr_ctx *psdr_group_ctx(psdr_group *g, int rank) { return (g && rank >= 0 && rank < g->n) ? g->ctx[rank] : nullptr; }

// ---- audio clients: the group picks the GPU ---------------------------------------------------------------------
// A client of the group on context c: untuned and without notches, whatever PSDR_OPT_FINE_TUNE and PSDR_OPT_AUTO_NOTCH of
// the rank's context say (a migration carries the fine-tune flag as 0 and no notches); the slot is given back on failure
static int place_client(psdr_ctx *c, int l, double audio_mid, int r, int mode, bool paused, int *id) {
    int rc = psdr_client_add(c, id);
    if (rc) return rc;
    rc = psdr_client_set_fine_tune(c, *id, 0);
    if (!rc) rc = psdr_client_set_auto_notch(c, *id, 0);
    if (!rc) rc = psdr_client_set_noise_reduction(c, *id, 0, 0.0, 0.0);  // (... nor PSDR_OPT_NOISE_REDUCTION: its state is not migrated)
    if (!rc) rc = psdr_client_set_audio_blanker(c, *id, 0, 0.0, 0);  // (... nor PSDR_OPT_AUDIO_BLANKER, for the same reason)
    if (!rc) rc = psdr_client_set_audio_demodulation(c, *id, mode);
    if (!rc) rc = psdr_client_set_audio_range(c, *id, l, audio_mid, r);
    if (!rc && paused) rc = psdr_client_set_paused(c, *id, 1);
    return rc ? fail_after(rc, [&] { psdr_client_remove(c, *id); }) : PSDR_OK;
}
extern "C" int psdr_group_client_add(psdr_group *g, int l, double audio_mid, int r, int mode, int *gid_out) {
    if (!g || !gid_out) return fail(PSDR_ERR_INVALID, "null argument");
    // (a group neither migrates nor fetches IQ rows: a context of its own serves such a client)
    if (mode == PSDR_IQ) return fail(PSDR_ERR_UNSUPPORTED, "PSDR_IQ clients are not served through a group");
    if (mode == PSDR_SAM) return fail(PSDR_ERR_UNSUPPORTED, "PSDR_SAM clients are not served through a group (the carrier tail is not migrated)");
    std::lock_guard<std::mutex> lk(g->mtx);
    const int rank = group_rank_for(g->facts, l, g->next_rr);
    int id = -1;
    const int rc = place_client(g->ctx[rank], l, audio_mid, r, mode, false, &id);
    if (rc) return rc;
    if (g->facts.shard != PSDR_SHARD_BAND) g->next_rr++;
    *gid_out = gid_new(g, rank, id);
    return PSDR_OK;
}
extern "C" int psdr_group_client_remove(psdr_group *g, int gid) {
    if (!g) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->mtx);
    int rank, id, rc = gid_split(g, gid, &rank, &id);
    if (rc) return rc;
    g->clients[gid].rank = -1;
    return psdr_client_remove(g->ctx[rank], id);
}
extern "C" int psdr_group_client_set_audio_demodulation(psdr_group *g, int gid, int mode) {
    if (!g) return fail(PSDR_ERR_INVALID, "null argument");
    if (mode == PSDR_IQ) return fail(PSDR_ERR_UNSUPPORTED, "PSDR_IQ clients are not served through a group");
    if (mode == PSDR_SAM) return fail(PSDR_ERR_UNSUPPORTED, "PSDR_SAM clients are not served through a group (the carrier tail is not migrated)");
    std::lock_guard<std::mutex> lk(g->mtx);
    int rank, id, rc = gid_split(g, gid, &rank, &id);
    return rc ? rc : psdr_client_set_audio_demodulation(g->ctx[rank], id, mode);
}
extern "C" int psdr_group_client_set_paused(psdr_group *g, int gid, int paused) {
    if (!g) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->mtx);
    int rank, id, rc = gid_split(g, gid, &rank, &id);
    return rc ? rc : psdr_client_set_paused(g->ctx[rank], id, paused);
}
extern "C" int psdr_group_client_rank(psdr_group *g, int gid) {
    if (!g) return -1;
    std::lock_guard<std::mutex> lk(g->mtx);
    int rank, id;
    return gid_split(g, gid, &rank, &id) ? -1 : rank;
}
// A retune inside the client's GPU is AudioClient::set_audio_range.  Band sharding only: a window that now starts in
// another band moves the client to that band's GPU BEHIND its gid (the caller's handle does not change).  What travels:
// the demodulation state the reference keeps across a retune (src/signal.cpp:81-94 touches none of it) - the SSB
// overlap-add tail, the AM / FM baseband tail and FM's last sample (one peer copy of the current state rows, ordered
// after the old device's last batch and before the new device's next one), the mode and the paused flag.  What does NOT
// travel: the post chain's history on the GPU (DC-blocker sums, AGC gain and look-ahead: the client starts there like a
// fresh one - an AGC transient of 0.2 s, where the reference has none), and the results of the batch demodulated before
// the move (psdr_group_fetched_audio answers PSDR_ERR_NO_DATA until the new device has demodulated a batch: one frame
// at F = 1).
extern "C" int psdr_group_client_set_audio_range(psdr_group *g, int gid, int l, double audio_mid, int r) {
    if (!g) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->mtx);
    int rank, id, rc = gid_split(g, gid, &rank, &id);
    if (rc) return rc;
    const int want = g->facts.shard == PSDR_SHARD_BAND ? group_rank_for(g->facts, l, 0) : rank;
    if (want == rank) return psdr_client_set_audio_range(g->ctx[rank], id, l, audio_mid, r);
    psdr_ctx *src = g->ctx[rank], *dst = g->ctx[want];
    int mode, nid = -1, src_par;
    bool paused;
    {
        std::lock_guard<std::mutex> lk2(src->mtx);
        if (id >= (int)src->aslots.size() || !src->aslots[id].active) return fail(PSDR_ERR_INVALID, "no client %d in this group", gid);
        mode = src->aslots[id].mode;
        paused = src->aslots[id].paused;
        src_par = src->aslots[id].state_cur;  // the parity the NEXT batch would read: what the last one wrote
    }
    rc = place_client(dst, l, audio_mid, r, mode, paused, &nid);
    if (rc) return rc;
    // the state rows: [parity][slot][n/2] (ctx.h); the fresh slot reads parity 0 first.  Ordered on the two ranks' streams:
    // after everything the old device has enqueued, before anything the new one enqueues from here on; the old slot may be
    // handed out again only after the copy has read it.
    auto move_state = [&]() -> int {
        const size_t h = (size_t)src->n / 2, Ss = src->aslots.size(), Sd = dst->aslots.size();
        HIPCHK(hipSetDevice(g->dev[rank]));
        HIPCHK(hipEventRecord(g->ev_rank[rank], g->st[rank]));
        HIPCHK(hipSetDevice(g->dev[want]));
        HIPCHK(hipStreamWaitEvent(g->st[want], g->ev_rank[rank], 0));
        HIPCHK(rank_copy(g, want, dst->d_real_prev + ((size_t)0 * Sd + nid) * h, rank, src->d_real_prev + ((size_t)src_par * Ss + id) * h, h * sizeof(float)));
        HIPCHK(rank_copy(g, want, dst->d_bb_tail + ((size_t)0 * Sd + nid) * h, rank, src->d_bb_tail + ((size_t)src_par * Ss + id) * h, h * sizeof(cf)));
        HIPCHK(rank_copy(g, want, dst->d_bb_last + ((size_t)0 * Sd + nid), rank, src->d_bb_last + ((size_t)src_par * Ss + id), sizeof(cf)));
        HIPCHK(hipEventRecord(g->ev_rank[want], g->st[want]));
        HIPCHK(hipSetDevice(g->dev[rank]));
        HIPCHK(hipStreamWaitEvent(g->st[rank], g->ev_rank[want], 0));
        return PSDR_OK;
    };
    rc = move_state();
    // (failed: the client stays where it was (gid -> src), the half-made slot on the new device is given back)
    if (rc) return fail_after(rc, [&] { psdr_client_remove(dst, nid); });
    psdr_client_remove(src, id);
    g->clients[gid] = GroupClient{want, nid};
    return PSDR_OK;
}

// ---- one batch ------------------------------------------------------------------------------------------------
// raw_root: nframes + 1 raw half-frames on the root device (nullptr: the root's ingest ring from first_half on)
struct StepArgs {
    const void *raw_root;
    uint64_t first_half;
    int nframes;
    uint64_t first_frame_num;
};
static hipEvent_t op_event(psdr_group *g, const GroupOp &o) {
    switch (o.ev) {
    case EV0: return g->ev0;
    case EV1: return g->ev1;
    case EV_X: return g->ev_x;
    case EV_RANK: return g->ev_rank[o.ev_rank];
    case EV_T0: return g->ev_t0[o.ev_rank];
    case EV_T1: return g->ev_t1[o.ev_rank];
    case EV_XDONE: return g->ev_xdone[o.ev_set];
    case EV_PULL: return g->ev_pull[o.ev_set][o.ev_rank];
    case EV_NONE: break;
    }
    return nullptr;
}
// raw from the ring: the copies of exactly the halves that are sent
static int ring_wait(psdr_group *g, uint64_t first_half, int nhalves) {
    psdr_ctx *c0 = g->ctx[0];
    if (!c0->ring.d) return fail(PSDR_ERR_STATE, "psdr_ring_create() on the root context first");
    const int s0 = (int)(first_half % (uint64_t)c0->ring.nhalves);
    if (s0 + nhalves - 1 > c0->ring.nhalves) return fail(PSDR_ERR_INVALID, "frames cross the end of the ring: split the batch");
    for (int i = 0; i < nhalves; i++) {
        const int slot = (s0 + i) % c0->ring.nhalves;
        if (!c0->ring.ever_written[slot]) return fail(PSDR_ERR_STATE, "half-frame slot %d was never written", slot);
        HIPCHK(hipStreamWaitEvent(g->st[0], c0->ring.ev_written[slot], 0));
    }
    return PSDR_OK;
}
// rank r's share of the root's data of this step: where it lies on the root, and where the rank takes it
static int share_of(psdr_group *g, const StepArgs &a, int r, const void **src, void **dst) {
    psdr_ctx *c0 = g->ctx[0];
    if (g->lay.shard == PSDR_SHARD_RAW) {  // (root: in place - its own transform reads the caller's buffer / the ring)
        *src = a.raw_root ? a.raw_root : c0->ring.d + (size_t)(a.first_half % (uint64_t)c0->ring.nhalves) * g->lay.half_frame_bytes;
        *dst = r == 0 ? (void *)*src : g->rbuf[r].get();
    } else if (g->lay.shard == PSDR_SHARD_CLIENTS) {  // straight out of the root's spectrum buffer into every rank's own
        *src = c0->d_spec;
        *dst = g->ctx[r]->d_spec;
    } else {
        const float *region = (const float *)g->sbuf[r].get();
        if (g->lay.banded) PSDRCHK(psdr_band_region(c0, r, &region, nullptr, nullptr, nullptr));  // the region of THIS batch (the sets alternate)
        *src = region;
        *dst = g->rbuf[r].get();
    }
    return PSDR_OK;
}
static int group_issue(psdr_group *g, const GroupOp &o, const StepArgs &a) {
    psdr_ctx *c = g->ctx[o.rank];
    const GroupBands &B = g->lay.band;
    const float *band = (const float *)g->rbuf[o.rank].get();
    switch (o.kind) {  // what a context does sets its own device
    case OP_TRANSFORM:
        return o.rank ? psdr_process_batch(c, g->rbuf[o.rank], a.nframes) : a.raw_root ? psdr_process_batch(c, a.raw_root, a.nframes) : psdr_process_ring(c, a.first_half, a.nframes);
    case OP_PACK: return psdr_pack_band(c, a.nframes, B.first[o.band], B.bins[o.band], (float *)g->sbuf[o.band].get(), B.stride);
    case OP_DEMOD_OWN: return psdr_demod_batch(c, a.first_frame_num);
    case OP_DEMOD_FROM_SPEC: return psdr_demod_batch_from(c, (const float *)c->d_spec, c->spec_stride, a.nframes, a.first_frame_num);
    case OP_DEMOD_FROM_BAND: return psdr_demod_batch_from_band(c, band, B.stride, B.first[o.rank], B.bins[o.rank], a.nframes, a.first_frame_num);
    case OP_DEMOD_FROM_BAND_REGION: return psdr_demod_batch_from_band_region(c, band, B.stride, B.first[o.rank], B.bins[o.rank], a.nframes, a.first_frame_num);
    case OP_WATERFALL: return psdr_waterfall_batch(c, a.first_frame_num);
    default: break;
    }
    const hipStream_t s = o.xs ? (hipStream_t)g->xs : (hipStream_t)g->st[o.rank];
    const void *src = nullptr;
    void *dst = nullptr;
    HIPCHK(hipSetDevice(g->dev[o.rank]));
    switch (o.kind) {
    case OP_WAIT: HIPCHK(hipStreamWaitEvent(s, op_event(g, o), 0)); break;
    case OP_RECORD: HIPCHK(hipEventRecord(op_event(g, o), s)); break;
    case OP_RING_WAIT: return ring_wait(g, a.first_half, (int)o.arg);
    case OP_GROUP_START: NCCLCHK(g_rccl.GroupStart()); break;
    case OP_GROUP_END: NCCLCHK(g_rccl.GroupEnd()); break;
    case OP_BCAST_RAW:
    case OP_BCAST_SPEC:
        PSDRCHK(share_of(g, a, o.rank, &src, &dst));
        NCCLCHK(g_rccl.Broadcast(src, dst, o.arg, o.kind == OP_BCAST_RAW ? ncclChar : ncclFloat, 0, g->comm[o.rank], s));
        break;
    case OP_SEND_BAND:
        PSDRCHK(share_of(g, a, o.band, &src, &dst));
        NCCLCHK(g_rccl.Send(src, o.arg, ncclFloat, o.band, g->comm[0], s));
        break;
    case OP_RECV_BAND:
        PSDRCHK(share_of(g, a, o.rank, &src, &dst));
        NCCLCHK(g_rccl.Recv(dst, o.arg, ncclFloat, 0, g->comm[o.rank], s));
        break;
    case OP_PULL:
        PSDRCHK(share_of(g, a, o.rank, &src, &dst));
        HIPCHK(rank_copy(g, o.rank, dst, 0, src, o.arg));
        break;
    default: break;
    }
    return PSDR_OK;
}
// One step is its plan (groupplan.h), issued in order.  The state moves as far as operations were issued: a failed step
// leaves the events it has recorded pending, and nothing it has not.
static int group_step(psdr_group *g, const StepArgs &a) {
    psdr_ctx *c0 = g->ctx[0];
    if (a.nframes < 1 || a.nframes > c0->max_batch) return fail(PSDR_ERR_INVALID, "nframes %d outside [1, max_batch=%d]", a.nframes, c0->max_batch);
    g->state.cur_set = c0->cur_set;
    const GroupStepPlan p = group_step_plan(g->lay, g->state, !a.raw_root, a.nframes);
    g->stats = STATS_NONE;
    g->link_bytes = 0;
    for (int i = 0; i < p.n; i++) {
        const GroupOp &o = p.op[i];
        const int rc = group_issue(g, o, a);
        if (rc) return rc;
        group_commit(g->state, o.commit, p.set);
        if (o.commit & GC_TIMED) g->stats = p.stats, g->link_bytes = (double)p.link_bytes;
    }
    g->steps++;
    return PSDR_OK;
}
extern "C" int psdr_group_step(psdr_group *g, const void *d_halves_root, int nframes, uint64_t first_frame_num) {
    if (!g || !d_halves_root) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->mtx);  // (enqueue only: a step never waits for the device)
    return group_step(g, StepArgs{d_halves_root, 0, nframes, first_frame_num});
}
extern "C" int psdr_group_step_ring(psdr_group *g, uint64_t first_half, int nframes, uint64_t first_frame_num) {
    if (!g) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->mtx);
    return group_step(g, StepArgs{nullptr, first_half, nframes, first_frame_num});
}
extern "C" int psdr_group_synchronize(psdr_group *g) {
    if (!g) return fail(PSDR_ERR_INVALID, "null argument");
    for (int r = 0; r < g->n; r++) {
        int rc = psdr_synchronize(g->ctx[r]);
        if (rc) return rc;
    }
    if (g->xs) {
        HIPCHK(hipSetDevice(g->dev[0]));
        HIPCHK(hipStreamSynchronize(g->xs));
    }
    return PSDR_OK;
}
// bytes that crossed ONE root -> peer link in the last step and how long the exchange took on the root's stream (0 when
// nothing was exchanged: one device, or time not yet available).  Synchronises the root.
extern "C" int psdr_group_link_stats(psdr_group *g, double *bytes_per_link, double *exchange_ms) {
    if (!g) return fail(PSDR_ERR_INVALID, "null argument");
    if (bytes_per_link) *bytes_per_link = g->link_bytes;
    if (exchange_ms) {
        *exchange_ms = 0;
        if (g->stats == STATS_T01) {  // the slowest peer's own copy
            for (int r = 1; r < g->n; r++) {
                HIPCHK(hipSetDevice(g->dev[r]));
                HIPCHK(hipEventSynchronize(g->ev_t1[r]));
                float ms = 0;
                HIPCHK(hipEventElapsedTime(&ms, g->ev_t0[r], g->ev_t1[r]));
                *exchange_ms = std::max(*exchange_ms, (double)ms);
            }
        } else if (g->stats == STATS_EV01) {
            HIPCHK(hipSetDevice(g->dev[0]));
            HIPCHK(hipEventSynchronize(g->ev1));
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, g->ev0, g->ev1));
            *exchange_ms = ms;
        }
    }
    return PSDR_OK;
}

// ---- results: one pinned copy per GPU and batch ----------------------------------------------------------------
extern "C" int psdr_group_fetch(psdr_group *g) {
    if (!g) return fail(PSDR_ERR_INVALID, "null argument");
    bool any = false;
    for (int r = 0; r < g->n; r++) {  // (no group lock: this waits for the devices; a context's own mutex guards its slots)
        const int rc = psdr_fetch_batch(g->ctx[r]);
        if (rc == PSDR_OK)
            any = true;
        else if (rc != PSDR_ERR_STATE)  // (PSDR_ERR_STATE: no client has been demodulated on that GPU yet)
            return rc;
    }
    return any ? PSDR_OK : fail(PSDR_ERR_STATE, "no demodulated batch to fetch on any device");
}
extern "C" int psdr_group_fetched_audio(psdr_group *g, int gid, int frame, const float **audio, float *pwr, int32_t *nan_flag, const int32_t **pcm) {
    if (!g) return fail(PSDR_ERR_INVALID, "null argument");
    // (the lock is held across the lookup AND the answer: a migration or a remove + add between the two would make the call act
    // on a stale (rank, id); psdr_fetched_* never wait for a device)
    std::lock_guard<std::mutex> lk(g->mtx);
    int rank, id, rc = gid_split(g, gid, &rank, &id);
    return rc ? rc : psdr_fetched_audio(g->ctx[rank], id, frame, audio, pwr, nan_flag, pcm);
}
extern "C" int psdr_group_fetched_window(psdr_group *g, int gid, int *l, double *audio_mid, int *r) {
    if (!g) return fail(PSDR_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->mtx);
    int rank, id, rc = gid_split(g, gid, &rank, &id);
    return rc ? rc : psdr_fetched_window(g->ctx[rank], id, l, audio_mid, r);
}

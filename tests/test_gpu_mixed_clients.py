"""Every client list of psdr_demod_batch populated at once.  Each client kind that has launches of its own - the old four, PSDR_SAM,
PSDR_IQ, the tuned USB / LSB / IQ clients, the sideband SAM clients - is tied to float64 truth by its own file, in contexts that
hold that kind alone (or beside the old four).  demod_impl packs all of them into ONE parameter-ring slot and computes every
kernel's arguments from the lists' counts; the carrier, tuned and sideband tails are zeroed through element offsets.  Here the
lists are full together, and every client must come out bit for bit as it does in a context that holds its family alone -
another max_clients, so another slot count S and other slot indices.

Rig: test_gpu_sam_sideband.py's stream (an AM carrier, a 1 kHz tone, an interferer in the lower sideband) and windows, 2^12-point
IQ and 2^13-point real (R = 4096), s16 input, audio_rate 12000, 25 frames as 19 + 1 + 5.  Every comparison is bit identity within
one path: no tolerance.  The float64 anchoring is the per-family files'."""
import numpy as np
import pytest

import test_gpu_sam_sideband as SB
from helpers import CLIENT_FAMILIES, CLIENT_KINDS, assert_same_bits, read_client, row_names, set_client_kind
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NF, BATCHES, MAXB, RATE, KC = SB.NF, SB.BATCHES, SB.MAXB, SB.RATE, SB.KC
PATHS = [(360, "1"), (360, "0"), (720, "1"), (256, "1"), (1024, "1")]  # (n, PSDR_DEMOD_CHAIN): every kernel concerned
PATH_IDS = [f"{n}-chain{c}" for n, c in PATHS]

# the order the clients are added in = the order of their slots; the lists are by family, so list order is not slot order.
# "sitter" (the twelfth) is paused over the second batch
ORDER = ("USB", "TUSB", "SAMU", "IQ", "LSB", "TIQ", "SAM", "AM", "SAML", "TLSB", "FM", "TUSB", "SAMU", "USB", "TUSB", "IQ", "LSB",
         "TLSB", "SAM", "AM", "SAML", "FM", "TIQ")
SITTER = 11
FRACS = (0.37, 0.81, 0.13, 0.63, 0.29, 0.55, 0.47)  # of the tuned clients, in ORDER
FULL_SLOTS = 32
FAMILY_SLOTS = {"old": 9, "sam": 4, "iq": 5, "tuned": 11, "sb": 6}
TIQ_SLOTS = 3
SIT = {1: [("sitter", "pause", None)], 2: [("sitter", "resume", None)]}


def population(n):
    """[(name, kind, window, family)] in ORDER: the k-th client of a kind on window k % 2 of windows(n) - both on the carrier,
    floor(audio_mid) even and odd - the tuned ones with a fraction of their own"""
    wins = SB.windows(n)[:2]
    pop, seen, nfrac = [], {}, 0
    for i, kind in enumerate(ORDER):
        k = seen.get(kind, 0)
        seen[kind] = k + 1
        l, mid, r = wins[k % 2]
        if CLIENT_KINDS[kind][1]:
            mid = float(np.floor(mid)) + FRACS[nfrac]
            nfrac += 1
        pop.append(("sitter" if i == SITTER else f"{kind}{k}", kind, (l, mid, r), CLIENT_KINDS[kind][3]))
    return pop


def test_the_population_is_what_the_tests_need():
    pop = population(360)
    fams = [p[3] for p in pop]
    assert all(a != b for a, b in zip(fams, fams[1:])), "two clients of one family in neighbouring slots"
    for kind in CLIENT_KINDS:
        assert sum(1 for p in pop if p[1] == kind) >= 2, kind
    fr = [p[2][1] - np.floor(p[2][1]) for p in pop if CLIENT_KINDS[p[1]][1]]
    assert len(fr) == len(FRACS) and len(set(np.round(fr, 6))) == len(fr) and min(fr) > 0
    assert len(pop) < FULL_SLOTS and len(set(FAMILY_SLOTS.values()) | {FULL_SLOTS}) == 6
    for fam in CLIENT_FAMILIES:
        assert sum(1 for f in fams if f == fam) < FAMILY_SLOTS[fam]


class Rig:
    """one context on nf frames of the shared stream; batch(F) transforms and demodulates the next F frames"""

    def __init__(self, is_real, n, max_clients, nf=NF, post=False, pcm16=False, agc=None):
        from phantomsdr_amd import Context
        self.n, self.h = n, n // 2
        raw, _ = SB.stream(is_real, n, nf)
        self.ctx = Context(SB.SHAPES[is_real], is_real, SB.LEVELS, additional_size=n, audio_fft_size=n, audio_rate=RATE,
                           input_format="s16", max_batch=MAXB, max_clients=max_clients)
        self.d = self.ctx.dev_alloc(raw.nbytes)
        self.ctx.h2d(self.d, raw)
        if post:
            if pcm16:
                self.ctx.set_option(self.ctx.OPT_POST_CHAIN_PCM16, 1)
            if agc is not None:
                self.ctx.set_option(self.ctx.OPT_POST_CHAIN_AGC, agc)
            self.ctx.set_post_chain(True)
        self.frame = 0

    def add(self, kind, win):
        from phantomsdr_amd import AudioClient
        g = AudioClient(self.ctx)
        set_client_kind(g, kind)
        g.set_audio_range(*win)
        return g

    def batch(self, F):
        self.ctx.process_batch(self.d, F, offset_bytes=self.frame * self.ctx.half_frame_bytes())
        self.ctx.demod_batch(self.frame)
        self.frame += F

    def close(self):
        self.ctx.dev_free(self.d)
        self.ctx.close()


def play(is_real, n, pop, script, batches, max_clients, only=None, nf=NF, post=False, pcm16=False, agc=None):
    """pop: the clients added before the first batch, in this order; script: {batch index: [(name, op, arg)]} carried out before
    that batch - "kind" (arg: the new kind), "pause", "resume", "remove", "add" (arg: (kind, window)); only: the names that
    exist in this run (everything that concerns another name is left out).
    -> ({name: per batch None (no client, or paused) or (kind, arrays of read_client[, the fetched PCM16 rows])}, {name: slot})"""
    rig = Rig(is_real, n, max_clients, nf=nf, post=post, pcm16=pcm16, agc=agc)
    try:
        cl, kinds, paused, got, ids = {}, {}, set(), {}, {}

        def add(name, kind, win, bi):
            cl[name], kinds[name] = rig.add(kind, win), kind
            got[name], ids[name] = [None] * bi, cl[name].id

        for name, kind, win, _ in pop:
            if only is None or name in only:
                add(name, kind, win, 0)
        for bi, F in enumerate(batches):
            for name, op, arg in script.get(bi, ()):
                if only is not None and name not in only:
                    continue
                if op == "add":
                    add(name, arg[0], arg[1], bi)
                elif op == "kind":
                    set_client_kind(cl[name], arg)
                    kinds[name] = arg
                elif op == "remove":
                    cl.pop(name).on_close()
                else:
                    cl[name].set_paused(op == "pause")
                    (paused.add if op == "pause" else paused.discard)(name)
            rig.batch(F)
            if pcm16:
                rig.ctx.fetch_begin(rig.ctx.FETCH_AUDIO | rig.ctx.FETCH_PCM | rig.ctx.FETCH_IQ)
                rig.ctx.fetch_end()
            for name in got:
                if name not in cl or name in paused:
                    got[name].append(None)
                    continue
                g, kind = cl[name], kinds[name]
                rows = tuple(x[:F].copy() for x in read_client(g, kind, MAXB, pcm=post))
                if pcm16 and CLIENT_KINDS[kind][0] != "IQ":
                    rows += (np.stack([rig.ctx.fetched_pcm16(g.id, f) for f in range(F)]),)
                got[name].append((kind, rows))
        return got, ids
    finally:
        rig.close()


def assert_clients_equal(a, b, names, tag, alive=True):
    """per name and batch: the same kind and the same bits in every array; alive: rows that are not all zero, no NaN flag"""
    for name in names:
        assert len(a[name]) == len(b[name]), (tag, name)
        for bi, (x, y) in enumerate(zip(a[name], b[name])):
            assert (x is None) == (y is None), f"{tag}: {name} batch {bi}: served in one run only"
            if x is None:
                continue
            assert x[0] == y[0]
            what = row_names(x[0], pcm=True) + ("pcm16",)
            assert_same_bits(x[1], y[1], f"{tag}: {name} ({x[0]}) batch {bi}", what)
            if alive:
                assert np.abs(x[1][0]).max() > 0 and not x[1][2].any(), f"{tag}: {name} ({x[0]}) batch {bi}: empty rows or a NaN flag"


def family_names(pop, fam):
    return [p[0] for p in pop if p[3] == fam]


# ---- A1. the full house against one context per family ------------------------------------------------------------------

@pytest.mark.parametrize("is_real", [0, 1])
@pytest.mark.parametrize("n,chain", PATHS, ids=PATH_IDS)
def test_full_house_equals_the_five_family_contexts(n, chain, is_real, monkeypatch):
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    pop = population(n)
    full, ids = play(is_real, n, pop, SIT, BATCHES, FULL_SLOTS)
    assert [ids[p[0]] for p in pop] == sorted(ids.values()), "slot order is the order of psdr_client_add"
    assert full["sitter"][1] is None and full["sitter"][2] is not None
    for fam in CLIENT_FAMILIES:
        names = family_names(pop, fam)
        ref, rid = play(is_real, n, pop, SIT, BATCHES, FAMILY_SLOTS[fam], only=names)
        assert any(ids[k] != rid[k] for k in names)
        assert_clients_equal(full, ref, names, f"n {n} chain {chain} real {is_real}: the full house against the {fam} context")
    # in the tuned context, too, the tuned list holds USB / LSB clients in front of the IQ ones: the tuned IQ clients also
    # against a context in which that list starts with them
    names = [p[0] for p in pop if p[1] == "TIQ"]
    ref, _ = play(is_real, n, pop, SIT, BATCHES, TIQ_SLOTS, only=names)
    assert_clients_equal(full, ref, names, f"n {n} chain {chain} real {is_real}: the full house against the tuned IQ clients alone")


# ---- A2. the same with the post chain on --------------------------------------------------------------------------------

def post_population(n):
    """IQ1 and TIQ1 start as AM clients: in the middle batch they are an IQ and a tuned IQ client WITH a post-chain history -
    beside IQ0 and TIQ0, which have none yet - and all four are AM clients in the last batch"""
    pop = [(name, "AM" if name in ("IQ1", "TIQ1") else kind, win, fam) for name, kind, win, fam in population(n)]
    script = {1: SIT[1] + [("IQ1", "kind", "IQ"), ("TIQ1", "kind", "TIQ")],
              2: SIT[2] + [(k, "kind", "AM") for k in ("IQ0", "IQ1", "TIQ0", "TIQ1")]}
    return pop, script


@pytest.mark.parametrize("n,chain,is_real,agc,pcm16", [(360, "1", 0, 1, False), (360, "1", 0, 0, False), (360, "1", 0, 1, True),
                                                         (256, "1", 1, 1, False), (256, "1", 1, 0, False)])
def test_full_house_with_the_post_chain_on(n, chain, is_real, agc, pcm16, monkeypatch):
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    pop, script = post_population(n)
    kw = dict(post=True, pcm16=pcm16, agc=agc)
    full, _ = play(is_real, n, pop, script, BATCHES, FULL_SLOTS, **kw)
    for name, kinds in (("IQ0", ["IQ", "IQ", "AM"]), ("IQ1", ["AM", "IQ", "AM"]), ("TIQ0", ["TIQ", "TIQ", "AM"]), ("TIQ1", ["AM", "TIQ", "AM"])):
        assert [b[0] for b in full[name]] == kinds, name
    for fam in CLIENT_FAMILIES:
        ref, _ = play(is_real, n, pop, script, BATCHES, FAMILY_SLOTS[fam], only=family_names(pop, fam), **kw)
        assert_clients_equal(full, ref, family_names(pop, fam), f"n {n} real {is_real} agc {agc} pcm16 {pcm16}: the full house against the {fam} context")
    # the PCM of one client of every audio kind: the oracle's DC blocker + AGC + int16 conversion fed the GPU's own float rows
    total = 0
    for name in ("USB0", "LSB0", "AM0", "FM0", "SAM0", "SAMU0", "SAML0", "TUSB0", "TLSB0"):
        ch = O.PostChain(RATE)
        for bi, (kind, rows) in enumerate(full[name]):
            audio, pcm = rows[0], rows[5 if CLIENT_KINDS[kind][0] == "SAM" else 3]
            for f in range(len(audio)):
                want = ch.process(audio[f])
                assert np.array_equal(pcm[f], want), f"{name} batch {bi} frame {f}: {np.count_nonzero(pcm[f] != want)} samples differ"
                if pcm16:
                    assert rows[-1].dtype == np.int16 and np.array_equal(rows[-1][f].astype(np.int32), want), (name, bi, f)
                total += int(np.count_nonzero(want))
    assert total > 1000, "the AGC never opened: the test did not exercise the chain"


# ---- A3. every way to read ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("is_real", [0, 1])
def test_every_way_to_read_the_full_house(is_real):
    """psdr_fetch_batch and psdr_fetch_begin(AUDIO | IQ) / _end against psdr_read_*: the IQ and SAM slots are interleaved with
    every other kind's, so the fetched spans - lowest to highest IQ slot, lowest to highest SAM slot - hold foreign slots"""
    n = 360
    pop = population(n)
    rig = Rig(is_real, n, FULL_SLOTS)
    try:
        cl = {name: (rig.add(kind, win), kind) for name, kind, win, _ in pop}
        iq_ids = [g.id for g, kind in cl.values() if CLIENT_KINDS[kind][0] == "IQ"]
        for bi, F in enumerate(BATCHES):
            cl["sitter"][0].set_paused(bi == 1)
            rig.batch(F)
            want = {k: read_client(g, kind, MAXB) for k, (g, kind) in cl.items() if not (k == "sitter" and bi == 1)}
            for how in ("fetch_batch", "fetch"):
                if how == "fetch_batch":
                    rig.ctx.fetch_batch()
                else:
                    rig.ctx.fetch_begin(rig.ctx.FETCH_AUDIO | rig.ctx.FETCH_IQ)
                    rig.ctx.fetch_end()
                lo, ns, nbytes = rig.ctx.fetched_iq_span()
                assert lo == min(iq_ids) and ns == max(iq_ids) - lo + 1 > len(iq_ids) and nbytes == ns * F * (n // 2) * 8
                for k, (g, kind) in cl.items():
                    tag = f"real {is_real} batch {bi} {how}: {k}"
                    mode = CLIENT_KINDS[kind][0]
                    if k not in want:
                        continue
                    w = want[k]
                    for f in range(F):
                        row, pw, nan = rig.ctx.fetched_iq(g.id, f) if mode == "IQ" else rig.ctx.fetched_audio(g.id, f)
                        assert row.tobytes() == w[0][f].tobytes() and np.abs(row).max() > 0, tag
                        assert np.float32(pw).tobytes() == w[1][f].tobytes() and nan == int(w[2][f]) == 0, tag
                        if mode == "SAM":
                            lv, off = rig.ctx.fetched_carrier(g.id, f)
                            assert np.float32(lv).tobytes() == w[3][f].tobytes() and np.float32(off).tobytes() == w[4][f].tobytes(), tag
                            assert lv > 0, tag
    finally:
        rig.close()


# ---- A4. one client migrates through the lists ---------------------------------------------------------------------------

MIG_BATCHES = (3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4)
MIG_NF = sum(MIG_BATCHES)
# the migrant's kind per batch: "-" paused, None removed, then a FRESH client ("mig2") in the slot the migrant left.
# Every tail is double-buffered and a slot's halves swap with each batch it is listed in: a stretch that is not zeroed reads a
# STALE tail only if an earlier stretch wrote the half it starts from.  The three sideband stretches of the first client all
# start from the half none of them writes (batches 2, 4, 8); the fresh client's halves start over, so its tuned USB stretch
# (batch 12) starts from the half the tuned stretches of batches 1 and 5 wrote, and its SAM-U stretch (batch 13) from the half
# the sideband and carrier tails of batches 2, 4 and 8 went to
MIG_KINDS = ("USB", "TUSB", "SAMU", "TIQ", "SAML", "TLSB", "IQ", "SAM", "SAMU", "-", "AM", None, "TUSB", "SAMU")


def migration(n):
    """(population with the migrant in a middle slot, its script, the script of the fresh clients and the SAM twin beside it
    in the context of its own)"""
    l, _, r = SB.windows(n)[0]
    win = (l, KC + 0.37, r)
    pop = population(n)
    pop.insert(SITTER + 1, ("mig", "USB", win, None))
    fams = [p[3] for p in pop]
    assert fams[SITTER] != "old" != fams[SITTER + 2]
    script = {bi: [("mig", "kind", k)] for bi, k in enumerate(MIG_KINDS[:12]) if bi and k not in ("-", None)}
    script[9] = [("mig", "pause", None)]
    script[10] = [("mig", "resume", None)] + script[10]
    script[11] = [("mig", "remove", None)]
    script[12] = [("mig2", "add", ("TUSB", win))]
    script[13] = [("mig2", "kind", "SAMU")]
    for bi, ops in SIT.items():
        script[bi] = script[bi] + ops
    # beside the migrant in its own context: a fresh client of the kind at the boundary where a SAM-U / SAM-L stretch starts
    # from another list (2, 4), a SAM (both) twin from the boundary where the migrant becomes SAM (7), a fresh SAM-U client
    # where the migrant goes on from SAM (both) to SAM-U (8), a fresh tuned USB and a fresh SAM-U client in slots never used
    # before where the client in the re-used slot becomes one (12, 13)
    beside = {2: [("fresh_u", "add", ("SAMU", win))], 4: [("fresh_l", "add", ("SAML", win))], 7: [("twin", "add", ("SAM", win))],
              8: [("fresh_u2", "add", ("SAMU", win))], 12: [("fresh_t", "add", ("TUSB", win))], 13: [("fresh_u3", "add", ("SAMU", win))]}
    return pop, script, beside


@pytest.mark.parametrize("is_real", [0, 1])
@pytest.mark.parametrize("n,chain", [(360, "1"), (360, "0"), (256, "1")], ids=["360-chain1", "360-chain0", "256-chain1"])
def test_a_client_migrates_through_every_list(n, chain, is_real, monkeypatch):
    monkeypatch.setenv("PSDR_DEMOD_CHAIN", chain)
    pop, script, beside = migration(n)
    tag = f"n {n} chain {chain} real {is_real}"
    full, ids = play(is_real, n, pop, script, MIG_BATCHES, FULL_SLOTS, nf=MIG_NF)
    assert ids["mig2"] == ids["mig"] == SITTER + 1, "the fresh client took the slot the migrant left"
    assert [b and b[0] for b in full["mig"]] == [None if k in ("-", None) else k for k in MIG_KINDS[:12]] + [None, None]
    assert [b and b[0] for b in full["mig2"]] == [None] * 12 + list(MIG_KINDS[12:])
    # 1. the neighbours: as in a run without the migrant
    others = [p[0] for p in pop if p[0] != "mig"]
    without, _ = play(is_real, n, pop, script, MIG_BATCHES, FULL_SLOTS, only=others, nf=MIG_NF)
    assert_clients_equal(full, without, others, f"{tag}: beside the migrant against without it")
    # 2. the migrant: as the same script in a context of its own - another S, another slot
    solo_script = {bi: script.get(bi, []) + beside.get(bi, []) for bi in range(len(MIG_BATCHES))}
    solo, sid = play(is_real, n, [p for p in pop if p[0] == "mig"], solo_script, MIG_BATCHES, 8, nf=MIG_NF,
                     only=("mig", "mig2", "fresh_u", "fresh_l", "twin", "fresh_u2", "fresh_t", "fresh_u3"))
    assert sid["mig"] == sid["mig2"] == 0 and len(set(sid.values())) == len(sid) - 1
    assert_clients_equal(full, solo, ("mig", "mig2"), f"{tag}: the migrant in the full house against a context of its own")
    # 3. the first batch of a stretch.  SAM-U from tuned USB, SAM-L from tuned IQ: carrier tail and B' tail both from zero - a
    #    fresh client's audio, pwr and carrier records
    mig = solo["mig"]
    assert_same_bits(mig[2][1], solo["fresh_u"][2][1], f"{tag}: SAM-U entered from tuned USB against a fresh SAM-U client")
    assert_same_bits(mig[4][1], solo["fresh_l"][4][1], f"{tag}: SAM-L entered from tuned IQ against a fresh SAM-L client")
    #    SAM-U entered from SAM (both) CONTINUES the carrier: the records of a SAM (both) twin that never changed, not a fresh client's
    for bi in (7, 8):
        assert_same_bits(mig[bi][1][3:5], solo["twin"][bi][1][3:5], f"{tag}: batch {bi}: carrier records against the SAM (both) twin's", ("carrier level", "carrier offset"))
    assert mig[8][1][3].tobytes() != solo["fresh_u2"][8][1][3].tobytes(), f"{tag}: the carrier restarted at SAM (both) -> SAM-U"
    #    the slot the migrant left: tails and phase from zero, as in a slot never used
    assert_same_bits(solo["mig2"][12][1], solo["fresh_t"][12][1], f"{tag}: a fresh tuned USB client in the re-used slot against one in a new slot")
    assert_same_bits(solo["mig2"][13][1], solo["fresh_u3"][13][1], f"{tag}: SAM-U entered from tuned USB in the re-used slot against a fresh SAM-U client")

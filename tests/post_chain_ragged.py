"""The cases of tests/test_gpu_post_chain_ragged.py: the post chain's forms (tests/post_chain_forms.py) with streams of
different lengths in one recurrence work-group - frames flagged non-finite, frames the squelch closes, paused clients - and
with the per-client features in front of and inside the chain (AGC profiles, audio filter, squelch).  Shared with the host-side
checks of the same cases (tests/test_post_chain_ragged_cover.py).

A case takes its geometry from the entry of post_chain_forms.CASES of the same name - rate, n, slots, max_batch, AGC option,
pcm16, occupied slots, late slot and the plan literal it must still resolve to - and has a batch list of its own (BATCHES),
longer where the drops ask for it.  192000-n248-600 is left out: its kernel, k_pc_mad<true>, runs at 48000, and its look-ahead
of 38400 samples does not fit a test of a few seconds once frames are dropped.

Input: a caller-owned linear spectrum per frame for psdr_demod_batch_from (2^12-point IQ context: client order), complex
Gaussian noise of a fixed seed at a level under which the AGC opens.  The clients are post_chain_forms.client_spec's disjoint
windows, so a NaN written into one bin of client k's window flags that frame for client k alone: the drop script is per client
and per frame.  What is scripted is poison[k][f], the NaN bins; alive[k][f], the frames that survive the NaN guard, follows from
it by the reference's rule (carries(): a USB or LSB client loses the poisoned frame, an AM client the next one it demodulates
too, an FM client the next two).  The poison comes from a fixed seed plus forced edges, by role:

  batch 0           client 0's first frame is dropped; where max_batch > 64, client 2 gets drops and survivors in every block
                    of 64 frames (the later ballots of k_pc_index)
  batch 1           client 1's (its window's owner's) last frame is dropped
  batch 2           the late client joins; its first frame is dropped
  batch 3 (PAUSE)   every client with an AGC profile is paused for this one batch: a pause leaves state untouched and is another
                    path than a drop flag - and the batch travels without a profile table, so the kernels without profiles get
                    streams of different lengths too: client 0, never paused, loses the batch's last frame (in the cases of
                    four slots it is the only stream there: a partial stream beside lanes of len 0)
  batch 4 (EMPTY)   one client loses every frame (len = 0) while another of the same recurrence work-group keeps all of them:
                    clients 0 -> 2 in the cases of four slots; in the 64-lane cases the client in slot 63 against the one in
                    slot 0.  The all-dropped client has no profile: it is never paused
  batch 5 (WHOLE)   both clients of the second work-group of 64 slots (slots 64 and 127) keep every frame while the client in
                    slot 128 loses one: where the plan is direct = 1, k_pc_ma2 reads one work-group DIRECT and gathers its
                    neighbour in the same launch
  every batch       but the paused one: should no work-group hold two clients with different surviving counts, client 0 loses
                    frames until one does
  the last batch    the squelch client's is left whole, and the key is up: every client is heard in it

Features, by rule over the client index k of n clients (features()): the audio filter (test_gpu_audio_filter.py's "two"
preset at the case's rate) on client 0 of four or on the last client, its twin - the same window and mode, another slot, no
filter: it shares the owner's drops - on client 1 or n - 3; the squelch on client n // 2, its window's bins keyed per frame
between full level and -30 dB; AGC profiles (one the oracle can express, one capped, one manual with a non-zero gain) on
clients 1, 2, 3 of four, or on 1, 2, n - 4, n - 2 (the late one) and n - 1: with more than 64 slots one of each feature sits
in a slot of 64 or above.

rules() checks all of it for every case without a GPU (the oracle's demodulator gives the squelch client's pwr)."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import agc_profile_model as M
import post_chain_forms as PF
import squelch_model as SQ
from oracle import oracle as O

N, LEVELS = PF.N, PF.LEVELS
SEED = 211
SCALE = 1e-3          # the noise's level per component
LOW_DB = -30.0        # the squelch client's keyed-down frames
P_DROP, P_DROP_SQUELCH = 0.15, 0.08
PAUSE, EMPTY, WHOLE = 3, 4, 5
LATE_BATCH = PF.LATE_BATCH

# as short as the roles (batches 0 to 5) and the look-ahead allow: the late, paused, capped client of the 48 kHz cases needs 77
# kept frames before its AGC opens.  What those two cases cost beyond their whole-stream twins is the host model of the profile
# clients (samples x look-ahead), not GPU time
BATCHES = {
    "1000-n248": (4, 3, 4, 2, 4, 4, 4, 4, 3),
    "3200-n248": (6, 5, 6, 3, 6, 6, 6, 4),
    "8000-n248": (9, 7, 9, 4, 9, 9, 9, 6),
    "8000-n248-agc0": (9, 7, 9, 4, 9, 9, 9, 6),
    "8000-n248-pcm16": (9, 7, 9, 4, 9, 9, 9, 6),
    "16000-n248": (12, 9, 12, 7, 12, 12, 12, 12, 8),
    "12000-n8": (256, 201, 5, 256, 191, 256, 256, 256, 256, 130),
    "12000-n32": (64, 50, 64, 45, 64, 64, 64, 64, 40),
    "12000-n360-600": (3, 2, 9, 9, 7, 9, 9, 6),
    "8000-n248-600": (4, 3, 9, 9, 7, 9, 9, 6),
    "48000-n248-600": (8, 5, 33, 33, 30, 33, 20),
    "12000-n360-2000": (3, 2, 9, 9, 7, 9, 9, 6),
    "48000-n248-1600": (8, 5, 33, 33, 30, 33, 20),
}
CASES = {name: PF.CASES[name]._replace(batches=b) for name, b in BATCHES.items()}

# ---- the per-client features -----------------------------------------------------------------------------------------------
REFERENCE = dict(desired=0.2, attack_ms=50.0, release_ms=300.0, max_gain=0.0, manual=0, manual_gain=0.0)
EXPRESSIBLE = dict(REFERENCE, attack_ms=5.0, release_ms=100.0, desired=0.5)   # orc_agc_create takes these numbers
# (the cap binds: under this noise the uncapped gain settles between 1.5 and 21, by the case, and a release of 10 ms brings the
# gain to within a tenth of the cap in 23 ms of stream - cap_binds() checks both in the cover test and in the GPU test)
CAPPED = dict(REFERENCE, attack_ms=5.0, release_ms=10.0, max_gain=0.1)
MANUAL = dict(REFERENCE, manual=1, manual_gain=40.0, attack_ms=5.0, release_ms=100.0)
# the squelch: thresholds against the window's nominal full level (full_db), attack and hang in frames
SQ_OPEN, SQ_CLOSE, SQ_ATTACK, SQ_HANG = -12.0, -18.0, 2, 1
SQ_SPARE_DB = 3.0     # every keyed frame's pwr keeps this far from both thresholds (rules())

Features = namedtuple("Features", "filter twin squelch profiles")
Expect = namedtuple("Expect", "pcm gain peak_gain uncapped")


def features(case):
    """which client index has what: filter, twin, squelch (one each) and {k: profile}"""
    n = len(PF.slots_of(case))
    if n == 4:
        return Features(0, 1, 2, {1: EXPRESSIBLE, 2: CAPPED, 3: MANUAL})
    return Features(n - 1, n - 3, n // 2, {1: CAPPED, 2: MANUAL, n - 4: EXPRESSIBLE, n - 2: CAPPED, n - 1: MANUAL})


def profile_kind(case, k):
    p = features(case).profiles[k]
    return "expressible" if p is EXPRESSIBLE else "capped" if p is CAPPED else "manual"


def owner(case, k):
    """the client whose window (and hence whose drops) client k has: itself, but for the twin"""
    ft = features(case)
    return ft.filter if k == ft.twin else k


def client_spec(case, k):
    """(mode, l, mid, r) of the case's k-th client: post_chain_forms.client_spec's, the twin has the filter client's"""
    return PF.client_spec(case, owner(case, k))


def work_group(case, slot):
    """the recurrence work-group of a slot, from the case's plan"""
    return slot // case.plan["lanes"]


def starts(case):
    """the first frame of every batch, and the total behind them"""
    return tuple(int(v) for v in np.concatenate([[0], np.cumsum(case.batches)]))


def paused(case, k, b):
    return b == PAUSE and k in features(case).profiles and PF.start_frame(case, PF.slots_of(case)[k]) <= starts(case)[b]


def has_table(case, b):
    """does batch b travel with the AGC profile table (agcplan.h agc_profile_plan: a client with a profile has a stream in it)"""
    s0 = starts(case)[b]
    return any(not paused(case, k, b) and PF.start_frame(case, PF.slots_of(case)[k]) <= s0 for k in features(case).profiles)


def squelch_key(case):
    """1 = full level, 0 = LOW_DB, per frame: eight frames up, two down, counted from the end (the last five frames are up: the
    gate is open in the last batch)"""
    total = sum(case.batches)
    return np.array([0 if (total - 1 - f) % 10 in (5, 6) else 1 for f in range(total)], np.int32)


def full_db(case):
    """the nominal pwr of the squelch client's window at full level, in dB: pwr is the sum of |bin|^2 over [l, r)"""
    _, l, _, r = client_spec(case, features(case).squelch)
    return 10 * np.log10((r - l) * 2 * SCALE * SCALE)


def squelch_params(case):
    """(open_db, close_db, attack, hang) of the squelch client"""
    return (round(full_db(case) + SQ_OPEN, 1), round(full_db(case) + SQ_CLOSE, 1), SQ_ATTACK, SQ_HANG)


# ---- the drop script -------------------------------------------------------------------------------------------------------
def carries(case, k):
    """how many of the frames client k demodulates behind a NaN frame are flagged too.  USB and LSB keep their tail behind the NaN
    guard: none.  AM and FM keep the second half of a frame's baseband for the next one in front of it (src/signal.cpp:235,
    266-271): one; FM's first sample pairs with the last one of the frame before (:258-262), which that made NaN: two"""
    return {"USB": 0, "LSB": 0, "AM": 1, "FM": 2}[client_spec(case, k)[0]]


@functools.lru_cache(maxsize=None)
def _script(name):
    case = CASES[name]
    slots, st = PF.slots_of(case), starts(case)
    n, total = len(slots), st[-1]
    ft = features(case)
    rng = np.random.default_rng([SEED, zlib.crc32(name.encode())])   # (from the name: a new case moves no other's script)
    poison = np.zeros((n, total), bool)
    for k in range(n):
        p = P_DROP_SQUELCH if k == ft.squelch else P_DROP
        poison[k] = rng.random(total) < p / (1 + carries(case, k))
    big = n > 4
    gone, kept = (3, 0) if big else (0, 2)

    def batch(k, b, clean=False):
        k = owner(case, k)
        if clean and carries(case, k):   # (the frames it demodulates in front of a batch that is to stay whole)
            before = np.nonzero(present(name)[k, :st[b]])[0]
            poison[k, before[len(before) - carries(case, k):]] = False
        return poison[k, st[b]:st[b + 1]]
    batch(kept, EMPTY, True)[:] = False
    batch(ft.squelch, len(case.batches) - 1, True)[:] = False   # (its last batch is heard)
    if big:
        batch(4, WHOLE, True)[:] = False
        batch(5, WHOLE, True)[:] = False
        batch(6, WHOLE)[1] = True
    batch(0, 0)[0] = True
    batch(1, 1)[-1] = True
    if case.late is not None:
        batch(slots.index(case.late), LATE_BATCH)[0] = True
    batch(gone, EMPTY)[:] = True
    batch(0, PAUSE)[-1] = True   # (client 0 is never paused: a partial stream beside the paused lanes' empty ones)
    if case.max_batch > 64:
        row = batch(2, 0)
        for m in range(0, len(row), 64):
            row[m:m + 64] = False
            for i in (2, 10, 37, 60):
                if m + i < len(row) - 2:
                    row[m + i] = True
    def flags():
        alive = np.zeros((n, total), bool)
        for k in range(n):
            poison[k] = poison[owner(case, k)]
            poison[k, :PF.start_frame(case, slots[k])] = False   # (not there yet)
            since = carries(case, k)   # frames demodulated since the last NaN frame (a paused client: what it left behind waits)
            for f in np.nonzero(present(name)[k])[0]:
                since = -1 if poison[k, f] else since
                alive[k, f] = since >= carries(case, k)
                since += 1
        return alive

    def level(alive, b):   # no work-group has two clients with different surviving counts
        counts = {}
        for k in range(n):
            if present(name)[k, st[b]]:
                counts.setdefault(work_group(case, slots[k]), set()).add(int(alive[k, st[b]:st[b + 1]].sum()))
        return not any(len(c) > 1 for c in counts.values())
    alive = flags()
    for b in range(len(case.batches)):   # every batch but the paused one is ragged: client 0 (USB: nothing spills over) loses more
        i = 1
        while b != PAUSE and level(alive, b) and i < case.batches[b]:
            poison[0, st[b] + i] = True
            alive = flags()
            i += 1
    poison.setflags(write=False)
    alive.setflags(write=False)
    return poison, alive


@functools.lru_cache(maxsize=None)
def present(name):
    """present[k][f]: client k demodulates frame f - it has joined and is not paused"""
    case = CASES[name]
    slots, st = PF.slots_of(case), starts(case)
    out = np.zeros((len(slots), st[-1]), bool)
    for k, slot in enumerate(slots):
        for b in range(len(case.batches)):
            if st[b] >= PF.start_frame(case, slot) and not paused(case, k, b):
                out[k, st[b]:st[b + 1]] = True
    out.setflags(write=False)
    return out


def alive(case_name):
    """alive[k][f]: does frame f of client k survive the NaN guard (False before a late client's first frame and while paused)"""
    return _script(case_name)[1]


def poison(case_name):
    """poison[k][f]: frame f holds a NaN in client k's window"""
    return _script(case_name)[0]


def spectra(name):
    """the case's spectra [frames][N] complex64 in client order: noise, the squelch client's window keyed, one NaN in the
    window of every (client, frame) the script drops"""
    case = CASES[name]
    slots, total = PF.slots_of(case), sum(case.batches)
    rng = np.random.default_rng([SEED + 1, zlib.crc32(name.encode())])
    x = np.empty((total, N), np.complex64)
    x.real = rng.standard_normal((total, N), np.float32) * np.float32(SCALE)
    x.imag = rng.standard_normal((total, N), np.float32) * np.float32(SCALE)
    ft = features(case)
    _, l, _, r = client_spec(case, ft.squelch)
    x[squelch_key(case) == 0, l:r] *= np.float32(10 ** (LOW_DB / 20))
    for k in range(len(slots)):
        _, l, _, r = client_spec(case, k)
        x[poison(name)[k], l + 1] = np.nan
    return x


# ---- the oracle's demodulator in the GPU's place ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def oracle_run(name):
    """-> per client k: (audio rows [frames][h], pwr [frames], dropped [frames]) of the frames the client demodulates (present();
    the other rows are zero), the oracle's AudioClient over spectra(name)"""
    case = CASES[name]
    slots, total, n = PF.slots_of(case), sum(case.batches), case.n
    x = spectra(name)
    ref = np.roll(x, N // 2 + 1, axis=1)   # the reference's bin order; the rows are in a client's own
    ref = np.ascontiguousarray(np.concatenate([ref, ref[:, :n + 8]], axis=1))
    out = []
    for k, slot in enumerate(slots):
        mode, l, m, r = client_spec(case, k)
        o = O.AudioClient(False, n, case.rate, N)
        o.set_audio_demodulation(mode)
        o.set_audio_range(l, m, r)
        audio, pwr, dropped = np.zeros((total, n // 2), np.float32), np.zeros(total, np.float32), np.zeros(total, bool)
        for f in np.nonzero(present(name)[k])[0]:
            audio[f], pwr[f], _, dropped[f] = o.send_audio(ref[f], f, stats=False)
            if dropped[f]:   # (the reference leaves before it hands pwr out: the sum as numpy forms it - NaN for a poisoned frame)
                pwr[f] = np.sum(np.abs(x[f, l:r].astype(np.complex64)) ** 2, dtype=np.float32)
        out.append((audio, pwr, dropped))
    return out


def squelch_flags(case, pwr, state=(0, 0)):
    """squelch_model.run with the case's parameters -> (flags, state)"""
    o, c, a, h = squelch_params(case)
    return SQ.run(pwr, SQ.threshold(o), SQ.threshold(c), a, h, state)


def keep_mask(name, squelch_open):
    """keep[k][f] = alive & open & not paused, with the squelch client's open flags [frames] given"""
    case = CASES[name]
    st, ft = starts(case), features(case)
    keep = alive(name).copy()
    keep[ft.squelch] &= np.asarray(squelch_open, bool)
    for k in ft.profiles:
        for b in range(len(case.batches)):
            if paused(case, k, b):
                keep[k, st[b]:st[b + 1]] = False
    return keep


# ---- the expectation ----------------------------------------------------------------------------------------------------------
def expected_pcm(name, audio, keep, exe, tmp, tag):
    """{k: PCM rows [kept frames][h]} from float rows audio[k] [frames][h] and keep[k][f]: clients without a profile through
    oracle.PostChain, clients with one through the oracle's DC blocker, the profile's AGC (the host program over agcplan.h; the
    oracle's own where it can express the profile) and the oracle's int16 conversion -> Expect: pcm, {k: carried gain}, and for
    the capped clients {k: the largest gain} and {k: the PCM of the same profile without its cap}"""
    case = CASES[name]
    ft, D, L = features(case), case.rate // 750 * 2, case.rate // 5
    out, gains, jobs = {}, {}, []
    for k in range(len(audio)):
        rows = np.ascontiguousarray(audio[k][keep[k]])
        if k in ft.profiles:
            jobs.append((k, M.dc_block(rows, delay=D)))
        else:
            out[k] = O.PostChain(case.rate).process(rows.reshape(-1)).reshape(rows.shape)
    capped = [(k, y) for k, y in jobs if ft.profiles[k] is CAPPED]
    runs = M.model_runs(exe, tmp, [(y, [(y.size, 0, ft.profiles[k])]) for k, y in jobs] + [(y, [(y.size, 0, dict(CAPPED, max_gain=0.0))]) for _, y in capped],
                        rate=case.rate, look=L, tag=tag)
    peak, uncapped = {}, {}
    for (k, y), (z, g) in zip(jobs, runs):
        if ft.profiles[k] is EXPRESSIBLE:
            z = M.oracle_agc(y, ft.profiles[k], rate=case.rate)
        out[k] = M.to_int16(z).reshape(-1, case.n // 2)
        gains[k] = g[-1]
        if ft.profiles[k] is CAPPED:
            peak[k] = g.max()
    for (k, _), (z, _) in zip(capped, runs[len(jobs):]):
        uncapped[k] = M.to_int16(z).reshape(-1, case.n // 2)
    return Expect(out, gains, peak, uncapped)


def cap_binds(e):
    """the capped clients of an Expect whose cap does not act: the gain stays below it, or the PCM is the uncapped profile's"""
    cap = np.float32(CAPPED["max_gain"])
    return [k for k in e.uncapped if not (0.9 * cap < e.peak_gain[k] <= cap) or np.array_equal(e.pcm[k], e.uncapped[k])]


# ---- the instantiations a case launches --------------------------------------------------------------------------------------
def kernels(plan, table):
    """the chain's kernels of a batch, from its plan (a dict of strings, post_chain_forms.resolve) and whether it travels with a
    profile table: postchain.hip post_chain_enqueue's choices, as names"""
    tf = {"0": "false", "1": "true"}
    own, att, p16 = tf[plan["own"]], tf[plan["att_faster"]], tf[plan["pcm16"]]
    prof = ", PcWithProfiles" if table else ""
    ks = {"k_pc_index", "k_pc_history", "k_pc_gather4" if plan["rows4"] == "1" else "k_pc_gather"}
    ma = plan["ma"]
    if ma == "MA2_CMW":
        ks.add("k_pc_ma2<true, true>")
    elif ma == "MA2":
        ks.add(f"k_pc_ma2<{own}>" + (" DIRECT" if plan["direct"] == "1" else ""))
    elif ma == "MAD":
        ks.add(f"k_pc_mad<{own}>")
    else:
        pow2 = tf[str(int(ma == "MA_POW2"))]
        ks |= {f"k_pc_ma<false, {pow2}>", f"k_pc_ma<true, {pow2}>"}
    if plan["agc"] == PF.ONE:
        ks |= {"k_pc_cm", "k_pc_cscan", "k_pc_zero", f"k_pc_agc<{att}, {p16}{prof}> h={plan['h']}"}
    else:
        if plan["nsub"] != "1":
            ks.add("k_pc_submax")
        ks |= {"k_pc_prefix", "k_pc_want_prof" if table else "k_pc_want", f"k_pc_gain<{att}, {own}{prof}>",
               "k_pc_out4" if plan["rows4"] == "1" else "k_pc_out"}
    return {f"{k} lanes={plan['lanes']}" if k.startswith(("k_pc_ma", "k_pc_gain", "k_pc_agc")) else k for k in ks}


# ---- the rules ---------------------------------------------------------------------------------------------------------------
def rules(name):
    """the rules of the module text as a list of the ones the case breaks"""
    case = CASES[name]
    slots, st, nb = PF.slots_of(case), starts(case), len(case.batches)
    n, h, L, D = len(slots), case.n // 2, case.rate // 5, case.rate // 750 * 2
    ft, al = features(case), alive(name)
    wg = [work_group(case, s) for s in slots]
    first = [PF.start_frame(case, s) for s in slots]
    broken = []

    def there(k, b):   # has client k a (possibly empty) stream in batch b
        return first[k] <= st[b] and not paused(case, k, b)

    def row(k, b):
        return al[k, st[b]:st[b + 1]]
    if nb < 3 or not any(b < case.max_batch for b in case.batches) or max(case.batches) != case.max_batch:
        broken.append("the batch list: at least three, one shorter than max_batch, one of max_batch, none longer")
    if not any(there(k, b) and not row(k, b)[0] for k in range(n) for b in range(nb)):
        broken.append("no batch whose first frame is dropped")
    if not any(there(k, b) and not row(k, b)[-1] for k in range(n) for b in range(nb)):
        broken.append("no batch whose last frame is dropped")
    empty = [(k, b) for k in range(n) for b in range(nb) if there(k, b) and not row(k, b).any()
             and any(j != k and wg[j] == wg[k] and there(j, b) and row(j, b).all() for j in range(n))]
    if not empty:
        broken.append("no client with every frame of a batch dropped beside one of its work-group that keeps all")
    never_paused = [k for k, _ in empty if k not in ft.profiles]
    if not never_paused or all(k in [e for e, _ in empty] for k in ft.profiles):
        broken.append("no all-dropped client that is never paused, or no paused client that is never all-dropped")
    level = 0
    for b in range(nb):
        counts = {}
        for k in range(n):
            if there(k, b):
                counts.setdefault(wg[k], set()).add(int(row(k, b).sum()))
        level += not any(len(c) > 1 for c in counts.values())
    if level > 1:
        broken.append(f"{level} batches in which no work-group has two clients with different surviving counts")
    if case.max_batch > 64:
        def blocks(r):
            return [r[m:m + 64] for m in range(0, len(r), 64)]
        if not any(there(k, b) and len(row(k, b)) > 192 and all(c.any() and not c.all() for c in blocks(row(k, b)))
                   and all(row(k, b)[m - 1] and row(k, b)[m] for m in range(64, len(row(k, b)), 64)) for k in range(n) for b in range(nb)):
            broken.append("no batch with drops and survivors in every block of 64 frames and survivors on both sides of 64, 128, 192")
    if h % 16 and not any((int(al[k, :st[b + 1]].sum()) * h) % 16 for k in range(n) for b in range(nb)):
        broken.append("no batch behind which a stream ends inside a 16-sample chunk")
    pauses = [(k, [b for b in range(nb) if paused(case, k, b)]) for k in range(n)]
    if not any(len(bs) == 1 and 0 < bs[0] < nb - 1 for _, bs in pauses):
        broken.append("no client paused for exactly one batch in mid-run")
    if any(has_table(case, b) == (b == PAUSE) for b in range(nb)):
        broken.append("the profile table travels with every batch but the paused one")
    if case.late is not None:
        k = slots.index(case.late)
        if first[k] != st[LATE_BATCH] or al[k, first[k]]:
            broken.append("the late client's first batch does not start with a dropped frame")
    if case.plan.get("direct") == 1 and len(set(wg)) > 1:
        def whole(g, b):
            return all(there(k, b) and row(k, b).all() for k in range(n) if wg[k] == g)
        if not any(whole(g, b) and any(wg[k] != g and there(k, b) and not row(k, b).all() for k in range(n)) for g in set(wg) for b in range(nb)
                   if case.batches[b] * h >= D):
            broken.append("no batch with one work-group whole (DIRECT) and a drop in another")
    if not any(there(k, PAUSE) and 0 < row(k, PAUSE).sum() < case.batches[PAUSE] for k in range(n)):
        broken.append("no partial stream in the paused batch")
    # the features: one of each, with more than 64 slots one of each in a slot of 64 or above
    placed = [("filter", ft.filter), ("squelch", ft.squelch)] + [(profile_kind(case, k), k) for k in ft.profiles]
    for what in ("filter", "squelch", "expressible", "capped", "manual"):
        ks = [k for w, k in placed if w == what]
        if not ks or (case.slots > 64 and not any(slots[k] >= 64 for k in ks)):
            broken.append(f"no {what} client" + (" in a slot of 64 or above" if ks else ""))
    if ft.twin == ft.filter or client_spec(case, ft.twin) != client_spec(case, ft.filter) or client_spec(case, ft.filter)[0] == "IQ":
        broken.append("the filter client has no twin")
    if MANUAL["manual_gain"] == 0 or CAPPED["max_gain"] == 0 or EXPRESSIBLE["manual"] or EXPRESSIBLE["max_gain"] != 0:
        broken.append("the profiles are not what their names say")
    # the squelch client: the oracle's pwr keeps its distance from both thresholds, the expected flags open and close
    o_db, c_db, _, _ = squelch_params(case)
    pwr, key = oracle_run(name)[ft.squelch][1], squelch_key(case)
    ok = al[ft.squelch]
    with np.errstate(all="ignore"):
        db = 10 * np.log10(pwr.astype(np.float64))
    if (db[ok & (key == 1)] < o_db + SQ_SPARE_DB).any() or (db[ok & (key == 0)] > c_db - SQ_SPARE_DB).any():
        broken.append("the squelch client's levels come within %g dB of a threshold" % SQ_SPARE_DB)
    flags, _ = squelch_flags(case, pwr[present(name)[ft.squelch]])
    d = np.diff(flags)
    if not (d > 0).any() or not (d < 0).any():
        broken.append("the squelch client's expected flags hold no opening or no closing")
    # the caps, on what the chain hears: alive & open & not paused
    opened = np.ones(al.shape[1], bool)
    opened[present(name)[ft.squelch]] = flags == 1
    keep = keep_mask(name, opened)
    for k in range(n):
        mine = al[k, first[k]:]
        if 2 * int((~mine).sum()) > mine.size:
            broken.append(f"client {k} loses more than half of its frames")
        have = int(keep[k].sum()) * h
        if have < L + D + 4 * h:
            broken.append(f"client {k}: a surviving stream of {have} samples, needs {L + D + 4 * h}")
    return broken


def mismatch(name, k, batch, want, got):
    """the first differing sample of a client's kept rows of a batch, by where it lies in the batch and in the client's stream"""
    case = CASES[name]
    h = case.n // 2
    i = int(np.nonzero(want != got)[0][0])
    return (f"{name} client {k} ({client_spec(case, k)[0]}) slot {PF.slots_of(case)[k]} batch {batch}: kept frame {i // h} of the batch, sample {i % h}: "
            f"want {int(want[i])}, got {int(got[i])} ({int(np.count_nonzero(want != got))} of {want.size} kept samples of the batch differ)")

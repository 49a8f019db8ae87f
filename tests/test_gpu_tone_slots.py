"""The tone decoder at high and sparse slots, and in a reused high slot (the layout: tests/audio_rows_shapes.py).

A context of 600 slots with the post chain on: every slot is filled, then all but (0, 1, 63, 64, 255, 256, 598, 599) are removed -
tests/test_gpu_audio_rows_slots.py's way of making holes - so the batch's table index is not the slot.  Each neighbouring pair
holds a tone client and its twin without the decoder, with the same window; which of the two comes first changes from pair to
pair, so a stride over the state, the history ring, the records or the drop flags that is off by one slot lands on a twin.  In
front of the second batch slot 599's client is removed and a new one takes the slot - the reused slot, a high one - and one more
client goes into slot 597 through the holes below it.

  slot   0  records only (gate = 0)          slot   1  twin
  slot  63  twin                             slot  64  gated, want = 12: opens and closes
  slot 255  gated, want = 13: stays shut     slot 256  twin
  slot 598  twin                             slot 599  gated, want = 12, with a level squelch; then its next occupant, gated, any tone
  slot 597  (late) gated, want = 12

Expected, without a tolerance: a tone client's records are tests/tone_model.py's on its own rows and NaN flags since its start; its
PCM rows are the oracle's chain fed the frames that are not dropped (nan | !squelch_open | !tone_open); a twin's rows, pwr and flags
are its neighbour's and its PCM the oracle's over every frame that is not NaN; and every reading equals, byte for byte, what the
same clients give in a dense context of 9 slots on the same stream and batches."""
import functools

import numpy as np
import pytest

import audio_rows_shapes as S
from helpers import assert_same_bits, read_client, row_names
from test_gpu_squelch import oracle_pcm
from test_gpu_tone_decoder import KEY_OFF, NF, SQ, TONE, WINDOW, TCtx, cat, model, rec_of

pytestmark = pytest.mark.gpu

BATCHES = (40, 40, 40)
CHANGE_BATCH = 1   # in front of it: the reused slot's new occupant and the late client
REUSED = S.KEPT[-1]
# per kept slot: the decoder's configuration (None: a twin) and the level squelch
ROLES = ((dict(gate=0, hang_blocks=2), None), (None, None), (None, None), (dict(want=12, gate=1, hang_blocks=2), None),
         (dict(want=13, gate=1), None), (None, None), (None, None), (dict(want=12, gate=1, hang_blocks=0), SQ))
LATE_ROLE = (dict(want=12, gate=1, hang_blocks=2), None)
REUSE_ROLE = (dict(gate=1, hang_blocks=2), None)
PAIRS = ((0, 1), (3, 2), (4, 5), (7, 6))  # (tone client, twin) as indices into the kept slots


def configure(g, role):
    tone, squelch = role
    g.set_audio_range(*WINDOW)
    if squelch is not None:
        g.set_squelch(True, *squelch)
    if tone is not None:
        g.set_tone_decoder(True, **tone)
    return g


def model_cfg(tone):
    return dict(want=tone.get("want", -1), gate=tone.get("gate", 1), hang=tone.get("hang_blocks"))


@functools.lru_cache(maxsize=None)
def run(n, sparse):
    """-> {name: dict(slot, role, first frame, read=(rows, pwr, flags, pcm), squelch, tone=(tone, level, open) or None)}; names: the
    kept slots' indices 0..7 (7: slot 599's first occupant), "late", "reuse" """
    from phantomsdr_amd import AudioClient
    nslots = S.SLOTS if sparse else len(S.KEPT) + 1
    kept = S.KEPT if sparse else tuple(range(len(S.KEPT)))
    late_slot, reused = (S.LATE_SLOT, REUSED) if sparse else (len(S.KEPT), len(S.KEPT) - 1)
    A = TCtx(n, nslots, maxb=max(BATCHES), post=True)
    try:
        everyone = [AudioClient(A.ctx) for _ in range(nslots if sparse else len(kept))]
        assert [g.id for g in everyone] == list(range(len(everyone)))
        for g in everyone:
            if g.id not in kept:
                g.on_close()
        live = {i: (configure(everyone[s], ROLES[i]), ROLES[i], 0) for i, s in enumerate(kept)}
        out = {}
        at = 0
        for b, F in enumerate(BATCHES):
            if b == CHANGE_BATCH:
                live.pop(len(kept) - 1)[0].on_close()
                fillers, found = [], {}
                while len(found) < 2:
                    g = AudioClient(A.ctx)
                    if g.id == late_slot:
                        found["late"] = (configure(g, LATE_ROLE), LATE_ROLE, at)
                    elif g.id == reused:
                        found["reuse"] = (configure(g, REUSE_ROLE), REUSE_ROLE, at)
                    else:
                        assert sparse and g.id < late_slot and g.id not in kept, g.id
                        fillers.append(g)
                for f in fillers:
                    f.on_close()
                live.update(found)
            A.batch(F)
            for name, (g, role, first) in live.items():
                o = out.setdefault(name, dict(slot=g.id, role=role, first=first, read=[], squelch=[], tone=[]))
                o["read"].append(read_client(g, "USB", F, pcm=True)), o["squelch"].append((g.read_squelch(F),))
                if role[0] is not None:
                    o["tone"].append(g.read_tone(F))
            at += F
        for o in out.values():
            o["read"], o["squelch"], o["tone"] = cat(o["read"]), cat(o["squelch"])[0], (cat(o["tone"]) if o["tone"] else None)
        return out
    finally:
        A.close()


@pytest.mark.parametrize("n", (360, 512))
def test_sparse_high_slots_give_the_models_records_and_the_oracles_chain(n):
    res = run(n, True)
    h = n // 2
    assert [res[i]["slot"] for i in range(8)] == list(S.KEPT) and res["late"]["slot"] == S.LATE_SLOT and res["reuse"]["slot"] == REUSED
    assert res[7]["first"] == 0 and len(res[7]["squelch"]) == BATCHES[0] and res["reuse"]["first"] == BATCHES[0] == res["late"]["first"]
    for name, r in res.items():
        rows, _, nan, pcm = r["read"]
        tone, squelch = r["role"]
        keep = (nan == 0) & (r["squelch"] == 1)
        if tone is not None:
            want = model(rows, nan, h, **model_cfg(tone))
            got = rec_of(r["tone"])
            bad = [f for f in range(len(got)) if got[f].tobytes() != want[f].tobytes()]
            assert not bad, (n, name, r["slot"], bad[:8], got[bad[:3]], want[bad[:3]])
            print(f"n {n} slot {r['slot']} ({name}): tone {got['tone'].tolist()} open {got['open'].tolist()}")
            if tone.get("gate", 1):
                keep &= got["open"] == 1
        assert squelch is None or (r["squelch"] == 0).any()
        assert np.array_equal(pcm, oracle_pcm(rows, keep, h)) and not pcm[~keep].any(), (n, name, r["slot"])
    for a, b in PAIRS:  # a twin's rows, pwr and NaN flags are its neighbour's (slot 599's first occupant: over its one batch)
        nf = len(res[a]["squelch"])
        assert_same_bits(res[a]["read"][:3], tuple(v[:nf] for v in res[b]["read"][:3]), f"slots {res[a]['slot']} and {res[b]['slot']}", row_names("USB"))
    assert_same_bits(res[0]["read"], res[1]["read"], "gate = 0 and its twin", row_names("USB", pcm=True))
    # what the stream holds at these slots: an opening and a closing at 64, shut throughout at 255, an opening in 599's first batch,
    # and from zero at frame 40 - the carrier ends at 70 - an opening and a closing in the late and the reused slot
    op = res[3]["tone"][2]
    assert op[0] == 0 and op[KEY_OFF - 1] == 1 and op[-1] == 0 and (res[3]["tone"][0][40:KEY_OFF] == TONE).all()
    assert not res[4]["tone"][2].any() and not res[4]["read"][3].any() and res[4]["tone"][1].max() > 0
    assert res[7]["tone"][2][0] == 0 and res[7]["tone"][2][-1] == 1
    for name in ("late", "reuse"):
        t, _, op = res[name]["tone"]
        assert len(op) == NF - BATCHES[0] and (t[:18] == -1).all() and not op[:18].any() and op.any() and op[-1] == 0 and (t == TONE).any(), name
        assert res[name]["read"][3].any()


@pytest.mark.parametrize("n", (360, 512))
def test_sparse_slots_read_what_a_dense_context_does(n):
    sparse, dense = run(n, True), run(n, False)
    assert sorted(map(str, sparse)) == sorted(map(str, dense)) and [dense[i]["slot"] for i in range(8)] == list(range(8))
    assert dense["late"]["slot"] == 8 and dense["reuse"]["slot"] == 7
    for name in sparse:
        a, b = sparse[name], dense[name]
        tag = f"n {n} slot {a['slot']} ({name})"
        assert_same_bits(a["read"], b["read"], tag, row_names("USB", pcm=True))
        assert np.array_equal(a["squelch"], b["squelch"]), tag
        if a["tone"] is not None:
            assert_same_bits(a["tone"], b["tone"], tag, ("tone", "level", "open"))

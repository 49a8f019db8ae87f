"""The CW decoder at high and sparse slots, and in a reused high slot (the layout: tests/audio_rows_shapes.py).

A context of 600 slots: every slot is filled, then all but (0, 1, 63, 64, 255, 256, 598, 599) are removed - tests/test_gpu_tone_slots.py's
way of making holes - so the batch's table index is not the slot.  Each neighbouring pair holds a CW client and a twin without the
decoder, with the same window; which of the two comes first changes from pair to pair, so a stride over the state, the text ring or
the records that is off by one slot lands on a twin.  In front of the second batch slot 599's client is removed and a new one takes
the slot - the reused slot, a high one - and one more client goes into slot 597 through the holes below it.

  slot   0  CW, default speed                slot   1  twin
  slot  63  twin                             slot  64  CW and a tone decoder on the same client
  slot 255  CW, search_hz 0, no tracking     slot 256  twin
  slot 598  twin                             slot 599  CW; then its next occupant, CW
  slot 597  (late) CW

Expected, without a tolerance: a CW client's records and text are tests/cw_model.py's on its own rows and NaN flags since its start;
a twin's rows, pwr and flags are its neighbour's; the tone decoder's records beside the CW decoder are tests/tone_model.py's."""
import functools

import numpy as np
import pytest

import audio_rows_shapes as S
import tone_model as TM
from helpers import assert_same_bits, read_client, row_names
from test_gpu_cw_decoder import CFG, NF, RATE, TEXT, WINDOW, CCtx, cat, model, rec_of

pytestmark = pytest.mark.gpu

CHANGE_BATCH = 1   # in front of it: the reused slot's new occupant and the late client
REUSED = S.KEPT[-1]
TONE = dict(gate=0, hang_blocks=2)
# per kept slot: the CW decoder's configuration (None: a twin) and the tone decoder's
ROLES = ((dict(), None), (None, None), (None, None), (CFG, TONE), (dict(CFG, search_hz=0.0, track_speed=0), None), (None, None), (None, None),
         (CFG, None))
LATE_ROLE = (CFG, None)
REUSE_ROLE = (dict(CFG, snr_db=18.0), None)
PAIRS = ((0, 1), (3, 2), (4, 5), (7, 6))  # (CW client, twin) as indices into the kept slots


def configure(g, role):
    cw, tone = role
    g.set_audio_range(*WINDOW)
    if cw is not None:
        g.set_cw_decoder(True, **cw)
    if tone is not None:
        g.set_tone_decoder(True, **tone)
    return g


@functools.lru_cache(maxsize=None)
def run(n):
    """-> {name: dict(slot, role, first frame, read=(rows, pwr, flags), cw=(records) or None, text, tone)}; names: the kept slots'
    indices 0..7 (7: slot 599's first occupant), "late", "reuse" """
    from phantomsdr_amd import AudioClient
    batches = (NF[n] // 3,) * 3
    A = CCtx(n, S.SLOTS, maxb=max(batches))
    try:
        everyone = [AudioClient(A.ctx) for _ in range(S.SLOTS)]
        assert [g.id for g in everyone] == list(range(S.SLOTS))
        for g in everyone:
            if g.id not in S.KEPT:
                g.on_close()
        live = {i: (configure(everyone[s], ROLES[i]), ROLES[i], 0) for i, s in enumerate(S.KEPT)}
        out = {}
        at = 0
        for b, F in enumerate(batches):
            if b == CHANGE_BATCH:
                live.pop(len(S.KEPT) - 1)[0].on_close()
                fillers, found = [], {}
                while len(found) < 2:
                    g = AudioClient(A.ctx)
                    if g.id == S.LATE_SLOT:
                        found["late"] = (configure(g, LATE_ROLE), LATE_ROLE, at)
                    elif g.id == REUSED:
                        found["reuse"] = (configure(g, REUSE_ROLE), REUSE_ROLE, at)
                    else:
                        assert g.id < S.LATE_SLOT and g.id not in S.KEPT, g.id
                        fillers.append(g)
                for f in fillers:
                    f.on_close()
                live.update(found)
            A.batch(F)
            for name, (g, role, first) in live.items():
                o = out.setdefault(name, dict(slot=g.id, role=role, first=first, read=[], cw=[], tone=[], text=None))
                o["read"].append(read_client(g, "USB", F))
                if role[0] is not None:
                    o["cw"].append(g.read_cw(F))
                    o["text"] = g.read_cw_text()
                if role[1] is not None:
                    o["tone"].append(g.read_tone(F))
            at += F
        for o in out.values():
            o["read"], o["cw"], o["tone"] = cat(o["read"]), (cat(o["cw"]) if o["cw"] else None), (cat(o["tone"]) if o["tone"] else None)
        return out
    finally:
        A.close()


@pytest.mark.parametrize("n", (360, 512))
def test_sparse_high_slots_give_the_models_records_and_text(n):
    res = run(n)
    h = n // 2
    assert [res[i]["slot"] for i in range(8)] == list(S.KEPT) and res["late"]["slot"] == S.LATE_SLOT and res["reuse"]["slot"] == REUSED
    assert res[7]["first"] == 0 and len(res[7]["read"][0]) == NF[n] // 3 and res["reuse"]["first"] == NF[n] // 3 == res["late"]["first"]
    for name, r in res.items():
        rows, _, nan = r["read"]
        cw, tone = r["role"]
        if cw is not None:
            want, wtext = model(rows, nan, h, **cw)
            got = rec_of(r["cw"])
            bad = [f for f in range(len(got)) if got[f].tobytes() != want[f].tobytes()]
            assert not bad, (n, name, r["slot"], bad[:8], got[bad[:3]], want[bad[:3]])
            assert r["text"] == (wtext, len(wtext)), (n, name, r["slot"], r["text"], wtext)
            print(f"n {n} slot {r['slot']} ({name}): text {wtext!r} wpm {got['wpm'][-1]:.2f} pitch {got['pitch_hz'][-1]}")
        if tone is not None:
            t = np.zeros(len(rows), TM.REC_DTYPE)
            t["tone"], t["level"], t["open"] = r["tone"]
            assert t.tobytes() == TM.records(rows, nan, h, RATE, gate=0, hang=2).tobytes(), (n, name)
    for a, b in PAIRS:  # a twin's rows, pwr and NaN flags are its neighbour's (slot 599's first occupant: over its one batch)
        nf = len(res[a]["read"][0])
        assert_same_bits(res[a]["read"], tuple(v[:nf] for v in res[b]["read"]), f"slots {res[a]['slot']} and {res[b]['slot']}", row_names("USB"))
    # what the stream holds at these slots: the whole text where the decoder ran from the start, its end where it started late
    for i in (0, 3, 4):
        assert res[i]["text"] == (TEXT, len(TEXT)), (i, res[i]["text"])
    assert rec_of(res[4]["cw"])["wpm"].max() == rec_of(res[4]["cw"])["wpm"][-1] == 25.0  # no tracking: u never moves
    for name in ("late", "reuse"):
        assert res[name]["text"][0].endswith("DE K"), (name, res[name]["text"])  # (`DE` begins 0.4 s behind the late clients' full ring)

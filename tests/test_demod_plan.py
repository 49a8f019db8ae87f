"""The demodulation batch's plan (phantomsdr_amd/csrc/demodplan.h demod_plan) without a GPU and without the library:
tests/demod_plan_table.cpp is compiled with the host C++ compiler - the header is plain C++17 - and runs the scripts below.
For a set of audio slots this is the one place that says who is demodulated in a batch, in which list of the parameter-ring
slot, and which carried state starts from zero.  Every expectation here is written from the rules, and the
whole output is held against the hash of what the list-building code printed before it became demod_plan."""
import hashlib
import json
import math
import os
import subprocess

import pytest

from conftest import ROOT

USB, LSB, AM, FM, IQ, SAM = range(6)
BOTH, UPPER, LOWER = range(3)
CP, SIDE, INT, NOTCH = 32, 16, 4, 16  # sizeof ClientParams, FtClient / SbClient, int, int4
# tests/helpers.py CLIENT_KINDS as (mode, fine, sideband)
KINDS = {"USB": (USB, 0, BOTH), "LSB": (LSB, 0, BOTH), "AM": (AM, 0, BOTH), "FM": (FM, 0, BOTH), "SAM": (SAM, 0, BOTH), "IQ": (IQ, 0, BOTH),
         "TUSB": (USB, 1, BOTH), "TLSB": (LSB, 1, BOTH), "TIQ": (IQ, 1, BOTH), "SAMU": (SAM, 0, UPPER), "SAML": (SAM, 0, LOWER)}


def kind(i, name):
    return "kind %d %d %d %d" % ((i,) + KINDS[name])


def client(i, name, l=10, mid=15.25, r=20):
    return ["add %d" % i, kind(i, name), "window %d %d %r %d" % (i, l, mid, r)]


def ft_off(S):
    return (S * (CP + INT) + 15) & ~15


def notch_off(S):
    return (ft_off(S) + S * (CP + SIDE) + 15) & ~15


def ring_bytes(S):
    return notch_off(S) + S * (NOTCH + CP)


# ---- the scripts: (name, lines); every `batch` of a case is numbered from 0
SCRIPTS = []


def script(name, *parts):
    lines = ["case " + name]
    for p in parts:
        lines += [p] if isinstance(p, str) else list(p)
    SCRIPTS.append((name, lines))


script("empty", "batch")
# one client of each kind, interleaved by family
ELEVEN = ["USB", "SAM", "IQ", "TUSB", "SAMU", "LSB", "TIQ", "SAML", "AM", "TLSB", "FM"]
script("kinds", "size 12 360 5", *[client(i, k, 10 + i, 15.25 + i, 22 + i) for i, k in enumerate(ELEVEN)], "batch")
script("post", "post on", client(1, "USB"), client(3, "USB"), client(4, "USB"), "batch",  # 0: three clients get a history
       kind(3, "TIQ"), kind(4, "IQ"), "pause 1", client(2, "USB"), "pause 2", client(5, "IQ"), client(6, "TIQ"), client(0, "USB"), "batch",  # 1
       "post off", kind(0, "LSB"), "batch",  # 2: the chain off
       "post on", "remove 0", "batch")  # 3: the chain on, IQ clients only
script("agc_reset", "post on", client(0, "USB"), "batch", kind(0, "LSB"), "batch", "post off", kind(0, "USB"), "batch",
       "post on", client(1, "IQ"), kind(0, "IQ"), "batch")
script("carrier", client(2, "USB"), "batch", kind(2, "SAM"), "batch", kind(2, "SAMU"), "batch", kind(2, "SAML"), "batch", kind(2, "SAM"), "batch",
       kind(2, "USB"), "batch", kind(2, "SAM"), "batch", "pause 2", "batch", "resume 2", "batch")
script("tuned_tail", client(3, "TUSB"), "batch", "batch", kind(3, "TLSB"), "batch", kind(3, "LSB"), "batch", kind(3, "TLSB"), "batch",
       "pause 3", "batch", "resume 3", "batch")
PLACED = ["TUSB", "SAMU", "TLSB", "SAML"]
script("placed", *[client(i, k) for i, k in enumerate(PLACED)],
       *[["window %d 10 %r 20" % (i, m) for i in range(4)] + ["batch"] for m in (5.5, 15.5, 25.5)])
FRACTIONS = (0.37, 0.5, 0.999)
script("phase", *[client(i, "TUSB", 10, 12 + fr, 20) for i, fr in enumerate(FRACTIONS)], "batch", "batch", "batch")
script("manual_notch", client(0, "USB"), client(1, "IQ"), client(2, "TIQ"), client(3, "USB"), "notch 0 0 3 5", "batch",
       "notch 1 1 7 9", "batch", "notch 1 1 0 0", "notch 2 0 1 2", "batch", "auto 1 1", "batch")
script("detector", client(0, "USB"), client(1, "USB"), client(2, "USB"), "auto 2 1", "auto 0 1", "batch", "batch",  # 0 on, 1 unchanged
       "window 0 10 15.25 21", "batch", "window 2 10 16.0 20", "batch", kind(0, "AM"), "batch",  # 2 window, 3 floor(mid), 4 mode
       "auto 0 0", "batch", "batch", "pause 2", "auto 2 0", "auto 2 1", "resume 2", "batch",  # 5 off, 6 unchanged, 7 off and on while paused
       "tab off", "batch")  # 8 no detector state
script("band", client(0, "USB"), "band 10 10", "batch", "band 11 10", "batch", "band 10 9", "batch",
       client(1, "USB", 50, 50.0, 50), client(2, "USB", 100, 105.0, 110), "pause 2", "band 10 10", "batch")
script("seeded", "size 16 360 5", "seeded 12345 200")


def parse(stdout):
    """-> {case: [batch]}, a batch: dict of its header, plan, off, copies, zero (dicts) and pre, cl, ft, sbl, nt, det, post (lists of dicts)"""
    cases, cur = {}, None
    for ln in stdout.splitlines():
        tag, *kvs = ln.split()
        d = dict(kv.split("=", 1) for kv in kvs)
        if tag == "case":
            cur = cases.setdefault(d["name"], [])
        elif tag == "batch":
            cur.append(dict(hdr=d, pre=[], cl=[], ft=[], sbl=[], nt=[], det=[], post=[], pre_lines=[], post_lines=[]))
        elif tag in ("plan", "off", "copies", "zero", "ci"):
            cur[-1][tag] = d
        else:
            cur[-1][tag].append(d)
            if tag in ("pre", "post"):
                cur[-1][tag + "_lines"].append(ln.split(None, 1)[1])
    return cases


def build(tmp, name, extra=()):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(ROOT, "phantomsdr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "demod_plan_table.cpp"), "-o", exe])
    return exe


INPUT = "\n".join(ln for _, lines in SCRIPTS for ln in lines) + "\n"


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("demod_plan")


@pytest.fixture(scope="module")
def stdout(tmp):
    r = subprocess.run([build(tmp, "demod_plan_table")], input=INPUT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def cases(stdout):
    return parse(stdout)


def ints(s):
    return [int(v) for v in s.split(",")] if s else []


def counts(b):
    return {k: int(b["plan"][k]) for k in ("nold", "nsam", "ntssb", "ntiq", "nsb", "niq", "nact", "npaused", "ndet", "iq_off")}


def slots_of(entries):
    return [int(e["slot"]) for e in entries]


def copies(b):
    return [tuple(int(v) for v in c.split(":")) for c in b["copies"]["list"].split(",")] if b["copies"]["list"] else []


def zeros(b):
    return {k: ints(v) for k, v in b["zero"].items()}


NOTHING = dict(car=[], ft=[], sb=[], det=[])


def test_empty_context(cases):
    (b,) = cases["empty"]
    assert b["plan"]["verdict"] == "OK" and b["plan"]["seq"] == "1" and b["hdr"]["seq"] == "0"  # (advanced before anybody is counted)
    assert set(counts(b).values()) == {0}
    assert copies(b) == [] and zeros(b) == NOTHING and b["cl"] == [] and b["plan"]["idle"] == "1"


def test_one_client_of_each_kind(cases):
    (b,) = cases["kinds"]
    S, h = 12, 180
    where = {k: i for i, k in enumerate(ELEVEN)}
    plain, sam, tssb, sb = [where[k] for k in ("USB", "LSB", "AM", "FM")], [where["SAM"]], [where["TUSB"], where["TLSB"]], [where["SAMU"], where["SAML"]]
    assert plain == sorted(plain) and tssb == sorted(tssb) and sb == sorted(sb)  # (slot order within a list)
    assert counts(b) == dict(nold=4, nsam=1, ntssb=2, ntiq=1, nsb=2, niq=1, nact=9, npaused=0, ndet=0, iq_off=9)
    assert slots_of(b["cl"]) == plain + sam + tssb + sb + [where["IQ"]]
    assert slots_of(b["ft"]) == tssb + [where["TIQ"]] and slots_of(b["sbl"]) == sb
    assert [int(e["paused"]) for e in b["cl"]] == [0] * 9 + [1]  # (to the post chain an IQ client is a paused one)
    assert [int(e["mode"]) for e in b["cl"]] == [USB, LSB, AM, FM, SAM, USB, LSB, SAM, SAM, IQ]
    f, n = ft_off(S), notch_off(S)
    assert (f, n, ring_bytes(S)) == (432, 1008, 1584) and int(b["plan"]["ring_bytes"]) == 1584
    assert b["off"] == dict(plain="0,0", sam="%d,0" % (4 * CP), iq="%d,0" % (9 * CP), tssb="%d,%d" % (f, f + 3 * CP), tiq="%d,%d" % (f + 2 * CP, f + 3 * CP + 2 * SIDE),
                            sb="%d,%d" % (f + 3 * (CP + SIDE), f + 3 * (CP + SIDE) + 2 * CP), det="%d,0" % (n + S * NOTCH), slot_ci=str(S * CP), notch=str(n))
    assert copies(b) == [(0, 10 * CP), (f, 3 * (CP + SIDE)), (f + 3 * (CP + SIDE), 2 * (CP + SIDE))]
    # every fresh SAM client of either kind starts its carrier tail from zero, every tuned USB / LSB and sideband client its own
    assert zeros(b) == dict(car=[s * h for s in sorted(sam + sb)], ft=[s * h for s in tssb], sb=[s * h for s in sb], det=[])
    for e in b["cl"]:
        s = int(e["slot"])
        assert (int(e["l"]), int(e["r"]), int(e["m"]), int(e["cur"]), int(e["agc"])) == (10 + s, 22 + s, 15 + s, 0, 0)
    assert all(p["cur"] == "1" for p in b["post"][:11]) and b["post"][11] == b["pre"][11]


def test_post_chain_on_off_and_iq_only(cases):
    b0, b1, b2, b3 = cases["post"]
    S = 8
    assert slots_of(b0["cl"]) == [1, 3, 4] and [e["agc"] for e in b0["cl"]] == ["2"] * 3 and b0["ci"]["list"] == "-1,0,-1,1,2,-1,-1,-1"
    # 1, the chain on: slot 0 audio; 1 paused with a history; 2 paused and fresh; 3 tuned IQ with a history; 4 IQ with a history;
    # 5 IQ, fresh; 6 tuned IQ, fresh
    assert counts(b1) == dict(nold=1, nsam=0, ntssb=0, ntiq=2, nsb=0, niq=2, nact=1, npaused=3, ndet=0, iq_off=3)
    assert slots_of(b1["cl"]) == [0, 1, 3, 4, 5] and [e["paused"] for e in b1["cl"]] == ["0", "1", "1", "1", "1"]
    assert slots_of(b1["ft"]) == [3, 6] and [e["paused"] for e in b1["ft"]] == ["1", "1"]
    same = ("l", "r", "m", "slot", "cur", "agc", "paused")
    assert {k: b1["cl"][2][k] for k in same} == {k: b1["ft"][0][k] for k in same} and b1["cl"][2]["mode"] == str(IQ)  # a paused copy
    assert b1["cl"][1] == dict(k="1", l="0", r="0", m="0", mode="0", slot="1", cur=b1["pre"][1]["cur"], agc="0", paused="1")  # (an empty stream)
    ci = ints(b1["ci"]["list"])
    assert ci == [0, 1, -1, 2, 3, -1, -1, -1]
    assert all(ci[int(e["slot"])] == k for k, e in enumerate(b1["cl"][:4]))  # the inverse of the list, -1 elsewhere
    assert copies(b1)[0] == (0, S * (CP + INT)) and b1["off"]["iq"] == "%d,0" % (3 * CP)
    assert b1["cl"][0]["agc"] == "2" and b1["post"][0]["agc"] == "0"  # (a fresh audio client: 2 goes into the list entry)
    assert [b1["post"][i]["agc"] for i in (1, 2, 3, 4, 5, 6)] == ["0", "2", "1", "1", "2", "2"]  # (kept: paused, IQ)
    assert b1["pre_lines"][1] == b1["post_lines"][1] and b1["pre_lines"][2] == b1["post_lines"][2]
    # 2, the chain off: nobody is listed for it
    assert counts(b2) == dict(nold=1, nsam=0, ntssb=0, ntiq=2, nsb=0, niq=2, nact=1, npaused=0, ndet=0, iq_off=1)
    assert slots_of(b2["cl"]) == [0, 4, 5] and "ci" not in b2 and copies(b2)[0] == (0, (1 + 2) * CP)
    assert b2["pre"][0]["agc"] == "1" and b2["cl"][0]["agc"] == "0" and b2["post"][0]["agc"] == "1"  # (kept with the chain off)
    # 3, the chain on and no audio client: the paused clients and the IQ clients' histories are not listed
    assert counts(b3) == dict(nold=0, nsam=0, ntssb=0, ntiq=2, nsb=0, niq=2, nact=0, npaused=0, ndet=0, iq_off=0)
    assert slots_of(b3["cl"]) == [4, 5] and slots_of(b3["ft"]) == [3, 6] and ints(b3["ci"]["list"]) == [-1] * S
    assert copies(b3)[0] == (0, S * (CP + INT))


def test_agc_reset(cases):
    b0, b1, b2, b3 = cases["agc_reset"]
    assert (b0["pre"][0]["agc"], b0["cl"][0]["agc"], b0["post"][0]["agc"]) == ("2", "2", "0")  # fresh, carried into the entry
    assert (b1["pre"][0]["agc"], b1["cl"][0]["agc"], b1["post"][0]["agc"]) == ("1", "1", "0")  # consumed with the chain on
    assert (b2["pre"][0]["agc"], b2["cl"][0]["agc"], b2["post"][0]["agc"]) == ("1", "0", "1")  # kept with the chain off
    assert slots_of(b3["cl"]) == [0, 1]  # two IQ clients: the one with a history first
    assert [(b3["pre"][i]["agc"], b3["cl"][k]["agc"], b3["post"][i]["agc"]) for k, i in enumerate((0, 1))] == [("1", "0", "1"), ("2", "0", "2")]


def tail(cur, slot, S=8, h=180):
    return (cur * S + slot) * h


def test_sam_tails_continue_or_start_from_zero(cases):
    b = cases["carrier"]
    curs = [int(x["pre"][2]["cur"]) for x in b]
    assert curs == [0, 1, 0, 1, 0, 1, 0, 1, 1]  # (flipped by every batch the slot takes part in)
    want = [NOTHING,  # USB
            dict(NOTHING, car=[tail(1, 2)]),  # USB -> SAM
            dict(NOTHING, sb=[tail(0, 2)]),  # SAM -> SAM-U: the carrier tail goes on
            dict(NOTHING, sb=[tail(1, 2)]),  # SAM-U -> SAM-L
            NOTHING,  # SAM-L -> SAM
            NOTHING,  # SAM -> USB
            dict(NOTHING, car=[tail(0, 2)]),  # USB -> SAM again
            NOTHING,  # paused
            NOTHING]  # ... and back: the pause interrupts nothing
    assert [zeros(x) for x in b] == want
    assert b[7]["pre_lines"][2] == b[7]["post_lines"][2] and b[7]["plan"]["idle"] == "1"


def test_tuned_tail_continues_or_starts_from_zero(cases):
    b = cases["tuned_tail"]
    want = [dict(NOTHING, ft=[tail(0, 3)]),  # a fresh tuned USB client
            NOTHING,
            dict(NOTHING, ft=[tail(0, 3)]),  # tuned USB -> tuned LSB
            NOTHING,  # -> LSB
            dict(NOTHING, ft=[tail(0, 3)]),  # -> tuned LSB again
            NOTHING,  # paused
            NOTHING]
    assert [zeros(x) for x in b] == want
    assert [x["post"][3]["b_tuned"] for x in b] == ["1", "1", "1", "0", "1", "1", "1"]


def test_placed_ranges(cases):
    upper = {5: (10, 20), 15: (15, 20), 25: (20, 20)}
    lower = {5: (10, 10), 15: (10, 16), 25: (10, 20)}
    for b, m in zip(cases["placed"], (5, 15, 25)):
        assert slots_of(b["ft"]) == [0, 2] and slots_of(b["sbl"]) == [1, 3]
        got = {int(e["slot"]): e for e in b["ft"] + b["sbl"]}
        for s, name in enumerate(PLACED):
            e = got[s]
            assert (int(e["l"]), int(e["r"])) == (upper if name in ("TUSB", "SAMU") else lower)[m], (name, m)
            assert (e["wl"], e["wr"], e["m"], e["mode"]) == ("10", "20", str(m), str(AM))
        assert [(e["side"], e["pad"]) for e in b["sbl"]] == [(str(UPPER), "0"), (str(LOWER), "0")]
        assert all((e["l"], e["r"]) == ("10", "20") for e in b["cl"])  # the batch's own list keeps the window and the mode
        assert [int(e["mode"]) for e in b["cl"]] == [USB, LSB, SAM, SAM]


def test_tuned_phase(cases):
    n, nframes = 360, 5
    phi = [0, 0, 0]
    wrapped = False
    for b in cases["phase"]:
        for i, fr in enumerate(FRACTIONS):
            mid = 12 + fr
            step = math.floor((mid - math.floor(mid)) * 2.0 ** 32 / n + 0.5)
            assert (int(b["ft"][i]["step"]), int(b["ft"][i]["phi0"])) == (step, phi[i]), (fr, b["hdr"])
            wrapped |= phi[i] + nframes * (n // 2) * step >= 2 ** 32
            phi[i] = (phi[i] + nframes * (n // 2) * step) % 2 ** 32
            assert int(b["post"][i]["phi"]) == phi[i]
    assert wrapped and all(phi)


def test_manual_notches(cases):
    b0, b1, b2, b3 = cases["manual_notch"]
    S = 8
    assert b0["plan"]["any_manual"] == "1" and b0["plan"]["iq_notched"] == "0"
    assert [e["v"] for e in b0["nt"]] == ["3,5,0,0"] + ["0,0,0,0"] * (S - 1)
    assert copies(b0)[-1] == (notch_off(S), S * NOTCH)
    assert b1["plan"]["iq_notched"] == "1" and [e["v"] for e in b1["nt"]][:2] == ["3,5,0,0", "0,0,7,9"]  # an untuned IQ client's
    assert b2["plan"]["iq_notched"] == "0" and [e["v"] for e in b2["nt"]][:3] == ["3,5,0,0", "0,0,0,0", "1,2,0,0"]  # a tuned one's is not
    assert b3["plan"]["iq_notched"] == "1" and slots_of(b3["det"]) == [1] and zeros(b3)["det"] == [1]  # an automatic one
    assert b3["post"][1]["b_notch"] == "0,0,0,0" and b3["post"][0]["b_notch"] == "3,5,0,0"


def test_detector_state(cases):
    b = cases["detector"]
    assert [slots_of(x["det"]) for x in b] == [[0, 2]] * 5 + [[2]] * 3 + [[]]  # slot order
    assert all(int(x["plan"]["ndet"]) == len(x["det"]) for x in b)
    assert [zeros(x)["det"] for x in b] == [[0, 2], [], [0], [2], [0], [0], [], [2], []]
    assert b[7]["pre"][2]["fresh"] == "1" and b[7]["post"][2]["fresh"] == "0"
    S = 8
    assert copies(b[0])[-1] == (notch_off(S) + S * NOTCH, 2 * CP) and b[0]["det"][1]["m"] == "15"
    assert len(copies(b[8])) == 1


def test_band(cases):
    b0, b1, b2, b3 = cases["band"]
    assert b0["plan"]["verdict"] == "OK" and b0["plan"]["seq"] == "1"
    for b in (b1, b2):  # one bin outside, on either side
        assert b["plan"]["verdict"] == "BAND_OUTSIDE" and b["plan"]["bad"] == "0,10,20"
        assert b["pre_lines"] == b["post_lines"] and b["plan"]["seq"] == b["hdr"]["seq"] == "1"
        assert "copies" not in b and b["cl"] == []
    # an empty window and a paused client outside the band do not count
    assert b3["plan"]["verdict"] == "OK" and slots_of(b3["cl"]) == [0, 1] and b3["plan"]["seq"] == "2"


def test_seeded_batches_keep_the_invariants(cases):
    batches = cases["seeded"]
    S, total = 16, ring_bytes(16)
    assert len(batches) == 200
    seen = set()
    for b in batches:
        live = [i for i, s in enumerate(b["pre"]) if s["active"] == "1" and s["paused"] == "0"]
        if b["plan"]["verdict"] != "OK":
            assert b["pre_lines"] == b["post_lines"] and b["plan"]["seq"] == b["hdr"]["seq"]
            seen.add("refused")
            continue
        assert int(b["plan"]["seq"]) == int(b["hdr"]["seq"]) + 1
        c = counts(b)
        cl, ft = slots_of(b["cl"]), slots_of(b["ft"])
        lists = dict(plain=cl[:c["nold"]], sam=cl[c["nold"]:c["nold"] + c["nsam"]], tssb=ft[:c["ntssb"]], tiq=ft[c["ntssb"]:], sb=slots_of(b["sbl"]),
                     iq=cl[c["iq_off"]:c["iq_off"] + c["niq"]] if c["niq"] else [])
        assert sorted(sum(lists.values(), [])) == live, b["hdr"]  # every active, unpaused slot in exactly one kernel list
        assert [len(lists[k]) for k in ("plain", "sam", "tssb", "tiq", "sb", "iq")] == [c[k] for k in ("nold", "nsam", "ntssb", "ntiq", "nsb", "niq")]
        assert c["nact"] == c["nold"] + c["nsam"] + c["ntssb"] + c["nsb"] and len(live) == c["nact"] + c["ntiq"] + c["niq"]
        assert cl[:c["nact"]] == lists["plain"] + lists["sam"] + lists["tssb"] + lists["sb"]
        assert c["ntssb"] + c["ntiq"] + c["nsb"] <= S and c["ndet"] <= S
        assert all(v == sorted(v) for v in lists.values())
        if b["hdr"]["post"] == "1":
            ci = ints(b["ci"]["list"])
            listed = c["nact"] + c["npaused"]
            assert sorted(x for x in ci if x >= 0) == list(range(listed)) and all(ci[cl[k]] == k for k in range(listed))
        else:
            assert c["npaused"] == 0
        # every offset + length inside the ring slot
        sizes = dict(plain=(c["nold"], 0), sam=(c["nsam"], 0), iq=(c["niq"], 0), tssb=(c["ntssb"], SIDE), tiq=(c["ntiq"], SIDE), sb=(c["nsb"], SIDE), det=(c["ndet"], 0))
        for name, (cnt, side) in sizes.items():
            o_cl, o_side = ints(b["off"][name])
            assert o_cl + cnt * CP <= total and o_side + cnt * side <= total
        assert int(b["off"]["slot_ci"]) + S * INT <= total and int(b["off"]["notch"]) + S * NOTCH <= total
        assert all(off + size <= total for off, size in copies(b))
        assert all(z < 2 * S * 180 for k in ("car", "ft", "sb") for z in zeros(b)[k]) and all(z < S for z in zeros(b)["det"])
        for i in range(S):
            if i in live:
                assert int(b["post"][i]["cur"]) == int(b["pre"][i]["cur"]) ^ 1 and b["post"][i]["seq"] == b["plan"]["seq"]
            else:
                assert b["pre_lines"][i] == b["post_lines"][i]  # a paused or inactive slot: no carried field moves
        seen |= {k for k, v in lists.items() if v} | {"zero " + k for k, v in zeros(b).items() if v}
        seen |= {"paused"} if c["npaused"] else set()
    assert seen == {"refused", "plain", "sam", "tssb", "tiq", "sb", "iq", "zero car", "zero ft", "zero sb", "zero det", "paused"}  # (the script reaches all of it)


def test_same_trace_as_before_the_planner(stdout):
    """the whole output - every table case and the seeded script - against what the parent's list-building code printed
    behind the same signature (tests/golden/demod_plan_trace.json): a mismatch is a change of behaviour"""
    with open(os.path.join(ROOT, "tests", "golden", "demod_plan_trace.json")) as f:
        golden = json.load(f)
    assert hashlib.sha256(INPUT.encode()).hexdigest() == golden["input_sha256"], "the scripts changed: the trace was recorded for others"
    assert hashlib.sha256(stdout.encode()).hexdigest() == golden["output_sha256"]


def test_sanitizers(tmp, stdout):
    try:
        exe = build(tmp, "demod_plan_table_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    except subprocess.CalledProcessError:
        pytest.skip("no sanitizer runtime to link against")
    r = subprocess.run([exe], input=INPUT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == stdout

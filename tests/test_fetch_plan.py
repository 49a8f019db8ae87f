"""The served end's planner (phantomsdr_amd/csrc/fetchplan.h) without a GPU and without the library: tests/fetch_plan_table.cpp is
compiled with the host C++ compiler - the header is plain C++17 - and runs the script below.  What it plans: the spans of the
IQ, carrier and squelch copies, the bytes of waterfall rows, the ordered list of a fetch's copies, the ring of host sets and
whose rows a slot of a fetched set holds.  Every expectation here is written from the rules (include/psdr.h), and
the whole output is held against the hash of what the same lines printed while they still sat in psdr_fetch_begin, between
the HIP calls."""
import hashlib
import json
import os
import subprocess

import pytest

import fetch_plan_table as T
from conftest import ROOT

AUDIO, PCM, WF, IQB = 1, 2, 4, 8  # PSDR_FETCH_*
USB, AM, IQ, SAM = 0, 2, 4, 5     # PSDR_USB, PSDR_AM, PSDR_IQ, PSDR_SAM
SETS = 4                          # PSDR_FETCH_SETS
MB, H = 4, 124                    # max_batch, n / 2 of the copies' grid
# slot -> (active, part of the batch, mode, squelch): tests/test_gpu_fetch_paths.py's population, and beside it what must not
# count - slot 2 matches everything and has no client, slot 7 matches everything and sat the batch out
SLOTS = [(1, 1, USB, 1), (1, 1, IQ, 0), (0, 1, IQ, 1), (1, 1, SAM, 0), (1, 1, AM, 1), (1, 1, IQ, 0), (1, 1, SAM, 0), (1, 0, SAM, 1)]
SPANS = {"iq": (1, 5), "car": (3, 4), "sq": (0, 5)}
# waterfall slot -> (active, nsent, out_off, l, r): 4 x 1000 bytes at 0, nobody, 4 x 701 bytes at 4000 (6804: 12 short of a piece)
WSLOTS = [(1, 4, 0, 0, 1000), (0, 4, 4000, 0, 4096), (1, 4, 4000, 10, 711)]
WF_BYTES = 6816
PLAIN = 16  # the clients of the byte count: bench.py's kind, nothing for a span


def slots_lines(slots):
    return ["slots %d" % len(slots)] + ["slot %d %d %d %d %d" % ((i,) + s) for i, s in enumerate(slots)]


def wf_lines(wslots):
    return ["wfslots %d" % len(wslots)] + ["wfslot %d %d %d %d %d %d" % ((i,) + w) for i, w in enumerate(wslots)]


# ---- the script: (line, key) - key names the output line of an operation that prints
def script():
    s = []
    say = lambda lines: s.extend((ln, None) for ln in lines)
    # spans
    say(wf_lines([(0, 0, 0, 0, 0)]))
    cases = {
        "nobody": [(1, 1, USB, 0)] * 8,
        "one": [(1, 1, USB, 0)] * 3 + [(1, 1, IQ, 1)] + [(1, 1, USB, 0)] * 4,
        "one_sam": [(1, 1, USB, 0)] * 7 + [(1, 1, SAM, 0)],
        "two": [(1, 1, AM, 0), (1, 1, IQ, 1), (1, 1, USB, 0), (1, 1, AM, 0), (1, 1, USB, 0), (1, 1, IQ, 1), (1, 1, USB, 0), (1, 1, AM, 0)],
        "two_sam": [(1, 1, AM, 0), (1, 1, SAM, 0), (1, 1, USB, 0), (1, 1, AM, 0), (1, 1, USB, 0), (1, 1, SAM, 0), (1, 1, USB, 0), (1, 1, AM, 0)],
        "absent": [(0, 1, IQ, 1), (1, 1, IQ, 1), (1, 1, USB, 0), (1, 0, IQ, 1), (1, 1, USB, 0), (1, 1, IQ, 1), (0, 0, IQ, 1), (1, 0, IQ, 1)],
        "absent_sam": [(0, 1, SAM, 1), (1, 1, SAM, 1), (1, 1, USB, 0), (1, 0, SAM, 1), (1, 1, USB, 0), (1, 1, SAM, 1), (0, 0, SAM, 1), (1, 0, SAM, 1)],
        "population": SLOTS,
    }
    for name, slots in cases.items():
        say(slots_lines(slots))
        for what in range(1, 16):
            s.append(("plan %d %d %d %d 0" % (what, MB, MB, H), ("span", name, what)))
    # copies
    say(slots_lines(SLOTS) + wf_lines(WSLOTS))
    for what in range(1, 16):
        for F in (1, MB - 1, MB):
            for p16 in (0, 1):
                s.append(("plan %d %d %d %d %d" % (what, MB, F, H, p16), ("copies", what, F, p16)))
    say(slots_lines([(1, 1, USB, 0)] * PLAIN))
    for F in (1, MB - 1, MB):
        s.append(("plan %d %d %d %d 0" % (AUDIO | WF, MB, F, H), ("bytes", F)))
    # waterfall bytes
    for name, ws in {"nothing": [(1, 0, 0, 0, 1000), (0, 4, 0, 0, 1000), (1, 0, 64, 0, 10)], "whole": [(1, 2, 0, 0, 8)], "one_over": [(1, 1, 0, 0, 17)],
                     "one_short": [(1, 3, 16, 0, 5)], "max_not_sum": [(1, 4, 4000, 10, 711), (1, 4, 0, 0, 1000)]}.items():
        say(wf_lines(ws))
        s.append(("plan %d %d %d %d 0" % (WF, MB, MB, H), ("wf", name)))
        s.append(("plan %d %d %d %d 0" % (AUDIO, MB, MB, H), ("wf_unasked", name)))
    # ring
    for fill in range(SETS):
        for nf in range(SETS + 1):
            s.append(("oldest %d %d" % (fill, nf), ("oldest", fill, nf)))
    s.append(("ring", None))
    s.append(("end", ("ring", 0)))
    for i, op in enumerate(["begin"] * 5 + ["end"] * 5 + ["begin", "end", "begin", "begin", "end", "begin", "end", "end", "end"] + ["begin"] * 4):
        s.append((op, ("ring", i + 1)))
    # membership and rows
    for wseq, wborn, seq, born in ((7, 3, 7, 3), (7, 3, 7, 4), (6, 3, 7, 3), (0, 3, 7, 3), (6, 2, 7, 3)):
        for mode in (USB, IQ, SAM):
            for want_iq in (0, 1):
                s.append(("member %d %d %d %d %d %d" % (wseq, wborn, seq, born, mode, want_iq), ("member", wseq, wborn, seq, born, mode, want_iq)))
    for lo, n in ((0, 0), (1, 5), (3, 1), (0, 8)):
        for ident in (0, 1, 3, 5, 6, 7):
            for frame in (0, MB - 1):
                s.append(("row %d %d %d %d %d" % (ident, lo, n, MB, frame), ("row", ident, lo, n, frame)))
    return s


SCRIPT = script()
INPUT = "\n".join(ln for ln, _ in SCRIPT) + "\n"
KEYS = [k for _, k in SCRIPT if k is not None]


@pytest.fixture(scope="module")
def stdout():
    return T.run(T.program(), INPUT)


@pytest.fixture(scope="module")
def out(stdout):
    """{key: the line the operation printed}"""
    lines = stdout.splitlines()
    assert len(lines) == len(KEYS) == len(set(KEYS))
    return dict(zip(KEYS, lines))


def test_trace_is_what_psdr_fetch_begin_computed_before_the_planner_moved(stdout):
    """recorded before any code moved: the parent's psdr_fetch_begin from its span loop to its last event record, the ring lines of
    psdr_fetch_begin / psdr_fetch_end, slot_in_fetched_set's conditions and psdr_fetched_iq's row arithmetic, compiled verbatim in
    front of a stand-in for the context and for the HIP calls, printed this script (tests/golden/fetch_plan_trace.json): a
    mismatch is a change of behaviour"""
    with open(os.path.join(ROOT, "tests", "golden", "fetch_plan_trace.json")) as f:
        golden = json.load(f)
    assert hashlib.sha256(INPUT.encode()).hexdigest() == golden["input_sha256"], "the script changed: the trace was recorded for another"
    assert hashlib.sha256(stdout.encode()).hexdigest() == golden["output_sha256"]


def span(f, k):
    lo, n = f[k].split(":")
    return int(lo), int(n)


# ---- spans
def test_spans_run_from_the_lowest_to_the_highest_slot_that_counts(out):
    audio_bits = lambda what: bool(what & (AUDIO | PCM | IQB))
    for what in range(1, 16):
        f = {name: T.fields(out[("span", name, what)]) for name in ("nobody", "one", "one_sam", "two", "two_sam", "absent", "absent_sam", "population")}
        iq, other = bool(what & IQB), audio_bits(what)  # IQ rows only with PSDR_FETCH_IQ; carrier records and flags with any audio bit
        assert [span(f["nobody"], k) for k in ("iq", "car", "sq")] == [(0, 0)] * 3
        assert span(f["one"], "iq") == ((3, 1) if iq else (0, 0)) and span(f["one"], "sq") == ((3, 1) if other else (0, 0)) and span(f["one"], "car") == (0, 0)
        assert span(f["one_sam"], "car") == ((7, 1) if other else (0, 0))
        assert span(f["two"], "iq") == ((1, 5) if iq else (0, 0)) and span(f["two"], "sq") == ((1, 5) if other else (0, 0))
        assert span(f["two_sam"], "car") == ((1, 5) if other else (0, 0)) and span(f["two_sam"], "iq") == (0, 0)
        # a slot without a client, or one that sat the batch out, does not count: at either end, or beyond it
        assert span(f["absent"], "iq") == ((1, 5) if iq else (0, 0)) and span(f["absent"], "sq") == ((1, 5) if other else (0, 0))
        assert span(f["absent_sam"], "car") == ((1, 5) if other else (0, 0))
        pop = f["population"]
        assert span(pop, "iq") == (SPANS["iq"] if iq else (0, 0))
        assert (span(pop, "car"), span(pop, "sq")) == ((SPANS["car"], SPANS["sq"]) if other else ((0, 0), (0, 0)))
        # who reads its flags from the span: the slots that ran with squelch - others inside the span read open
        assert pop["winsq"] == ("10001000" if other else "00000000")


# ---- copies
def expected_ops(what, S, F, p16, spans, wfb):
    ops = []

    def rows(buf, first, slots, row_bytes, elems, stream=0):
        off = first * MB * elems
        if F == MB:  # the batch fills max_batch: one plain copy, every byte of the slots' rows
            ops.append("copy:%s:%d:plain:%d:%d" % (buf, off, slots * MB * row_bytes, stream))
        else:
            ops.append("copy:%s:%d:pitched:%d:%d:%d:%d" % (buf, off, MB * row_bytes, F * row_bytes, slots, stream))

    if wfb:
        ops += ["copy:wf:0:plain:%d:0" % wfb, "record:ev_wf:0"]
    if what & (AUDIO | PCM | IQB):
        rows("pwr", 0, S, 4, 1)
        rows("nan", 0, S, 4, 1)
        if what & AUDIO:
            rows("audio", 0, S, H * 4, H)
        for buf, k, rb, el in (("iq", "iq", H * 8, H), ("car", "car", 8, 1), ("sq", "sq", 4, 1)):
            lo, n = spans[k]
            if n:
                rows(buf, lo, n, rb, el)
        ops.append("record:ev_audio:0")
    ops.append("record:done:0")
    if what & PCM:
        rows("pcm", 0, S, H * (2 if p16 else 4), H, stream=1)
        ops.append("record:ev_pcm:1")
    return ops


def moved(ops):
    """{buffer: bytes that matter}"""
    res = {}
    for op in ops:
        p = op.split(":")
        if p[0] == "copy":
            res[p[1]] = int(p[4]) if p[3] == "plain" else int(p[5]) * int(p[6])
    return res


def test_every_fetch_gets_exactly_its_copies_in_order(out):
    for what in range(1, 16):
        for F in (1, MB - 1, MB):
            for p16 in (0, 1):
                f = T.fields(out[("copies", what, F, p16)])
                audio = bool(what & (AUDIO | PCM | IQB))
                spans = {"iq": SPANS["iq"] if what & IQB else (0, 0), "car": SPANS["car"] if audio else (0, 0), "sq": SPANS["sq"] if audio else (0, 0)}
                wfb = WF_BYTES if what & WF else 0
                ops = f["ops"].split(",")
                assert ops == expected_ops(what, len(SLOTS), F, p16, spans, wfb), (what, F, p16)
                ncopy = sum(1 for op in ops if op.startswith("copy:"))
                assert ncopy <= 8 and all((":plain:" in op) == (F == MB) for op in ops if op.startswith("copy:") and not op.startswith("copy:wf:"))
                m = moved(ops)
                want = {}
                if wfb:
                    want["wf"] = wfb
                if audio:
                    want.update(pwr=len(SLOTS) * F * 4, nan=len(SLOTS) * F * 4)
                    want.update({k: spans[k][1] * F * rb for k, rb in (("iq", H * 8), ("car", 8), ("sq", 4)) if spans[k][1]})
                if what & AUDIO:
                    want["audio"] = len(SLOTS) * F * H * 4
                if what & PCM:
                    want["pcm"] = len(SLOTS) * F * H * (2 if p16 else 4)
                assert m == want, (what, F, p16)
                assert int(f["iq_bytes"]) == m.get("iq", 0) and int(f["wf_bytes"]) == wfb
                assert (int(f["frames"]), int(f["seq"]), int(f["has_pcm"])) == (F if audio else 0, int(audio), int(bool(what & PCM)))


def test_bytes_of_an_audio_and_waterfall_fetch(out):
    """bench.py's served-end figure (tests/test_bench_cli.py): clients x F x (n/2 x 4 + 8) + the waterfall rows"""
    for F in (1, MB - 1, MB):
        f = T.fields(out[("bytes", F)])
        assert sum(moved(f["ops"].split(",")).values()) == PLAIN * F * (H * 4 + 8) + WF_BYTES


# ---- waterfall bytes
def test_waterfall_bytes(out):
    wfb = lambda name: int(T.fields(out[("wf", name)])["wf_bytes"])
    assert wfb("nothing") == 0                       # no frame sent, or no client
    assert T.fields(out[("wf", "nothing")])["ops"] == "record:done:0"
    assert wfb("whole") == 16 and wfb("one_over") == 32 and wfb("one_short") == 32  # up to whole 16-byte pieces
    assert wfb("max_not_sum") == WF_BYTES            # the client that reaches furthest, whatever its slot: not 4000 + 6804
    for name in ("nothing", "whole", "one_over", "one_short", "max_not_sum"):
        assert int(T.fields(out[("wf_unasked", name)])["wf_bytes"]) == 0  # without PSDR_FETCH_WATERFALL


# ---- ring
def test_oldest_set_in_flight(out):
    for fill in range(SETS):
        for nf in range(SETS + 1):
            assert int(T.fields(out[("oldest", fill, nf)])["set"]) == (fill - nf) % SETS


def test_five_begins_four_ends(out):
    ring = lambda i: out[("ring", i)]
    assert ring(0).startswith("end none")  # nothing begun
    for i in range(1, 6):
        f = T.fields(ring(i))
        # the fifth begin takes the first one's set, which is still in flight, and gives that fetch up
        assert (int(f["set"]), int(f["gave_up"]), int(f["inflight"]), int(f["cur"])) == ((i - 1) % SETS, int(i == 5), min(i, SETS), -1)
    for i in range(6, 10):
        f = T.fields(ring(i))
        assert int(f["fetch"]) == i - 4 and int(f["set"]) == int(f["cur"]) == (i - 5) % SETS and int(f["inflight"]) == 9 - i  # fetches 2..5
    assert ring(10).startswith("end none") and T.fields(ring(10))["cur"] == "0"
    # in step: every end delivers the oldest begin not yet delivered; a begin onto the set psdr_fetched_* read takes it away
    f = [T.fields(ring(i)) for i in range(11, 20)]
    assert (f[0]["set"], f[0]["cur"]) == ("1", "0") and (f[1]["fetch"], f[1]["cur"]) == ("6", "1")
    assert (f[2]["set"], f[3]["set"]) == ("2", "3") and (f[4]["fetch"], f[4]["cur"]) == ("7", "2")
    assert (f[5]["set"], f[5]["cur"]) == ("0", "2") and (f[6]["fetch"], f[7]["fetch"]) == ("8", "9") and f[7]["cur"] == "0"
    assert ring(19).startswith("end none")
    assert [(T.fields(ring(i))["set"], T.fields(ring(i))["cur"]) for i in range(20, 24)] == [("1", "0"), ("2", "0"), ("3", "0"), ("0", "-1")]


# ---- membership, rows
def test_membership(out):
    for key, ln in out.items():
        if key[0] != "member":
            continue
        _, wseq, wborn, seq, born, mode, want_iq = key
        f = T.fields(ln)
        # the slot's batch is the set's, and the client that holds the slot now was born as the one that did then
        assert int(f["part"]) == int(wseq == seq and wborn == born), key
        assert int(f["kind"]) == int((mode == IQ) == bool(want_iq)), key
    part = lambda *k: int(T.fields(out[("member",) + k])["part"])
    assert part(7, 3, 7, 3, USB, 0) == 1
    assert part(7, 3, 7, 4, USB, 0) == 0  # the same slot, a new client
    assert part(6, 3, 7, 3, USB, 0) == 0  # the same client, an earlier batch
    assert part(0, 3, 7, 3, USB, 0) == 0  # no client at the time of the fetch


def test_rows(out):
    for key, ln in out.items():
        if key[0] != "row":
            continue
        _, ident, lo, n, frame = key
        f = T.fields(ln)
        assert int(f["row"]) == ident * MB + frame
        held = lo <= ident < lo + n
        assert int(f["held"]) == int(held) and ("span_row" in f) == held
        if held:
            assert int(f["span_row"]) == (ident - lo) * MB + frame


def test_sanitizers(tmp_path, stdout):
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    probe = tmp_path / "sanitizer_probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17", *flags, str(probe), "-o", str(tmp_path / "sanitizer_probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime to link against")
    san = T.build(tmp_path, "fetch_plan_table_san", flags)
    assert T.run(san, INPUT, timeout=600) == stdout

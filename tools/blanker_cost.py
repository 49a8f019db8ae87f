"""What the impulse blanker costs the step: cfg2's shape (2^20-point IQ, s16), 512-frame psdr_process_ring launches out of a ring
of 1024 halves, no clients - the library without the feature (PARENT_LIB: a libpsdr_hip.so built from the parent commit) against
this one with the blanker off, on with a threshold that is never reached (90 dB) and on with one planted impulse per half
(12 dB, guard 7), interleaved in one job on one GPU, one child process per measurement.  Every step first rewrites the 513
halves it reads (untimed: the impulses must be there again), then times ONE process call between two synchronisations.

    python tools/blanker_cost.py PARENT_LIB [OUT.json]             the driver
    python tools/blanker_cost.py --child parent|off|clean|impulse  one measurement: prints one JSON line
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEPS, WARMUP, F, NHALVES, ROUNDS = 20, 4, 512, 1024, 3
N = 1 << 20
STATES = ("parent", "off", "clean", "impulse")


def child(state):
    import numpy as np

    from helpers import quantize_raw, synth_stream
    from phantomsdr_amd import Context
    ctx = Context(N, False, 11, input_format="s16", max_batch=F, max_clients=1)
    ctx.ring_create(NHALVES)
    half = quantize_raw(synth_stream(N // 2, False, seed=5, ntones=0, fft_size=N), "s16", False)
    if state == "impulse":
        half[2 * 1000:2 * 1000 + 2] = (30000, -30000)
    pinned = ctx.pinned_array(half.nbytes)
    pinned[:] = half.view(np.uint8)
    if state == "clean":
        ctx.ring_set_blanker(True, 90.0, 7)
    elif state == "impulse":
        ctx.ring_set_blanker(True, 12.0, 7)
    ms = []
    for i in range(WARMUP + STEPS):
        first = i * F
        for h in range(first if i == 0 else first + 1, first + F + 1):  # (half `first` was the last one of the step before)
            ctx.ring_write_async(h, pinned)
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.process_ring(first, F)
        ctx.synchronize()
        if i >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    out = {"state": state, "ms_per_step": sum(ms) / len(ms), "min_ms": min(ms), "max_ms": max(ms)}
    if state in ("clean", "impulse"):
        last = (WARMUP + STEPS - 1) * F
        out["blanked_in_last_step"] = sum(ctx.ring_read_blanker(h)[0] for h in range(last + 1, last + F + 1))
        ctx.set_profiling(1)
        ctx.reset_kernel_stats()
        for i in range(WARMUP + STEPS, WARMUP + STEPS + 6):
            for h in range(i * F + 1, i * F + F + 1):
                ctx.ring_write_async(h, pinned)
            ctx.process_ring(i * F, F)
        ctx.synchronize()
        for name in ("blanker_scan", "blanker_apply", "fft_pass1"):
            us = sorted(ctx.kernel_samples(name))
            out[name + "_us"] = {"launches": len(us), "median": float(us[len(us) // 2]), "min": float(us[0]), "max": float(us[-1])}
        ctx.set_profiling(0)
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    parent_lib = os.path.abspath(sys.argv[1])
    res = {s: [] for s in STATES}
    detail = {}
    for r in range(ROUNDS):
        for state in STATES:
            env = dict(os.environ)
            if state == "parent":
                env["PSDR_LIB"], env["PSDR_LIB_LENIENT"] = parent_lib, "1"
            t0 = time.time()
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", state], env=env, capture_output=True, text=True, timeout=280)
            if p.returncode != 0:  # (nothing more is started on the GPU after a child that failed)
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit(p.returncode or 1)
            line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            res[state].append(round(line["ms_per_step"], 4))
            detail[state] = {k: v for k, v in line.items() if k not in ("state", "ms_per_step")}
            print(f"round {r} {state}: {line['ms_per_step']:.4f} ms per step ({time.time() - t0:.0f} s)", flush=True)
    lo, hi = min(res["parent"]), max(res["parent"])
    out = {"workload": f"cfg2's shape (2^20-point IQ, s16), {F}-frame psdr_process_ring launches, ring of {NHALVES} halves, no clients; {STEPS} steps behind "
                       f"{WARMUP} warm-up steps, each timed alone between two synchronisations, one process each, interleaved",
           "ms_per_step": res, "mean": {k: round(sum(v) / len(v), 4) for k, v in res.items()},
           "parent_spread_percent": round(100 * (hi - lo) / lo, 2),
           "off_within_parent_spread": bool(lo <= sum(res["off"]) / len(res["off"]) <= hi), "last_round": detail}
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

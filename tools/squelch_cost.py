"""What the squelch costs the step: cfg3's stream, 256 clients, 512-frame launches, post chain on - the library without the
feature (PARENT_LIB: a libpsdr_hip.so built from the parent commit) against this one with every client's squelch always open
(open_db = -300: the chain does the full work) and never open (open_db = 300: the chain's streams are empty), interleaved in one
job on one GPU, one child process per measurement (the first context of a process gets the quiet queues for the chain's streams).

    python tools/squelch_cost.py PARENT_LIB [OUT.json]          the driver
    python tools/squelch_cost.py --child parent|open|never      one measurement: prints one JSON line
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS, WARMUP, F, NCLIENTS, ROUNDS = 20, 6, 512, 256, 3


def child(state):
    import torch

    import bench
    wl = dict(bench.WORKLOADS["cfg3"])
    run = bench.SingleGpuRun(torch, torch.device("cuda:0"), 0, "cfg3", wl, F, 512, nclients=NCLIENTS)
    ctx = run.eng.ctx
    ctx.set_post_chain(True)
    if state != "parent":
        for c in run.eng.audio_clients:
            c.set_squelch(True, -300.0 if state == "open" else 300.0, None, 1, 0)
    dt = run.timed_block(STEPS, WARMUP)
    out = {"state": state, "ms_per_step": dt * 1e3 / STEPS}
    if state != "parent":
        heard = sum(int(c.read_squelch(F).sum()) for c in run.eng.audio_clients[:8])
        out["heard_frames_of_8_clients"] = heard
        ctx.set_profiling(1)
        ctx.reset_kernel_stats()
        for i in range(8):
            run.step(run.next_step + i)
        run.sync()
        us = ctx.kernel_samples("squelch")
        out["k_squelch_us"] = {"launches": int(len(us)), "median": float(sorted(us)[len(us) // 2]), "min": float(min(us)), "max": float(max(us))}
        ctx.set_profiling(0)
    run.close()
    print(json.dumps(out), flush=True)


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    parent_lib = os.path.abspath(sys.argv[1])
    res = {"parent": [], "open": [], "never": []}
    kernel = {}
    for r in range(ROUNDS):
        for state in ("parent", "open", "never"):
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
            if "k_squelch_us" in line:
                kernel[state] = line["k_squelch_us"]
                kernel[state + "_heard_frames_of_8_clients"] = line["heard_frames_of_8_clients"]
            print(f"round {r} {state}: {line['ms_per_step']:.4f} ms per step ({time.time() - t0:.0f} s)", flush=True)
    out = {"workload": f"cfg3 stream, {NCLIENTS} clients, {F}-frame launches, post chain on; {STEPS} steps behind {WARMUP} warm-up steps, one process each, interleaved",
           "ms_per_step": res, "mean": {k: round(sum(v) / len(v), 4) for k, v in res.items()},
           "parent_spread_percent": round(100 * (max(res["parent"]) - min(res["parent"])) / min(res["parent"]), 2), "k_squelch_us": kernel}
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""What the audio filter costs the step: cfg3's stream, 256 clients, 512-frame launches, post chain on - the library without the
feature (PARENT_LIB: a libpsdr_hip.so built from the parent commit) against this one with no filter client and with every
client on two sections (high-pass 300 Hz + de-emphasis 212 Hz), interleaved in one job on one GPU, one child process per
measurement (the first context of a process gets the quiet queues for the chain's streams).  With --bench the benchmark's own
workload (bench.py --gpus 1, cfg2, no filter client) is measured the same way against the parent's library.

    python tools/audio_filter_cost.py PARENT_LIB [OUT.json] [--bench]    the driver
    python tools/audio_filter_cost.py --child parent|none|two            one measurement: prints one JSON line

The driver starts nothing more on the GPU after a child that failed or ran into its time limit.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS, WARMUP, F, NCLIENTS, ROUNDS = 20, 6, 512, 256, 3
CHILD_LIMIT, BENCH_LIMIT = 200, 200  # seconds per process


def child(state):
    import torch

    import bench
    wl = dict(bench.WORKLOADS["cfg3"])
    run = bench.SingleGpuRun(torch, torch.device("cuda:0"), 0, "cfg3", wl, F, 512, nclients=NCLIENTS)
    ctx = run.eng.ctx
    ctx.set_post_chain(True)
    if state == "two":
        from phantomsdr_amd import design_audio_filter
        two = [design_audio_filter("highpass", 12000, 300.0), design_audio_filter("deemphasis", 12000, 212.0)]  # (the engine's audio rate)
        for c in run.eng.audio_clients:
            c.set_audio_filter(two)
    dt = run.timed_block(STEPS, WARMUP)
    out = {"state": state, "ms_per_step": dt * 1e3 / STEPS}
    if state != "parent":
        ctx.set_profiling(1)
        ctx.reset_kernel_stats()
        for i in range(8):
            run.step(run.next_step + i)
        run.sync()
        us = ctx.kernel_samples("audio_filter")
        if state == "none":
            assert len(us) == 0, "a batch without a filter client launched the kernel"
        else:
            out["k_audio_filter_us"] = {"launches": int(len(us)), "median": float(sorted(us)[len(us) // 2]), "min": float(min(us)), "max": float(max(us))}
        ctx.set_profiling(0)
    run.close()
    print(json.dumps(out), flush=True)


def one(cmd, env, limit):
    """one process under its own time limit -> its last JSON line; the driver ends with it if it fails"""
    try:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.stderr.write("time limit: %s\n" % " ".join(cmd))
        sys.exit(124)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(p.returncode or 1)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def spread(v):
    return round(100 * (max(v) - min(v)) / min(v), 2)


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    args = [a for a in sys.argv[1:] if a != "--bench"]
    parent_lib = os.path.abspath(args[0])
    parent_env = dict(os.environ, PSDR_LIB=parent_lib, PSDR_LIB_LENIENT="1")
    out = {"tool": "tools/audio_filter_cost.py"}
    if "--bench" in sys.argv:
        res = {"parent": [], "this": []}
        for r in range(ROUNDS):
            for state in ("parent", "this"):
                line = one([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                           parent_env if state == "parent" else dict(os.environ), BENCH_LIMIT)
                res[state].append(round(line["ms_per_step"], 4))
                print(f"bench round {r} {state}: {line['ms_per_step']:.4f} ms per step", flush=True)
        out["bench"] = {"workload": "bench.py --gpus 1 --steps 20 --warmup 5 (cfg2, no filter client), one process each, interleaved", "ms_per_step": res,
                        "mean": {k: round(sum(v) / len(v), 4) for k, v in res.items()}, "parent_spread_percent": spread(res["parent"])}
    else:
        res = {"parent": [], "none": [], "two": []}
        kernel = {}
        for r in range(ROUNDS):
            for state in ("parent", "none", "two"):
                t0 = time.time()
                line = one([sys.executable, os.path.abspath(__file__), "--child", state], parent_env if state == "parent" else dict(os.environ), CHILD_LIMIT)
                res[state].append(round(line["ms_per_step"], 4))
                if "k_audio_filter_us" in line:
                    kernel["round %d" % r] = line["k_audio_filter_us"]
                print(f"round {r} {state}: {line['ms_per_step']:.4f} ms per step ({time.time() - t0:.0f} s)", flush=True)
        out.update({"workload": f"cfg3 stream, {NCLIENTS} clients, {F}-frame launches, post chain on; {STEPS} steps behind {WARMUP} warm-up steps, one process each, interleaved",
                    "ms_per_step": res, "mean": {k: round(sum(v) / len(v), 4) for k, v in res.items()}, "parent_spread_percent": spread(res["parent"]),
                    "k_audio_filter_us": kernel})
    print(json.dumps(out))
    if len(args) > 1:
        with open(args[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

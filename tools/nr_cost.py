"""What the noise reduction costs the step: cfg2's shape with 16 and with 256 clients, 512-frame launches - every client with noise
reduction on (PSDR_NR_NORMAL) against the same library with it off, one child process per measurement, alternating - and the
benchmark's own line (bench.py --gpus 1, no such client) of this library against the parent's (PARENT_LIB: a libpsdr_hip.so built
from the parent commit), three alternating runs each.

    python tools/nr_cost.py PARENT_LIB [OUT.json]          the driver
    python tools/nr_cost.py --child off|on NCLIENTS        one measurement: prints one JSON line

The driver starts nothing more on the GPU after a child that failed or ran into its time limit.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS, WARMUP, F, ROUNDS = 20, 6, 512, 3
CLIENTS = (16, 256)
CHILD_LIMIT, BENCH_LIMIT = 200, 200  # seconds per process


def child(state, nclients):
    import torch

    import bench
    wl = dict(bench.WORKLOADS["cfg2"])
    run = bench.SingleGpuRun(torch, torch.device("cuda:0"), 0, "cfg2", wl, F, 512, nclients=nclients)
    ctx = run.eng.ctx
    if state == "on":
        for c in run.eng.audio_clients:
            c.set_noise_reduction("normal")
    dt = run.timed_block(STEPS, WARMUP)
    out = {"state": state, "clients": nclients, "ms_per_step": dt * 1e3 / STEPS}
    ctx.set_profiling(1)
    ctx.reset_kernel_stats()
    for i in range(8):
        run.step(run.next_step + i)
    run.sync()
    us = ctx.kernel_samples("audio_nr")
    if state == "off":
        assert len(us) == 0, "a batch without a noise-reduction client launched the kernel"
    else:
        out["k_audio_nr_us"] = {"launches": int(len(us)), "median": float(sorted(us)[len(us) // 2]), "min": float(min(us)), "max": float(max(us))}
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


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]))
    parent_env = dict(os.environ, PSDR_LIB=os.path.abspath(sys.argv[1]), PSDR_LIB_LENIENT="1")
    out = {"tool": "tools/nr_cost.py", "on_off": {}}
    for n in CLIENTS:
        res, kernel = {"off": [], "on": []}, []
        for r in range(ROUNDS):
            for state in ("off", "on"):
                line = one([sys.executable, os.path.abspath(__file__), "--child", state, str(n)], dict(os.environ), CHILD_LIMIT)
                res[state].append(round(line["ms_per_step"], 4))
                if "k_audio_nr_us" in line:
                    kernel.append(line["k_audio_nr_us"])
                print(f"{n} clients, round {r}, {state}: {line['ms_per_step']:.4f} ms per step", flush=True)
        mean = {k: sum(v) / len(v) for k, v in res.items()}
        out["on_off"][str(n)] = {"ms_per_step": res, "mean": {k: round(v, 4) for k, v in mean.items()}, "on_over_off": round(mean["on"] / mean["off"], 4),
                                 "k_audio_nr_us": kernel}
    out["workload"] = f"cfg2, {F}-frame launches, {STEPS} steps behind {WARMUP} warm-up steps, one process each, alternating"
    res = {"parent": [], "this": []}
    for r in range(ROUNDS):
        for state in ("parent", "this"):
            line = one([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                       parent_env if state == "parent" else dict(os.environ), BENCH_LIMIT)
            res[state].append(round(line["ms_per_step"], 4))
            print(f"bench round {r} {state}: {line['ms_per_step']:.4f} ms per step", flush=True)
    lo, hi = min(res["parent"]), max(res["parent"])
    mean = {k: round(sum(v) / len(v), 4) for k, v in res.items()}
    out["bench"] = {"workload": "bench.py --gpus 1 --steps 20 --warmup 5 (no noise-reduction client), one process each, alternating", "ms_per_step": res,
                    "mean": mean, "parent_spread_percent": round(100 * (hi - lo) / lo, 2), "this_mean_inside_parent_spread": lo <= mean["this"] <= hi}
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

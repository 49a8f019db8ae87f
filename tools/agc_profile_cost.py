"""What AGC profiles cost the step, and that a context without one costs what it did: cfg2's stream (35 MSPS IQ, 2^20 points:
12 kHz audio, audio_fft_size 360), 512-frame launches, post chain on, with 16 and with 256 clients, in three cases -
  parent   the library without the feature (PARENT_LIB: a libpsdr_hip.so built from the parent commit)
  none     this library, no profile set
  all      this library, every client on a profile (fast, capped: attack 5 ms, release 100 ms, max_gain 200)
interleaved in one job on one GPU, one child process per measurement (the first context of a process gets the quiet queues for
the chain's streams).

The condition is `none` against `parent`: the same launches (the per-kind launch counts of eight profiled steps), no table
allocated and a null PostArgs::agc_tab, the same registers and no scratch in the code objects of k_pc_want, k_pc_gain and
k_pc_agc (read from both libraries), and a mean step time no further above the parent's than the run-to-run spread of the
same command on this box - the larger of the two cases' own spreads, measured in the same job.  `all` is reported, not gated.
The driver writes the record first and then exits 1 if the condition fails.

    python tools/agc_profile_cost.py PARENT_LIB [OUT.json]              the driver
    python tools/agc_profile_cost.py --resources PARENT_LIB             the code objects' table alone (no GPU)
    python tools/agc_profile_cost.py --child parent|none|all NCLIENTS   one measurement: prints one JSON line

The driver starts nothing more on the GPU after a child that failed or ran into its time limit.
"""
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEPS, WARMUP, F, ROUNDS, COUNTS = 20, 6, 512, 3, (16, 256)
CHILD_LIMIT = 200  # seconds per process
STATES = ("parent", "none", "all")
KERNELS = ("psdr::k_pc_want", "psdr::k_pc_gain<", "psdr::k_pc_agc<")


def child(state, nclients):
    import torch

    import bench
    wl = dict(bench.WORKLOADS["clients256"])
    run = bench.SingleGpuRun(torch, torch.device("cuda:0"), 0, "clients256", wl, F, 512, nclients=nclients)
    ctx = run.eng.ctx
    ctx.set_post_chain(True)
    if state == "all":
        for c in run.eng.audio_clients:
            c.set_agc_profile("fast", max_gain=200.0)
    dt = run.timed_block(STEPS, WARMUP)
    out = {"state": state, "nclients": nclients, "ms_per_step": dt * 1e3 / STEPS}
    ctx.set_profiling(1)
    ctx.reset_kernel_stats()
    for i in range(8):
        run.step(run.next_step + i)
    run.sync()
    out["launches"] = {k: int(v[1]) for k, v in sorted(ctx.kernel_stats().items())}
    ctx.set_profiling(0)
    if state != "parent":
        ptrs = (ctypes.c_void_p * 2)()
        ctx.lib.psdr_debug_agc_profile_ptrs.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        assert ctx.lib.psdr_debug_agc_profile_ptrs(ctx.h, ptrs) == 0
        out["table_allocated"], out["agc_tab_passed"] = bool(ptrs[0]), bool(ptrs[1])
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


def resources(parent_lib):
    """registers and scratch of the kernels that form w or step the gain, from both libraries' gfx950 code objects"""
    import codeobj
    this_lib = os.environ.get("PSDR_LIB") or codeobj.SO
    pick = lambda meta: {k: {f: v[f] for f in ("vgpr", "agpr", "sgpr", "scratch", "lds")} for k, v in sorted(meta.items()) if k.startswith(KERNELS)}  # noqa: E731
    parent, this = pick(codeobj.kernel_metadata(parent_lib)), pick(codeobj.kernel_metadata(this_lib))
    return {"parent": parent, "this": this,
            "kernels_of_the_parent_unchanged": all(this.get(k) == v for k, v in parent.items()),
            "new_kernels": sorted(set(this) - set(parent)),
            "scratch_is_zero": all(v["scratch"] == 0 for v in list(parent.values()) + list(this.values()))}


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]))
    if sys.argv[1] == "--resources":
        print(json.dumps(resources(os.path.abspath(sys.argv[2])), indent=1))
        return 0
    parent_lib = os.path.abspath(sys.argv[1])
    parent_env = dict(os.environ, PSDR_LIB=parent_lib, PSDR_LIB_LENIENT="1")
    out = {"tool": "tools/agc_profile_cost.py", "resources": resources(parent_lib), "jobs": []}
    ok = out["resources"]["kernels_of_the_parent_unchanged"] and out["resources"]["scratch_is_zero"]
    for n in COUNTS:
        res = {s: [] for s in STATES}
        last = {}
        for r in range(ROUNDS):
            for state in STATES:
                t0 = time.time()
                line = one([sys.executable, os.path.abspath(__file__), "--child", state, str(n)], parent_env if state == "parent" else dict(os.environ), CHILD_LIMIT)
                res[state].append(round(line["ms_per_step"], 4))
                last[state] = line
                print(f"{n} clients round {r} {state}: {line['ms_per_step']:.4f} ms per step ({time.time() - t0:.0f} s)", flush=True)
        mean = {k: round(sum(v) / len(v), 4) for k, v in res.items()}
        sp = max(spread(res["parent"]), spread(res["none"]))
        cond = {"same_launches": last["none"]["launches"] == last["parent"]["launches"],
                "no_table_allocated": not last["none"]["table_allocated"], "agc_tab_null": not last["none"]["agc_tab_passed"],
                "none_over_parent_percent": round(100 * (mean["none"] / mean["parent"] - 1), 2),
                "allowed_percent": sp, "within_spread": mean["none"] <= mean["parent"] * (1 + sp / 100)}
        ok = ok and cond["same_launches"] and cond["no_table_allocated"] and cond["agc_tab_null"] and cond["within_spread"]
        out["jobs"].append({"workload": f"cfg2 stream (2^20-point IQ, 12 kHz audio, audio_fft_size 360), {n} clients, {F}-frame launches, post chain on; "
                                        f"{STEPS} steps behind {WARMUP} warm-up steps, one process each, interleaved",
                            "ms_per_step": res, "mean": mean, "spread_percent": {k: spread(v) for k, v in res.items()},
                            "launches_in_8_profiled_steps": {s: last[s]["launches"] for s in STATES}, "condition_b": cond,
                            "all_over_parent_percent": round(100 * (mean["all"] / mean["parent"] - 1), 2),
                            "all_passed_a_table": last["all"]["agc_tab_passed"]})
    out["condition_b_holds"] = bool(ok)
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

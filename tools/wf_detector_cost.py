"""Cost of the waterfall detectors on the cfg2 step (process + demod + waterfall, 512 frames, 16 SSB + 4 waterfall
clients): the same engine, same process, all four waterfall clients on SAMPLE, PEAK and MEAN in turn - median of
`--reps` repetitions of `--steps` steps each, the spread of the SAMPLE repetitions, the library's own event timing of
the two new kernels - and once the frame-at-a-time loop (max_batch = 1, a psdr_waterfall_batch call on every frame).

    python tools/wf_detector_cost.py [--out profiles/wf_detector_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def reps_ms(run, steps, reps, k0):
    out, k = [], k0
    for _ in range(reps):
        run.sync()
        t0 = time.perf_counter()
        for i in range(steps):
            run.step(k + i)
        run.sync()
        out.append((time.perf_counter() - t0) * 1e3 / steps)
        k += steps
    return out, k


def measure(torch, B, F, steps, reps, ring_mib):
    wl = B.WORKLOADS["cfg2"]
    run = B.SingleGpuRun(torch, torch.device("cuda", 0), 0, "cfg2", wl, F, ring_mib)
    res, k = {}, 0
    try:
        for i in range(max(3, steps // 2)):
            run.step(i)
        k = max(3, steps // 2)
        # SAMPLE twice (first and last): drift of the box shows as the difference between the two
        for name in ("sample", "peak", "mean", "sample_again"):
            for w in run.eng.waterfall_clients:
                w.set_detector(name.split("_")[0])
            _, k = reps_ms(run, max(2, steps // 4), 1, k)  # settle: allocates the carry on the first detector step
            t, k = reps_ms(run, steps, reps, k)
            res[name] = {"median_ms_per_step": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "reps_ms": [round(x, 4) for x in t]}
        # the two new kernels by the library's event brackets (a replay: markers lengthen the passes)
        for w in run.eng.waterfall_clients:
            w.set_detector("peak")
        ctx = run.eng.ctx
        ctx.set_profiling(1)
        ctx.reset_kernel_stats()
        for i in range(8):
            run.step(k + i)
        run.sync()
        st = ctx.kernel_stats()
        ctx.set_profiling(0)
        res["kernel_event_us_per_launch"] = {n: round(1e3 * ms / max(cnt, 1), 2) for n, (ms, cnt) in st.items()
                                             if n.startswith("waterfall")} if isinstance(st, dict) else str(st)
    finally:
        run.eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ring-mib", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wf_detector_cost.json"))
    a = ap.parse_args()
    import torch

    import bench as B
    out = {"workload": "cfg2: 2^20-point IQ s16, 16 SSB + 4 waterfall clients, skip_num 6",
           "batch_512": measure(torch, B, 512, a.steps, a.reps, a.ring_mib),
           "batch_1": measure(torch, B, 1, 600, a.reps, 64)}
    s = out["batch_512"]
    spread = s["sample"]["max"] - s["sample"]["min"]
    out["sample_spread_ms"] = spread
    for d in ("peak", "mean"):
        out[d + "_minus_sample_ms"] = s[d]["median_ms_per_step"] - s["sample"]["median_ms_per_step"]
        out[d + "_within_sample_spread"] = bool(s["sample"]["min"] <= s[d]["median_ms_per_step"] <= s["sample"]["max"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

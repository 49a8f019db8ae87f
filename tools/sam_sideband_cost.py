"""Cost of selectable-sideband SAM on the cfg2 step (process + demod + waterfall, 512 frames): the same engine, same process,
256 audio clients (bench.py's `clients256`) all PSDR_SAM, their sideband all BOTH and all UPPER in turn (interleaved: BOTH,
UPPER, BOTH, UPPER, ... - drift of the box lands on both alike) - medians of `--reps` repetitions of `--steps` steps each.
A sideband client's frame is a SAM client's - two plan runs - plus a mask and a multiplication.

    python tools/sam_sideband_cost.py [--out profiles/sam_sideband_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def block_ms(run, steps, k0):
    run.sync()
    t0 = time.perf_counter()
    for i in range(steps):
        run.step(k0 + i)
    run.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def measure(torch, B, nclients, F, steps, reps, ring_mib):
    wl = B.WORKLOADS["cfg2"]
    run = B.SingleGpuRun(torch, torch.device("cuda", 0), 0, "cfg2", wl, F, ring_mib, nclients=nclients)
    t = {"both": [], "upper": []}
    try:
        k = 0
        for c in run.eng.audio_clients:
            c.set_audio_demodulation("SAM")
        for mode in ("upper", "both"):  # settle: the sideband tails are allocated by the first sideband SAM client
            for c in run.eng.audio_clients:
                c.set_sam_sideband(mode)
            block_ms(run, max(3, steps // 2), k)
            k += max(3, steps // 2)
        for _ in range(reps):
            for mode in ("both", "upper"):
                for c in run.eng.audio_clients:
                    c.set_sam_sideband(mode)
                block_ms(run, 2, k)  # (the first batch after a switch)
                k += 2
                t[mode].append(block_ms(run, steps, k))
                k += steps
    finally:
        run.eng.close()
    res = {m: {"median_ms_per_step": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "reps_ms": [round(x, 4) for x in v]}
           for m, v in t.items()}
    both, up = res["both"]["median_ms_per_step"], res["upper"]["median_ms_per_step"]
    res.update(audio_clients=len(run.clients), frames_per_step=F, upper_minus_both_ms=up - both, upper_minus_both_percent=100.0 * (up - both) / both,
               upper_within_both_spread=bool(res["both"]["min"] <= up <= res["both"]["max"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--ring-mib", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_sideband_cost.json"))
    a = ap.parse_args()
    import torch

    import bench as B
    out = {"workload": "cfg2: 2^20-point IQ s16, 4 waterfall clients, every audio client PSDR_SAM with sideband BOTH / with sideband UPPER",
           "clients256": measure(torch, B, 256, a.frames, a.steps, a.reps, a.ring_mib)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

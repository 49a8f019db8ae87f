"""Cost of PSDR_IQ on the cfg2 step (process + demod + waterfall, 512 frames): the same engine, same process, its audio
clients all AM and all IQ in turn (interleaved: AM, IQ, AM, IQ, ... - drift of the box lands on both alike), with cfg2's 16
clients and with the 256-client shape (bench.py's `clients256`) - medians of `--reps` repetitions of `--steps` steps each.
An IQ client writes 8 bytes per sample where an AM client writes 4: 4 * (n/2) more bytes per client and frame.

    python tools/iq_mode_cost.py [--out profiles/iq_mode_cost.json]
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
    t = {"AM": [], "IQ": []}
    try:
        k = 0
        for mode in ("IQ", "AM"):  # settle: the IQ rows are allocated by the first IQ client
            for c in run.eng.audio_clients:
                c.set_audio_demodulation(mode)
            block_ms(run, max(3, steps // 2), k)
            k += max(3, steps // 2)
        for _ in range(reps):
            for mode in ("AM", "IQ"):
                for c in run.eng.audio_clients:
                    c.set_audio_demodulation(mode)
                block_ms(run, 2, k)  # (the first batch after a switch)
                k += 2
                t[mode].append(block_ms(run, steps, k))
                k += steps
    finally:
        run.eng.close()
    h = run.params["audio_fft_size"] // 2
    res = {m: {"median_ms_per_step": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "reps_ms": [round(x, 4) for x in v]}
           for m, v in t.items()}
    am, iq = res["AM"]["median_ms_per_step"], res["IQ"]["median_ms_per_step"]
    res.update(audio_clients=len(run.clients), frames_per_step=F, extra_bytes_per_step=4 * h * len(run.clients) * F,
               iq_minus_am_ms=iq - am, iq_minus_am_percent=100.0 * (iq - am) / am,
               iq_within_am_spread=bool(res["AM"]["min"] <= iq <= res["AM"]["max"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--ring-mib", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iq_mode_cost.json"))
    a = ap.parse_args()
    import torch

    import bench as B
    out = {"workload": "cfg2: 2^20-point IQ s16, 4 waterfall clients, every audio client AM / every audio client IQ",
           "clients16": measure(torch, B, None, a.frames, a.steps, a.reps, a.ring_mib),
           "clients256": measure(torch, B, 256, a.frames, a.steps, a.reps, a.ring_mib)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

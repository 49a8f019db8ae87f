"""Cost of fine tuning on the cfg2 step (process + demod + waterfall, 512 frames): the same engine, same process, its audio
clients all USB and all tuned USB in turn (interleaved: USB, tuned, USB, tuned, ... - drift of the box lands on both alike),
with cfg2's 16 clients and with the 256-client shape (bench.py's `clients256`) - medians of `--reps` repetitions of `--steps`
steps each.  A tuned USB client's frame is the transform of a USB client's plus one rotator and one complex product per
sample.

    python tools/fine_tune_cost.py [--out profiles/fine_tune_cost.json]
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
    t = {"USB": [], "tuned USB": []}
    try:
        k = 0
        for c in run.eng.audio_clients:
            c.set_audio_demodulation("USB")
        for fine in (True, False):  # settle: the tuned tails are allocated by the first tuned client
            for c in run.eng.audio_clients:
                c.set_fine_tune(fine)
            block_ms(run, max(3, steps // 2), k)
            k += max(3, steps // 2)
        for _ in range(reps):
            for name, fine in (("USB", False), ("tuned USB", True)):
                for c in run.eng.audio_clients:
                    c.set_fine_tune(fine)
                block_ms(run, 2, k)  # (the first batch after a switch)
                k += 2
                t[name].append(block_ms(run, steps, k))
                k += steps
    finally:
        run.eng.close()
    res = {m: {"median_ms_per_step": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "reps_ms": [round(x, 4) for x in v]}
           for m, v in t.items()}
    usb, ft = res["USB"]["median_ms_per_step"], res["tuned USB"]["median_ms_per_step"]
    res.update(audio_clients=len(run.clients), frames_per_step=F, tuned_minus_usb_ms=ft - usb, tuned_minus_usb_percent=100.0 * (ft - usb) / usb,
               tuned_within_usb_spread=bool(res["USB"]["min"] <= ft <= res["USB"]["max"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--ring-mib", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fine_tune_cost.json"))
    a = ap.parse_args()
    import torch

    import bench as B
    out = {"workload": "cfg2: 2^20-point IQ s16, 4 waterfall clients, every audio client USB / every audio client tuned USB",
           "clients16": measure(torch, B, None, a.frames, a.steps, a.reps, a.ring_mib),
           "clients256": measure(torch, B, 256, a.frames, a.steps, a.reps, a.ring_mib)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""bench.py — headline benchmark of the hot path (BASELINE.json metric).

A "step" is one pass of the hot path over one batch of F consecutive frames of a
device-resident raw sample ring: windowed 50 %-overlap forward FFT + int8 waterfall
pyramid, then the per-client slice -> inverse DFT -> demodulation for every audio client
and the byte gather for every waterfall client.  N=1 workload = BASELINE.json configs[1]:
35 MSPS-shape IQ cs16, 2^20-point FFT, 16 SSB audio clients + 4 waterfall clients.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

Rank 0 prints ONE JSON line.  `value` is whole-job ingest in MSamples/s (new complex
samples per second = frames/s * N/2) with the ring already resident in HBM, over ONE block
of exactly K timed steps after W warm-up steps; `ms_per_step` is that block's time / K.
A plain run does only that; --full adds everything else the line can carry (per-kernel
figures, post chain, served end, other workloads and shardings, the CPU baseline).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X spec (MI355X_MICROARCH.md)
COPY_CEILING = 6.29e12  # B/s: the plain device copy SURVEY.md 8(d) measured ("also report vs 6.29 TB/s measured-copy ceiling")

WORKLOADS = {
    # BASELINE.json configs[1]
    "cfg2": dict(sps=35_000_000, fft_size=1 << 20, is_real=False, fmt="s16", audio=16, waterfall=4,
                 modes=("USB", "LSB"), desc="35 MSPS IQ cs16, 2^20-pt C2C, 16 SSB audio + 4 waterfall clients"),
    # BASELINE.json configs[2]
    "cfg3": dict(sps=70_000_000, fft_size=1 << 21, is_real=True, fmt="s16", audio=64, waterfall=0,
                 modes=("USB", "LSB", "AM", "FM"), desc="70 MSPS real s16, 2^21-pt R2C, 64 mixed AM/FM/SSB clients"),
    # per-GPU share of BASELINE.json configs[3] (256 audio clients over 8 GPUs)
    "cfg4": dict(sps=35_000_000, fft_size=1 << 20, is_real=False, fmt="s16", audio=32, waterfall=0,
                 modes=("USB", "LSB", "AM", "FM"), desc="35 MSPS IQ cs16, 2^20-pt C2C, 32 audio clients per GPU"),
    # per-GPU share of BASELINE.json configs[4] (1024 clients + 64 zoomed waterfalls over 8 GPUs)
    "cfg5": dict(sps=70_000_000, fft_size=1 << 22, is_real=True, fmt="s16", audio=128, waterfall=8,
                 modes=("USB", "LSB", "AM", "FM"),
                 desc="70 MSPS real s16, 2^22-pt R2C, 128 audio clients + 8 zoomed waterfalls per GPU"),
    # the target's own wording: 256 concurrent (mixed) audio clients on one MI355X, cfg2's stream (the `clients256`
    # sub-object of the default line is this workload; here it can be profiled on its own)
    # (tuning only: 2^21-point IQ frames - the IQ twin of cfg5's 2^21-point packed transform, for A/Bs of the M1 x M2 split)
    "iq21": dict(sps=70_000_000, fft_size=1 << 21, is_real=False, fmt="s16", audio=32, waterfall=4,
                 modes=("USB", "LSB", "AM", "FM"), desc="70 MSPS IQ cs16, 2^21-pt C2C, 32 mixed audio + 4 waterfall clients (tuning)"),
    "clients256": dict(sps=35_000_000, fft_size=1 << 20, is_real=False, fmt="s16", audio=256, waterfall=4,
                       modes=("USB", "LSB", "AM", "FM"),
                       desc="35 MSPS IQ cs16, 2^20-pt C2C, 256 mixed USB/LSB/AM/FM audio + 4 waterfall clients"),
}
# frames per step: the latency / throughput knob (docs/history.md section 5, batch-size table).  A step of the two persistent passes has
# ~60-80 us of fixed cost (ramp, prologue, tail, the gaps between the kernels) whatever F is: 96.5 GS/s at F = 256, 99.9 at 512, 100.5
# at 1024 on one box.  512 frames of cfg2 are 7.7 s of a 35 MSPS stream and 13 GB of the 288 GB of HBM.
DEFAULT_BATCH = 512
# --dump-outputs: frames of the last step whose spectrum and pyramid are written, the seed that draws them (and the samples of
# arrays above their cap), and each array's cap in float32 entries (50 MiB in all)
DUMP_FRAMES = 2
DUMP_SEED = 0x5D5D0003
DUMP_CAPS = {"spectrum": 4 << 20, "pyramid": 2 << 20, "audio": 4 << 20, "audio_power": 1 << 18, "audio_nan": 1 << 18,
             "waterfall": 2 << 20}
SAMPLE_BYTES = {"u8": 1, "s8": 1, "u16": 2, "s16": 2, "f32": 4, "f64": 8}


def make_clients(wl, params, seed, count=None, first=0):
    """tuned ranges as in SURVEY 8d: centre uniform over the middle 90 % of [0,R); USB
    [m, m+3 kHz), LSB (m-3 kHz, m], AM/FM m +- 5 kHz; widths BW*N/sps bins."""
    rng = np.random.default_rng(seed)
    R = params["fft_result_size"]
    N, sps = wl["fft_size"], wl["sps"]
    b3 = int(3000 * N / sps)
    b5 = int(5000 * N / sps)
    out = []
    total = wl["audio"] if count is None else count
    for i in range(first + total):
        mode = wl["modes"][i % len(wl["modes"])]
        m = int(rng.uniform(0.05 * R, 0.95 * R))
        if mode == "USB":
            c = (mode, m, float(m), m + b3)
        elif mode == "LSB":
            c = (mode, m - b3, float(m), m)
        else:
            c = (mode, m - b5, float(m), m + b5)
        if i >= first:
            out.append(c)
    return out


def make_waterfalls(wl, params, seed):
    rng = np.random.default_rng(seed + 1000)
    R, levels = params["fft_result_size"], params["downsample_levels"]
    out = [(levels - 1, 0, R >> (levels - 1))]  # full span at the coarsest level
    for i in range(1, wl["waterfall"]):
        lv = int(rng.integers(0, levels - 1))
        width = 1024
        l = int(rng.integers(0, (R >> lv) - width))
        out.append((lv, l, l + width))
    return out[: wl["waterfall"]]


def algorithmic_bytes_per_frame(wl, params, clients, waterfalls):
    """B_frame = N*S_in + 8*R_spec + Q + C*(8*w + 4*n/2 + 4) + W*2*v"""
    N, is_real = wl["fft_size"], wl["is_real"]
    R = params["fft_result_size"]
    n = params["audio_fft_size"]
    s_in = SAMPLE_BYTES[wl["fmt"]] * (1 if is_real else 2)
    r_spec = N // 2 + 1 if is_real else N
    q = sum(R >> i for i in range(params["downsample_levels"]))
    b_in, b_spec, b_q = N * s_in, 8 * r_spec, q
    b_cl = sum(8 * (r - l) + 4 * (n // 2) + 4 for _, l, _, r in clients)
    b_wf = sum(2 * (r - l) for _, l, r in waterfalls) / params["skip_num"]
    return dict(input=b_in, spectrum=b_spec, pyramid=b_q, clients=b_cl, waterfall=b_wf,
                total=b_in + b_spec + b_q + b_cl + b_wf)


def gen_ring_torch(torch, device, nhalves, N, is_real, seed):
    """synthetic raw ring on the GPU: white Gaussian noise at sigma = 2^-9 FS plus 8 CW
    tones, quantised to s16 (interleaved I/Q for IQ)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    comps = 1 if is_real else 2
    half = (N // 2) * comps
    ring = torch.empty((nhalves, half), dtype=torch.int16, device=device)
    rng = np.random.default_rng(seed)
    tones = [(rng.uniform(-0.45, 0.45), rng.uniform(0.3, 1.0), rng.uniform(0, 6.28)) for _ in range(8)]
    amp = (2.0 if is_real else 1.0) / np.sqrt(N)
    for h in range(nhalves):
        t = torch.arange(h * (N // 2), (h + 1) * (N // 2), device=device, dtype=torch.float64)
        x = torch.randn((N // 2, comps), generator=g, device=device, dtype=torch.float32) * (2.0 ** -9)
        for f, a, ph in tones:
            arg = (2 * np.pi * f) * t + ph
            x[:, 0] += (amp * a * torch.cos(arg)).float()
            if not is_real:
                x[:, 1] += (amp * a * torch.sin(arg)).float()
        ring[h] = torch.clamp(torch.round(x * 32768.0), -32768, 32767).to(torch.int16).reshape(-1)
    return ring


def usable_host_threads():
    """(cpu ids this process may run on, the container's CPU quota in threads or None): the cgroup quota, not the
    affinity mask, is what a CPU-limited container sustains beyond a burst"""
    try:
        cpus = sorted(os.sched_getaffinity(0))
    except Exception:
        cpus = list(range(os.cpu_count() or 1))
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    quota = float(txt[0]) / float(txt[1])
            else:
                q = float(txt[0])
                if q > 0:
                    quota = q / float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            break
        except Exception:
            continue
    return cpus, quota


def cpu_baseline(wl, params, clients, waterfalls, budget_s=22.0, fft_library=None):
    """The oracle ("port") timed on this host's cores over a bounded sample of the same workload.
    The big forward transform runs through the first library found with the FFTW3 API - libfftw3f.so.3,
    then MKL's wrappers (libmkl_rt.so) - i.e. the kind of FFT the reference's FFTW back-end calls
    (src/fft_impl.cpp:89-117,145); if none loads, through the oracle's own radix-4 transform.  Which
    one is stated in `fft`.  Frames are independent for everything but the clients' overlap-add tails,
    so the CPU gets the same deal as the GPU's batches: W workers (threads; the oracle's C calls
    release the GIL), each a single-threaded pipeline PINNED to its own host thread - forward FFT + pyramid +
    every client's send_audio + the waterfall slices - on its own frames.
    A short probe over worker counts picks W; `value` is then the MEDIAN of three timed runs of >= 3.4 s each at that W
    (>= 10 s in total: what the host sustains, not what a 2-second burst under a cgroup CPU quota shows), and
    `stable` says whether it is within 20 % of the probe at the same W.  If not, the two best probe counts are
    re-measured the long way and the better sustained one is reported - with the disagreement spelled out."""
    import threading
    from oracle import oracle as O
    N, is_real = wl["fft_size"], wl["is_real"]
    n, levels = params["audio_fft_size"], params["downsample_levels"]
    R = params["fft_result_size"]
    rng = np.random.default_rng(1)
    nh = 4
    if is_real:
        halves = (rng.standard_normal((nh, N // 2)) * 2.0 ** -9).astype(np.float32)
    else:
        halves = ((rng.standard_normal((nh, N // 2)) + 1j * rng.standard_normal((nh, N // 2))) * 2.0 ** -9).astype(np.complex64)
    O.set_threads(1)
    libname = O.use_fft_library(fft_library) if fft_library != "" else ""
    cpus, quota = usable_host_threads()
    ncpu = len(cpus)
    eff = ncpu if quota is None else max(1, min(ncpu, int(quota + 0.999)))

    class Worker:
        def __init__(self, k):
            self.cpu = cpus[k % ncpu]
            self.fo = O.FFT(N, is_real, levels, 0, n)
            self.ocl = []
            for mode, l, m, r in clients:
                c = O.AudioClient(is_real, n, 12000, R)
                c.set_audio_demodulation(mode)
                c.set_audio_range(l, m, r)
                self.ocl.append(c)
            self.frames = 0

        def run(self, stop_at):
            try:
                os.sched_setaffinity(0, {self.cpu})  # pid 0 = the calling THREAD on Linux
            except Exception:
                pass
            fo = self.fo
            while time.perf_counter() < stop_at:
                f = self.frames
                fo.load(halves[f % (nh - 1)], halves[f % (nh - 1) + 1])
                fo.execute()
                spec = fo.output()
                for c in self.ocl:
                    c.send_audio(spec, f, fft=fo, stats=False)
                if f % params["skip_num"] == 0:
                    q = fo.quantized()
                    for lv, l, r in waterfalls:
                        off = sum(R >> t for t in range(lv))
                        _ = q[off + l: off + r].tobytes()
                self.frames += 1

    def measure(workers, seconds):
        for w in workers:
            w.frames = 0
        t0 = time.perf_counter()
        ths = [threading.Thread(target=w.run, args=(t0 + seconds,)) for w in workers]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        dt = time.perf_counter() - t0
        return sum(w.frames for w in workers), dt

    cand = sorted({c for c in (1, 2, 4, 8, 16, 32, 64, 128, eff, ncpu) if c <= ncpu})
    pool = [Worker(k) for k in range(max(cand))]
    to_msps = (N // 2) / 1e6
    probe_s = max(0.8, min(1.5, budget_s * 0.3 / len(cand)))
    probe = {}
    for c in cand:
        fr, dt = measure(pool[:c], probe_s)
        probe[c] = fr / dt * to_msps
    long_s = max(3.4, budget_s * 0.5 / 3)

    def sustained(c):
        runs = []
        for _ in range(3):
            fr, dt = measure(pool[:c], long_s)
            runs.append((fr / dt * to_msps, fr, dt))
        runs.sort()
        return runs[1], [round(r[0], 1) for r in runs]

    order = sorted(probe, key=probe.get, reverse=True)
    cores = order[0]
    (msps, frames, dt), runs = sustained(cores)
    tried = {str(cores): runs}
    stable = abs(msps - probe[cores]) <= 0.2 * probe[cores]
    note = None
    if not stable:
        sys.stderr.write(f"bench.py: CPU BASELINE UNSTABLE: {cores} workers gave {probe[cores]:.1f} MS/s in a {probe_s:.1f} s probe but "
                         f"{msps:.1f} MS/s sustained over 3 x {long_s:.1f} s (CPU quota of the container: {quota}); re-measuring\n")
        for alt in order[1:3]:
            (m2, f2, d2), r2 = sustained(alt)
            tried[str(alt)] = r2
            if m2 > msps:
                cores, msps, frames, dt, runs = alt, m2, f2, d2, r2
        note = (f"probe and sustained rate disagreed by more than 20 % at {order[0]} workers (a burst under the container's CPU quota); "
                f"`value` is the best SUSTAINED median among the probe's three best worker counts")
    fr1, dt1 = measure(pool[:1], max(1.5, budget_s / 12))
    fft = (os.path.basename(libname) + " through the FFTW3 API (fftwf_plan_dft_1d / fftwf_execute, ESTIMATE, 1 thread per plan)"
           if libname else "built-in radix-4 (oracle/psdr_oracle.c): no FFTW3-API library could be loaded")
    return {"value": round(msps, 3), "unit": "MSamples/s", "cores": cores, "kind": "port", "fft": fft,
            "stable": bool(stable), "note": note,
            "sustained_runs_MSamples_per_s": tried,
            "one_thread_MSamples_per_s": round(fr1 * (N // 2) / dt1 / 1e6, 3),
            "host_threads_available": ncpu, "container_cpu_quota_threads": quota,
            "probe_MSamples_per_s_by_workers": {str(k): round(v, 1) for k, v in sorted(probe.items())},
            "sample": f"{frames} frames of the same workload in {dt:.1f} s (the median of three such runs): {cores} single-threaded "
                      f"pipelines (oracle/psdr_oracle.c, forward FFT as stated in 'fft'), each pinned to its own host thread, of "
                      f"{ncpu} usable threads (CPU quota {quota}); one pipeline alone: {fr1} frames in {dt1:.1f} s"}


def cpu_threaded_pipeline(wl, params, threads, seconds=4.0):
    """ONE pipeline with the FFT library's own threads - the reference's configuration (fft_threads, src/fft_impl.cpp:82-88:
    fftwf_plan_with_nthreads + OpenMP loops around the window and the quantiser) and the shape of BASELINE.md section 2's
    table (the reference's `class FFTW` with MKL's threaded FFT, no clients attached: 269 MS/s on 8 threads at 2^20
    points).  FFT::load_*_input + FFT::execute only."""
    from oracle import oracle as O
    N, is_real = wl["fft_size"], wl["is_real"]
    rng = np.random.default_rng(1)
    if is_real:
        halves = (rng.standard_normal((3, N // 2)) * 2.0 ** -9).astype(np.float32)
    else:
        halves = ((rng.standard_normal((3, N // 2)) + 1j * rng.standard_normal((3, N // 2))) * 2.0 ** -9).astype(np.complex64)
    libname = O.use_fft_library(None)
    O.set_threads(threads)
    threaded = bool(libname) and O.fft_library_threads(threads)
    fo = O.FFT(N, is_real, params["downsample_levels"], 0, params["audio_fft_size"])
    for i in range(2):
        fo.load(halves[i], halves[i + 1])
        fo.execute()
    t0 = time.perf_counter()
    frames = 0
    while time.perf_counter() - t0 < seconds:
        fo.load(halves[frames % 2], halves[frames % 2 + 1])
        fo.execute()
        frames += 1
    dt = time.perf_counter() - t0
    return {"threads": threads, "MSamples_per_s": round(frames * (N // 2) / dt / 1e6, 1), "ms_per_frame": round(dt / frames * 1e3, 3),
            "fft": os.path.basename(libname) if libname else "built-in", "library_threads": threaded,
            "what": "one pipeline, FFT::load + FFT::execute (window, transform, /N, power, int8 pyramid), no clients: BASELINE.md section 2's measurement"}


def cpu_baseline_subprocess(wl_name, timeout_s=300, nclients=None):
    """runs cpu_baseline() in a child process (a third-party FFT library is dlopen()ed there: keep it
    away from the process that owns the GPU context) and falls back to the built-in transform; then, in further
    children with the FFT library's threading on, ONE pipeline with 8 and with all usable threads
    (`threaded_single_pipeline`: the reference's own configuration, comparable with BASELINE.md section 2)"""
    import subprocess
    out = None
    for lib in (None, ""):
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", wl_name]
        if nclients is not None:
            cmd += ["--cpu-clients", str(nclients)]
        if lib == "":
            cmd.append("--cpu-builtin-fft")
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s)
            if r.stderr and "UNSTABLE" in r.stderr:
                sys.stderr.write(r.stderr[-600:])
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode == 0 and line:
                out = json.loads(line[-1])
                break
            err = (r.stderr or "")[-300:]
        except Exception as e:  # timeout or a crash inside the library
            err = repr(e)
    if out is None:
        return {"error": err}
    cpus, quota = usable_host_threads()
    eff = len(cpus) if quota is None else max(1, min(len(cpus), int(quota + 0.999)))
    thr = []
    for k in sorted({min(8, eff), eff}):
        env = dict(os.environ, MKL_THREADING_LAYER="GNU", MKL_NUM_THREADS=str(k), OMP_NUM_THREADS=str(k), MKL_DYNAMIC="FALSE")
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-threaded-only", wl_name, "--cpu-threads", str(k)],
                               capture_output=True, text=True, timeout=120, env=env)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            thr.append(json.loads(line[-1]) if r.returncode == 0 and line else {"threads": k, "error": (r.stderr or "")[-200:]})
        except Exception as e:
            thr.append({"threads": k, "error": repr(e)})
    out["threaded_single_pipeline"] = thr
    return out


def visible_hip_devices():
    """hipGetDeviceCount without creating a context in this (launcher) process"""
    import ctypes
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        return n.value if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 else 0
    except OSError:
        return 0


def self_launch(ngpus):
    """N > 1 without a launcher: re-execute as `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
    --master-addr 127.0.0.1 --master-port P bench.py <same arguments>`.  Refuses (exit code 3, nothing on stdout)
    when fewer than N devices are visible: an N-GPU line is never printed by fewer than N ranks."""
    import socket
    import subprocess
    have = visible_hip_devices()
    if os.environ.get("PSDR_BENCH_ONE_DEVICE") == "1" and have >= 1:
        have = ngpus  # testing mode: all ranks share cuda:0 (see run_sharded_bench)
    if have < ngpus:
        sys.stderr.write(f"bench.py: --gpus {ngpus} but {have} HIP device(s) visible; not running\n")
        raise SystemExit(3)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this driver (RCCL needs it)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ngpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


def emit(out):
    """the ONE JSON line, as the last thing on stdout: RCCL prints a banner through C stdio whose
    buffer would otherwise be flushed after Python's at exit"""
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()
    if out is not None:
        print(json.dumps(out), flush=True)


TARGET_FRAC = 0.40  # BASELINE.json north_star: ">= 40 % of HBM roofline"


def path_roofline(b_frame, frames_per_s):
    """SURVEY 8(d) / BASELINE.md section 3, the graded figure: compulsory bytes of the WHOLE path per frame x frames/s
    over the HBM spec peak.  Reproduces from `value` alone: frames/s = value * 1e6 / (N/2)."""
    achieved = b_frame * frames_per_s
    return {"bound": "hbm", "achieved": round(achieved / 1e9, 2), "peak": HBM_PEAK / 1e9, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK, 4), "target_frac": TARGET_FRAC,
            "definition": "B_frame x frames/s / 8.0e12 (SURVEY 8d: input read once + spectrum + int8 pyramid written once + per-client "
                          "slices and audio; intermediates count zero); one step = one launch of every kernel of the path over "
                          "frames_per_launch frames",
            "algorithmic_bytes_per_frame": int(b_frame)}


def post_chain_measure(run, eng, params, wl, F, N, nclients, plain_ms):
    """SURVEY 8f-2 (widened row): the step with the optional post-demodulation chain on (DC blocker + AGC + int16).  NOT part
    of `value` (the metric's clients end at float audio).  The chain is a pipeline over the side stream, two chain streams and three
    rotating buffer sets: a batch's PCM is ready about two steps after its passes, so a repetition of K steps carries
    about two steps of drain - 200 steps per repetition (a server never drains), 50-step repetitions beside it."""
    try:
        # (this process creates several contexts: the chain's streams by measurement - psdr.h PSDR_OPT_POST_CHAIN_STREAMS = 1;
        # a server's one context gets the quiet hardware queues from the default creation order)
        if os.environ.get("PSDR_BENCH_AGC_FORM") is not None:  # (A/B of the chain's two AGC forms: psdr.h PSDR_OPT_POST_CHAIN_AGC)
            eng.ctx.set_option(eng.ctx.OPT_POST_CHAIN_AGC, int(os.environ["PSDR_BENCH_AGC_FORM"]))
        eng.ctx.set_post_chain(True, measured_streams=True)
        pk = 200
        pt = run.timed(pk, 5, min_reps=3, min_total_s=0.1)
        pt50 = run.timed(50, 3, min_reps=3, min_total_s=0.05)
        eng.ctx.set_post_chain(False)
        pdt = float(np.median(pt)) / pk
        h = params["audio_fft_size"] // 2
        return {"ms_per_step": round(pdt * 1e3, 3), "plain_ms_per_step": plain_ms,
                "over_plain": round(pdt * 1e3 / plain_ms, 4) if plain_ms else None,
                "MSamples_per_s_ingest": round(F * (N // 2) / pdt / 1e6, 1),
                "audio_clients": nclients,
                "audio_samples_per_s": round(nclients * F * h / pdt, 1),
                "realtime_factor": round(F * (N // 2) / pdt / wl["sps"], 1),
                "steps_per_repetition": pk,
                "ms_per_step_50_step_repetitions": round(float(np.median(pt50)) / 50 * 1e3, 3),
                "chain_streams": "chosen by measurement (PSDR_OPT_POST_CHAIN_STREAMS = 1)",
                "note": "whole step with psdr_set_post_chain(1): three f32 recurrences, sequential per client (one lane each); "
                        "repetitions of 200 steps between full synchronisations (50-step repetitions, as in round 4, beside it)"}
    except Exception as e:
        return {"error": repr(e)}


def with_fetch_measure(run, eng, params, wl, F, N, nclients, plain_ms, post):
    """The SERVED end of the path: the reference's send_audio / send_waterfall end in host memory
    (src/signal.cpp:283-291 -> src/audio.cpp:26-44, src/waterfall.cpp:44-51); `value`'s timed step leaves every client's
    results in HBM.  Here every step is followed by psdr_fetch_begin (the batch's audio + pwr + NaN flags + waterfall rows to
    pinned host memory on a copy stream, behind its kernels), the NEXT step is enqueued, then psdr_fetch_end of the previous
    batch: the copies run beside the next batch's passes.  Float audio without the post chain; with it the int32 PCM the
    reference hands its encoder INSTEAD of the floats.  NOT part of `value`."""
    ctx = eng.ctx
    h = params["audio_fft_size"] // 2
    wf_bytes = 0
    for lv, l, r in run.waterfalls:
        wf_bytes += (F + params["skip_num"] - 1) // params["skip_num"] * (r - l)
    d2h = nclients * F * (h * 4 + 8) + wf_bytes

    def reps(what, steps, nrep, warm=3, lag=1):
        # lag: how many batches the host stays behind - 1 for the float audio (ready right behind the demodulation), 3 for the
        # post chain's PCM (a batch's chain ends two to three steps after its passes: waiting for a younger batch right after
        # enqueueing batch b would leave the GPU without queued work); the ring of PSDR_FETCH_SETS = 4 host sets carries either
        def one(n):
            inflight = 0
            for i in range(n):
                run.step(run.next_step + i)
                if inflight == lag:
                    ctx.fetch_end()
                    inflight -= 1
                ctx.fetch_begin(what)
                inflight += 1
            while inflight:
                ctx.fetch_end()
                inflight -= 1
            run.sync()
            run.next_step += n
        one(warm)
        ts = []
        for _ in range(nrep):
            run.sync()
            t0 = time.perf_counter()
            one(steps)
            ts.append((time.perf_counter() - t0) / steps)
        return float(np.median(ts))

    def alone(what):  # the copies of one batch with nothing beside them
        run.step(run.next_step)
        run.next_step += 1
        run.sync()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            ctx.fetch_begin(what)
            ctx.fetch_end()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    def block(dt, base_ms, copy_s):
        return {"ms_per_step": round(dt * 1e3, 4), "step_without_fetch_ms": base_ms,
                "over_step_without_fetch": round(dt * 1e3 / base_ms, 4) if base_ms else None,
                "MSamples_per_s_ingest": round(F * (N // 2) / dt / 1e6, 1),
                "d2h_bytes_per_step": int(d2h), "d2h_GB_per_s_sustained": round(d2h / dt / 1e9, 2),
                "copies_alone_ms": round(copy_s * 1e3, 4), "copies_alone_GB_per_s": round(d2h / copy_s / 1e9, 2)}

    out = {"audio_clients": nclients, "frames_per_step": F,
           "pattern": "step(b); psdr_fetch_end(b - lag); psdr_fetch_begin(b) ... - a ring of four pinned host sets, the host `lag` "
                      "batches behind (1; 3 for the post chain's PCM, which is ready two to three steps after its passes, on its own copy stream); "
                      "repetitions of 50 steps between full synchronisations, median of 5"}
    try:
        what = ctx.FETCH_AUDIO | ctx.FETCH_WATERFALL
        out["float_audio"] = block(reps(what, 50, 5), plain_ms, alone(what))
        if post and post.get("ms_per_step"):
            ctx.set_post_chain(True)
            what = ctx.FETCH_PCM | ctx.FETCH_WATERFALL
            out["post_chain_pcm"] = block(reps(what, 50, 5, warm=6, lag=3), post.get("ms_per_step_50_step_repetitions") or post["ms_per_step"], alone(what))
            out["post_chain_pcm"]["host_lag_batches"] = 3
            out["post_chain_pcm"]["step_without_fetch_is"] = "post_chain.ms_per_step_50_step_repetitions (the same repetition length)"
            # the same with the PCM as int16 rows (psdr.h PSDR_OPT_POST_CHAIN_PCM16): half the bytes to the host - with hundreds of
            # clients the copy is what bounds this path
            try:
                ctx.set_option(ctx.OPT_POST_CHAIN_PCM16, 1)
                d2h_full = d2h
                d2h = nclients * F * (h * 2 + 8) + wf_bytes
                out["post_chain_pcm16"] = block(reps(what, 50, 5, warm=6, lag=3), post.get("ms_per_step_50_step_repetitions") or post["ms_per_step"], alone(what))
                out["post_chain_pcm16"]["host_lag_batches"] = 3
                out["post_chain_pcm16"]["note"] = "PSDR_OPT_POST_CHAIN_PCM16 = 1: int16 PCM rows (the reference's int32 buffer holds 16-bit values)"
                d2h = d2h_full
            finally:
                ctx.set_option(ctx.OPT_POST_CHAIN_PCM16, 0)
            ctx.set_post_chain(False)
    except Exception as e:
        out["error"] = repr(e)
    return out


def kernel_roofline(ctx, step, first_step, nsteps, wl, wl_name, params, clients, waterfalls, frames_per_launch,
                    clock_us=None, ms_per_step=None, ms_per_step_stamped=None, frames_per_s=None):
    """Per-kernel durations and the roofline block: `frac` is the whole path's
    (path_roofline: SURVEY 8d's figure), the dominant kernel on its own algorithmic bytes sits beside it as `kernel_*`.

    clock_us: {"fft_pass1": [...], "fft_pass2": [...]} - per-launch durations of the two FFT passes stamped on
      the device clock in the INSTRUMENTED repetitions of the timed loop (psdr_set_profiling mode 2: first work-group
      in -> last work-group out, no marker packets between the kernels; every third repetition of SingleGpuRun.timed,
      interleaved with the uninstrumented ones `value` comes from).  `roofline.achieved` uses their median.
    hipEvents: a replay of at least 50 steps after the timed loop with every launch bracketed by events on
      the stream it runs on (mode 1), in chunks of 5 steps; reported per kernel as the median chunk.  The
      marker packets lengthen the two passes (their sum can exceed the step): `perturbed` says so."""
    nsteps = max(nsteps, 50)
    chunk = 5
    ctx.set_profiling(1)
    per_chunk = {}
    launches = {}
    for c0 in range(0, nsteps, chunk):
        ctx.reset_kernel_stats()
        for i in range(chunk):
            step(first_step + c0 + i)
        ctx.synchronize()
        for name, (ms, cnt) in ctx.kernel_stats().items():
            per_chunk.setdefault(name, []).append(ms / cnt * 1e3)
            launches[name] = launches.get(name, 0) + int(cnt)
    ctx.set_profiling(0)
    ab = algorithmic_bytes_per_frame(wl, params, clients, waterfalls)
    Fl = frames_per_launch
    # algorithmic bytes by kernel: pass 1 reads the raw input once; the kernel that finishes the spectrum
    # writes it and the pyramid (IQ: pass 2; real input of 2^21 points and more: the fused pass 2; smaller real
    # transforms: the untangle pass); the demodulation kernels read slices and write audio; intermediates count zero.
    three_pass_real = wl["is_real"] and "untangle_real" in per_chunk
    per_kernel_bytes = {
        "fft_pass1": ab["input"] * Fl,
        "fft_pass2": 0 if three_pass_real else (ab["spectrum"] + ab["pyramid"]) * Fl,
        "untangle_real": (ab["spectrum"] + ab["pyramid"]) * Fl if three_pass_real else 0,
        "demod_idft": ab["clients"] * Fl,
    }
    kernels = {name: {"hip_event_us_median": round(float(np.median(v)), 3), "launches": launches[name]}
               for name, v in per_chunk.items()}
    clock_med = {}
    for name, v in (clock_us or {}).items():
        if len(v):
            clock_med[name] = float(np.median(v))
            kernels.setdefault(name, {})
            kernels[name].update({"device_clock_us_median": round(clock_med[name], 3),
                                  "device_clock_us_min_max": [round(float(np.min(v)), 2), round(float(np.max(v)), 2)],
                                  "device_clock_launches": int(len(v))})
    dur = {name: clock_med.get(name, float(np.median(v))) for name, v in per_chunk.items()}
    dom = max(dur, key=lambda k: dur[k]) if dur else None
    roofline = None
    if dom:
        avg_s = dur[dom] / 1e6
        achieved = per_kernel_bytes.get(dom, 0) / avg_s
        traffic = step_traffic = None
        tfile = os.path.join(ROOT, "profiles", "traffic.json")
        if os.path.exists(tfile):
            try:
                tj = json.load(open(tfile)).get(wl_name, {})
                scale = Fl / tj.get("_frames_per_launch", Fl)  # measured at tj["_frames_per_launch"] frames per launch
                traffic = tj.get(dom)
                if traffic is not None:
                    traffic = int(traffic * scale)
                tot = sum(v for k, v in tj.items() if not k.startswith("_"))
                step_traffic = int(tot * scale) if tot else None
            except Exception:
                traffic = step_traffic = None
        ev = {k: float(np.median(per_chunk[k])) for k in ("fft_pass1", "fft_pass2", "untangle_real") if k in per_chunk}
        fps = frames_per_s if frames_per_s else (Fl / (ms_per_step * 1e-3) if ms_per_step else 0.0)
        roofline = path_roofline(ab["total"], fps)
        roofline.update({
            "frames_per_launch": Fl, "traffic": step_traffic,
            "traffic_source": "rocprofv3 --pmc passes of this workload (profiles/traffic.json: FETCH_SIZE + WRITE_SIZE of every kernel of one "
                              "step), scaled to this batch size",
            "algorithmic_bytes_per_step": int(ab["total"] * Fl),
            # the dominant kernel on ITS OWN algorithmic bytes (pass 2: spectrum + pyramid written once)
            "kernel": dom, "kernel_achieved": round(achieved / 1e9, 2), "kernel_frac": round(achieved / HBM_PEAK, 4),
            "kernel_traffic": traffic, "kernel_algorithmic_bytes_per_launch": int(per_kernel_bytes.get(dom, 0)),
            "kernel_avg_launch_us": round(avg_s * 1e6, 2),
            "kernel_method": ("median launch duration on the device clock, stamped by the kernel itself in the instrumented repetitions of the timed loop (path.instrumentation)"
                              if dom in clock_med else "median of hipEvent brackets in a replay after the timed loop"),
            "kernel_hip_event_us": round(ev.get(dom, 0.0), 2) if dom in ev else None})
        if ms_per_step:
            # the passes of one step run back to back on one stream: their durations cannot add up to more
            # than the step unless the measurement itself lengthened them
            roofline["passes_sum_over_step"] = {
                # (against the step of the repetitions that carried the stamps)
                "device_clock": round(sum(clock_med.get(k, 0.0) for k in ("fft_pass1", "fft_pass2"))
                                      / ((ms_per_step_stamped or ms_per_step) * 1e3), 4)
                if clock_med else None,
                "hip_events": round(sum(ev.values()) / (ms_per_step * 1e3), 4)}
            roofline["perturbed"] = bool(sum(ev.values()) > 1.03 * ms_per_step * 1e3)
            roofline["perturbed_note"] = ("hipEvent figures only: the marker packets between the kernels lengthen the "
                                          "passes; `achieved` does not use them when device-clock stamps exist")
    return roofline, kernels, ab


def c_group_bench(ngpus, steps, warmup, F, ring_mib):
    """SURVEY 8e from C in ONE process: psdr_group_* (phantomsdr_amd/csrc/group.hip) over `ngpus` devices, RCCL called by
    the library itself - what the C++ server links (HipFanout with a device list).  cfg4's per-GPU shape (32 clients per
    GPU); the three shardings of the group, each with its achieved bytes per second over ONE root-to-peer link.
    With one device the communicator and the collectives are forced (PSDR_SHARD_FORCE_COMM): a plumbing run."""
    import ctypes as C
    from phantomsdr_amd import Group
    from phantomsdr_amd.core import derived_params
    wl = WORKLOADS["cfg4"]
    N = wl["fft_size"]
    p = derived_params(wl["sps"], N, wl["is_real"])
    nclients = wl["audio"] * ngpus
    clients = make_clients(dict(wl, audio=nclients), p, seed=0x5D5D0004)
    rng = np.random.default_rng(4)
    out = {"devices": ngpus, "frames_per_step": F, "audio_clients": nclients, "forced_single_device": ngpus == 1,
           "what": "one process, psdr_group_step: root transform -> RCCL exchange -> every device demodulates its clients", "by_shard": {}}
    for shard in ("band", "clients", "raw"):
        try:
            g = Group(list(range(ngpus)), shard, N, wl["is_real"], p["downsample_levels"], force_comm=ngpus == 1,
                      additional_size=p["audio_fft_size"], audio_fft_size=p["audio_fft_size"], input_format=wl["fmt"], max_batch=F,
                      max_clients=max(2 * wl["audio"], 1) if shard == "band" else wl["audio"], max_waterfall_clients=1, skip_num=p["skip_num"])
            root = g.root
            hb = root.half_frame_bytes()
            nb = max(2, (ring_mib << 20) // (hb * F))
            raw = rng.integers(-64, 64, size=(nb * F + 1) * hb // 2, dtype=np.int16)
            d = root.dev_alloc(raw.nbytes)
            root.h2d(d, raw)
            placed = 0
            for mode, l, m, r in clients:
                try:
                    g.client_add(l, m, r, mode)
                    placed += 1
                except Exception:
                    pass  # (band sharding: a band's device is full - the uniformly drawn windows do not split evenly)
            for i in range(warmup):
                g.step(d, F, i * F, offset_bytes=(i % nb) * F * hb)
            g.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                g.step(d, F, (warmup + i) * F, offset_bytes=(i % nb) * F * hb)
            g.synchronize()
            dt = time.perf_counter() - t0
            link_bytes, ex_ms = g.link_stats()
            out["by_shard"][shard] = {
                "value": round(steps * F * (N // 2) / dt / 1e6, 2), "ms_per_step": round(dt / steps * 1e3, 4), "clients_placed": placed,
                "link_bytes_per_step": int(link_bytes), "exchange_ms_last_step": round(ex_ms, 4),
                # (one device: the "exchange" is a copy onto itself - no link, no rate)
                "GB_per_s_per_link_during_exchange": round(link_bytes / (ex_ms * 1e-3) / 1e9, 2) if ex_ms > 0 and ngpus > 1 else None,
                "GB_per_s_per_link_over_the_step": round(link_bytes * steps / dt / 1e9, 2) if ngpus > 1 else None,
                "link_peak_GB_per_s": 153.0}
            root.dev_free(d)
            g.close()
        except Exception as e:
            out["by_shard"][shard] = {"error": repr(e)}
    return out


def run_sharded_bench(args, torch, rank, world, local_rank):
    """N > 1, one process per GPU over RCCL.  Five ways to shard the path are measured in the same run; `value` is the one
    --shard names - default `clients`, BASELINE.json configs[3] verbatim (256 audio clients sharded over the GPUs with an RCCL
    broadcast of the shared forward spectrum); the others sit beside it under `sharding`:

      clients  audio clients sharded over the ranks (client i -> rank i mod G); rank 0 FFTs and
               broadcasts each spectrum batch (8N bytes per frame) over RCCL/xGMI
      clients_pipelined  the same exchange, software-pipelined: the broadcast of batch i (from a staged copy) runs
               beside the transform of batch i+1 and the demodulation of batch i-1
      raw      the same sharding, but rank 0 broadcasts the RAW new half-frames (cs16: 2N bytes per
               frame, 4x fewer) and every rank runs the forward FFT itself (SURVEY 8e variant i)
      band     clients sharded by frequency band (rank g owns the windows starting in its 1/G of the spectrum);
               rank 0 FFTs, packs and SCATTERS one band + halo per rank: 8N/G bytes per frame and link
               (SURVEY 8e variant ii)
      time     the STREAM is sharded - batch g goes to rank g mod G with a two-frame warm-up instead of
               any exchange; every rank serves all the clients of its frames; no data-path collective
    """
    import torch.distributed as dist
    from phantomsdr_amd import SpectrumEngine
    from phantomsdr_amd.distributed import (BandShardedRunner, HipBackend, HipBandBackend, HipPipelinedBackend, HipRawBackend,
                                            HipTimeBackend, PipelinedShardedRunner, RawShardedRunner, ShardedRunner,
                                            TimeShardedRunner, assign_clients, assign_clients_by_band, band_bounds)

    device = torch.device("cuda", local_rank)
    # PSDR_BENCH_ONE_DEVICE=1 (testing only): every rank on cuda:0 over gloo - RCCL refuses two ranks on one device -
    # so that the N-process orchestration (self-launch, runners, HIP back-ends, stream ordering around the
    # collectives) can be exercised on a one-GPU box.  The line says so in `testing_mode`; its numbers mean nothing.
    one_device = os.environ.get("PSDR_BENCH_ONE_DEVICE") == "1"
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if one_device:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)

    def measure(mode, steps, warmup):
        time_mode = mode == "time"
        wl_name = args.workload or ("cfg2" if time_mode else "cfg4")
        wl = WORKLOADS[wl_name]
        N = wl["fft_size"]
        warm = TimeShardedRunner.WARMUP if time_mode else 0
        # time mode: a launch carries --batch frames INCLUDING the two warm-up frames, so its tile
        # count stays a multiple of the work-group count; F = the NEW frames per step
        F = args.batch - warm
        per_gpu = wl["audio"]
        # band mode: the uniformly drawn windows do not split evenly over the bands (the outer 5 % of the
        # spectrum hold none): room for twice the mean
        eng = SpectrumEngine(wl["sps"], N, wl["is_real"], input_format=wl["fmt"], max_batch=F + warm,
                             max_clients=max(per_gpu * (2 if mode == "band" else 1), 1),
                             max_waterfall_clients=max(wl["waterfall"], 1), device=local_rank)
        params = eng.params
        hb = eng.ctx.half_frame_bytes()
        nbatches = max(2, (args.ring_mib * (1 << 20)) // (hb * F))
        ring = None
        if time_mode or rank == 0:
            ring = gen_ring_torch(torch, device, nbatches * F + 1, N, wl["is_real"], seed=0x5D5D0004)
        torch.cuda.synchronize()
        waterfalls = []
        if time_mode:
            clients = make_clients(wl, params, seed=0x5D5D0002)
            waterfalls = make_waterfalls(wl, params, seed=0x5D5D0002)
            for mode_, l, m, r in clients:
                eng.add_audio_client(l, m, r, mode_)
            for lv, l, r in waterfalls:
                eng.add_waterfall_client(lv, l, r)
            backend = HipTimeBackend(eng.ctx, ring.data_ptr(), nbatches * F + 1, F + warm)
            runner = TimeShardedRunner(backend, rank, world, F)

            def step(i):
                first, skip = runner.step(i)
                if waterfalls:
                    eng.ctx.waterfall_batch(first - skip)
            nclients_total = len(clients)
            par = f"stream sharded over {world} GPUs: batch g -> rank g mod G, 2-frame warm-up, no data-path collective"
            bytes_per_frame = 0
        else:
            all_clients = make_clients(wl, params, seed=0x5D5D0004, count=per_gpu * world)
            if mode == "band":
                halo = params["audio_fft_size"]
                mine = assign_clients_by_band([(l, r) for _, l, _, r in all_clients], params["fft_result_size"], world,
                                              halo)[rank]
            else:
                mine = assign_clients(len(all_clients), world)[rank]
            clients = [all_clients[c] for c in mine]
            for mode_, l, m, r in clients:
                eng.add_audio_client(l, m, r, mode_)
            torch.cuda.synchronize()
            if mode == "raw":
                backend = HipRawBackend(torch, eng.ctx, device, ring.view(nbatches * F + 1, -1) if ring is not None else None,
                                        nbatches, F)
                runner = RawShardedRunner(backend, dist, rank, world, F)
                par = (f"clients sharded over {world} GPUs (client i -> rank i mod G); rank 0 broadcasts the RAW new "
                       "half-frames over RCCL, every rank runs the forward FFT")
                bytes_per_frame = hb
            elif mode == "clients_pipelined":
                backend = HipPipelinedBackend(torch, eng.ctx, device, ring.data_ptr() if ring is not None else 0, nbatches, F,
                                              rank == 0)
                runner = PipelinedShardedRunner(backend, dist, rank, world, F)
                par = (f"clients sharded over {world} GPUs (client i -> rank i mod G); rank 0 FFT + staged copy + RCCL "
                       "broadcast of the spectrum batch, the broadcast of batch i overlapping the transform of batch i+1")
                bytes_per_frame = 8 * params["fft_result_size"]
            elif mode == "band":
                backend = HipBandBackend(torch, eng.ctx, device, ring.data_ptr() if ring is not None else 0, nbatches, F,
                                         rank, world, halo, banded=False if os.environ.get("PSDR_BAND_PACK") == "1" else None)
                runner = BandShardedRunner(backend, dist, rank, world, F)
                how = ("rank 0's second FFT pass writes one contiguous region per band, the regions are the send buffers (no pack)"
                       if backend.banded else "rank 0 FFT + pack")
                par = (f"clients sharded by frequency band over {world} GPUs; {how} + RCCL scatter of one "
                       "band (+ one window of halo) per rank, the scatter of batch i overlapping the transform of batch i+1")
                bytes_per_frame = 8 * backend.bins
            else:
                backend = HipBackend(torch, eng.ctx, device, ring.data_ptr() if ring is not None else 0, nbatches, F)
                runner = ShardedRunner(backend, dist, rank, world, F)
                par = (f"clients sharded over {world} GPUs (client i -> rank i mod G); rank 0 FFT + RCCL broadcast "
                       "of the spectrum batch")
                bytes_per_frame = 8 * N
            step = runner.step
            nclients_total = per_gpu * world

        def fence():
            eng.ctx.synchronize()
            torch.cuda.synchronize()
            dist.barrier()
            torch.cuda.synchronize()

        flush = getattr(runner, "flush", lambda: None)  # band mode is pipelined: the last batch's scatter + demodulation
        for i in range(warmup):
            step(i)
        flush()
        fence()
        if not time_mode:
            runner.bytes_broadcast = 0
        t0 = time.perf_counter()
        for i in range(steps):
            step(warmup + i)
        flush()  # inside the timed region: K steps = K batches transformed, shipped AND demodulated
        fence()
        dt = time.perf_counter() - t0
        tmax = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
        # time mode: every rank ingests its own F new frames per step; client modes: one stream
        frames = steps * F * (world if time_mode else 1)
        msps = frames * (N // 2) / dt / 1e6
        # (the root GPU's: rank 0 reads the ring, transforms, and serves its share of the clients; time sharding: every rank its own frames)
        ab = algorithmic_bytes_per_frame(wl, params, clients, waterfalls)
        if args.full:
            roofline, kernels, _ = kernel_roofline(eng.ctx, step, warmup + steps, min(steps, 20), wl, wl_name, params,
                                                   clients, waterfalls, F + warm, ms_per_step=dt / steps * 1e3,
                                                   frames_per_s=frames / dt / (world if time_mode else 1))
        else:  # (the per-kernel replay is --full's)
            roofline, kernels = path_roofline(ab["total"], frames / dt / (world if time_mode else 1)), None
        if roofline:
            roofline["gpu"] = "rank 0 (root: raw ring, forward FFT, waterfalls, its share of the clients)"
        fence()
        res = {"value": round(msps, 2), "ms_per_step": round(dt / steps * 1e3, 4), "steps": steps,
               "workload": wl_name + ": " + wl["desc"], "frames_per_step": F, "fft_size": N,
               "audio_clients": nclients_total, "waterfall_clients": len(waterfalls), "parallelism": par,
               "realtime_factor": round(msps * 1e6 / wl["sps"], 1), "roofline": roofline,
               "path": {"algorithmic_bytes_per_frame": int(ab["total"]), "frames_per_s": round(frames / dt, 1),
                        "kernels": kernels,
                        "frac_of_hbm_peak_per_gpu": round(ab["total"] * frames / dt / HBM_PEAK / (world if time_mode else 1), 4)},
               "xgmi": None if time_mode else {
                   "broadcast_bytes_per_frame": bytes_per_frame,
                   "GB_per_s_per_link": round(runner.bytes_broadcast / dt / 1e9, 2) if world > 1 else None,
                   "link_peak_GB_per_s": 153.0,
                   "ingest_ceiling_MSamples_per_s": round(153.0e9 / bytes_per_frame * (N // 2) / 1e6, 1)}}
        eng.close()
        del ring
        torch.cuda.empty_cache()
        return res

    # `value`: the north star's sharding - clients over the ranks, ONE RCCL broadcast of the spectrum batch per step
    # (BASELINE.json configs[3]; link-bound at ~9.5 GS/s by construction: SURVEY 8e).  The cheaper exchanges of SURVEY 8e
    # (raw half-frames, one band per rank - the one whose ceiling grows with G), the pipelined broadcast and time sharding
    # are measured in the same run and reported under `sharding`.
    main_mode = args.shard or "clients"
    results = {}
    others = tuple(x for x in ("clients", "clients_pipelined", "raw", "band", "time") if x != main_mode) if args.full else ()
    for m in (main_mode,) + others:
        try:
            results[m] = measure(m, args.steps if m == main_mode else min(args.steps, 30),
                                 args.warmup if m == main_mode else min(args.warmup, 5))
        except Exception as e:  # a mode that fails must not take the line with it
            results[m] = {"error": repr(e)}
            try:
                torch.cuda.synchronize()
            except Exception:
                pass
    if "value" not in results[main_mode]:  # report the first sharding that ran, and say so
        ok = [m for m in results if "value" in results[m]]
        if not ok:
            raise SystemExit("every sharding failed: " + json.dumps(results))
        results["_requested"] = {"shard": main_mode, "error": results[main_mode]["error"]}
        main_mode = ok[0]
    # SURVEY 8e from C, in the same run: rank 0 starts ONE extra process that drives all N devices through psdr_group_*
    # (RCCL called by the library).  A child with a timeout: whatever happens to it, this line is still printed; the
    # other ranks wait on the rendezvous store (host side - a RCCL barrier would keep a kernel spinning on their GPUs).
    # (PSDR_BENCH_ONE_DEVICE: the child drives the one device with forced collectives - the orchestration is what is tested)
    c_group = None
    try:
        store = dist.distributed_c10d._get_default_store()
        if not args.full:
            pass
        elif rank == 0:
            import subprocess
            try:
                env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                                                       "GROUP_RANK", "ROLE_RANK", "LOCAL_WORLD_SIZE", "TORCHELASTIC_RUN_ID")}
                rr = subprocess.run([sys.executable, os.path.abspath(__file__), "--c-group-only", str(1 if one_device else world), "--steps", "10", "--warmup", "3",
                                     "--batch", str(args.batch)], capture_output=True, text=True, timeout=240, env=env)
                line = [ln for ln in rr.stdout.splitlines() if ln.startswith("{")]
                c_group = json.loads(line[-1]) if line else {"error": (rr.stderr or "")[-400:]}
            except Exception as e:
                c_group = {"error": repr(e)}
            store.set("psdr_c_group_done", "1")
        else:
            store.wait(["psdr_c_group_done"])
    except Exception as e:
        c_group = {"error": repr(e)}
    # the CPU baseline of THIS job (the oracle on rank 0's host cores over a bounded sample of the same workload with the
    # whole job's clients; a child process, the other ranks wait on the rendezvous store with idle GPUs)
    cpu = None
    try:
        store = dist.distributed_c10d._get_default_store()
        if rank == 0:
            if args.full and not args.no_cpu_baseline:
                r0 = results[main_mode]
                cpu = cpu_baseline_subprocess((r0.get("workload") or "cfg4").split(":")[0], nclients=r0.get("audio_clients"))
            store.set("psdr_cpu_baseline_done", "1")
        else:
            store.wait(["psdr_cpu_baseline_done"])
    except Exception as e:
        cpu = {"error": repr(e)}
    if rank == 0:
        r = results[main_mode]
        out = {
            "metric": "ingest MSamples/s + concurrent audio clients at 2^20-pt FFT",
            "value": r["value"], "unit": "MSamples/s", "n_gpus": int(dist.get_world_size()) if dist.is_initialized() else world,
            "rccl_ranks": int(dist.get_world_size()) if dist.is_initialized() else 0, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": r["ms_per_step"],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {k: r[k] for k in ("workload", "frames_per_step", "fft_size", "audio_clients", "waterfall_clients",
                                         "parallelism", "realtime_factor")},
            "roofline": r["roofline"], "path": r["path"], "xgmi": r["xgmi"],
            "shard": main_mode,
            "testing_mode": "PSDR_BENCH_ONE_DEVICE: all ranks on cuda:0 over gloo - orchestration smoke test, not a measurement" if one_device else None,
            "sharding": {m: {k: v for k, v in results[m].items() if k in ("value", "ms_per_step", "steps", "audio_clients",
                                                                           "parallelism", "xgmi", "error", "workload", "shard")}
                         for m in results},
            "north_star_sharding": {k: v for k, v in results.get("clients", {}).items() if k in ("value", "ms_per_step", "xgmi", "error")},
            "c_group": c_group,
            "cpu_baseline": cpu,
        }
    else:
        out = None
    if dist.is_initialized():
        emit(None)  # every rank flushes what RCCL wrote through C stdio ...
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        time.sleep(0.2)  # ... and rank 0's line comes last
    emit(out)


class SingleGpuRun:
    """One workload on one GPU: engine + device-resident ring + the bench's clients."""

    def __init__(self, torch, device, local_rank, wl_name, wl, F, ring_mib, nclients=None):
        from phantomsdr_amd import SpectrumEngine
        self.torch, self.wl_name, self.wl, self.F = torch, wl_name, wl, F
        nc = wl["audio"] if nclients is None else nclients
        self.eng = eng = SpectrumEngine(wl["sps"], wl["fft_size"], wl["is_real"], input_format=wl["fmt"],
                                        max_batch=F, max_clients=max(nc, 1),
                                        max_waterfall_clients=max(wl["waterfall"], 1), device=local_rank)
        self.params = eng.params
        self.N = wl["fft_size"]
        self.hb = eng.ctx.half_frame_bytes()
        # ring > 256 MiB Infinity Cache; a whole number of batches (+1 trailing half)
        self.nbatches = max(1, (ring_mib * (1 << 20)) // (self.hb * F))
        self.nhalves = self.nbatches * F + 1
        self.ring = gen_ring_torch(torch, device, self.nhalves, self.N, wl["is_real"], seed=0x5D5D0002)
        torch.cuda.synchronize()
        self.ring_ptr = self.ring.data_ptr()
        self.clients = make_clients(dict(wl, audio=nc), self.params, seed=0x5D5D0002)
        self.waterfalls = make_waterfalls(wl, self.params, seed=0x5D5D0002)
        for mode, l, m, r in self.clients:
            eng.add_audio_client(l, m, r, mode)
        for lv, l, r in self.waterfalls:
            eng.add_waterfall_client(lv, l, r)

    def step(self, i):
        eng = self.eng
        eng.ctx.process_batch(self.ring_ptr, self.F, offset_bytes=(i % self.nbatches) * self.F * self.hb)
        if self.clients:
            eng.ctx.demod_batch(eng.frame_num)
        if self.waterfalls:
            eng.ctx.waterfall_batch(eng.frame_num)
        eng.frame_num += self.F

    def sync(self):
        self.eng.ctx.synchronize()
        self.torch.cuda.synchronize()

    def timed_block(self, steps, warmup):
        """The headline's timing: `warmup` untimed steps, then ONE block of exactly `steps` uninstrumented steps between two
        full synchronisations.  Returns the block's wall time (seconds)."""
        self.eng.ctx.set_profiling(0)
        for i in range(warmup):
            self.step(i)
        self.sync()
        t0 = time.perf_counter()
        for i in range(steps):
            self.step(warmup + i)
        self.sync()
        dt = time.perf_counter() - t0
        self.next_step = warmup + steps
        return dt

    def dump_outputs(self, out_dir):
        """--dump-outputs: what the last step handed its caller, as float32 DIR/<name>.npy - the spectrum and the int8 pyramid
        of DUMP_FRAMES frames of the batch drawn with DUMP_SEED, every audio client's audio rows, power and NaN flags, every
        waterfall client's rows (flattened, in client order).  An array longer than its DUMP_CAPS entry is replaced by the
        entries at a sorted sample of its flat indices drawn with DUMP_SEED: the same for the same shape, run after run."""
        ctx, F = self.eng.ctx, self.F
        rng = np.random.default_rng(DUMP_SEED)
        frames = np.sort(rng.choice(F, size=min(DUMP_FRAMES, F), replace=False))
        out = {"spectrum": np.stack([ctx.read_spectrum(int(f)).view(np.float32) for f in frames]),
               "pyramid": np.stack([ctx.read_quantized(int(f)) for f in frames])}
        if self.eng.audio_clients:
            got = [c.read_audio(F) for c in self.eng.audio_clients]
            out["audio"] = np.stack([g[0] for g in got])
            out["audio_power"] = np.stack([g[1] for g in got])
            out["audio_nan"] = np.stack([g[2] for g in got])
        if self.eng.waterfall_clients:
            out["waterfall"] = np.concatenate([w.read_waterfall()[0].reshape(-1) for w in self.eng.waterfall_clients])
        os.makedirs(out_dir, exist_ok=True)
        total = 0
        for name, a in out.items():
            a = a.astype(np.float32)
            if a.size > DUMP_CAPS[name]:
                idx = np.sort(np.random.default_rng(DUMP_SEED).choice(a.size, DUMP_CAPS[name], replace=False))
                a = a.reshape(-1)[idx]
            np.save(os.path.join(out_dir, name + ".npy"), a)
            total += a.nbytes
        assert total <= 64 * 10 ** 6, total
        return {"frames": [int(f) for f in frames], "arrays": sorted(out), "bytes": total}

    def timed(self, steps, warmup, min_reps=5, min_total_s=1.0, max_reps=40):
        """`warmup` untimed steps, then repetitions of EXACTLY `steps` steps, each bracketed by a full
        synchronisation; at least `min_reps` and until `min_total_s` of timed work.  Returns the
        per-repetition wall times (seconds) of the UNINSTRUMENTED repetitions: those are what `value` is taken from.
        Interleaved with them run repetitions with psdr_set_profiling(2) - the two FFT passes stamp the device clock at
        their first work-group's entry and their last work-group's exit (a vmcnt(0), a barrier and two atomics per
        work-group and launch; no events, no marker packets) - which give the per-kernel durations of the roofline
        block on the same box in the same minute (`self.clock_us`), and their own wall times (`self.times_stamped`):
        the two medians side by side are the price of the instrumentation."""
        ctx = self.eng.ctx
        for i in range(warmup):
            self.step(i)
        self.sync()
        ctx.set_profiling(2)
        ctx.reset_kernel_stats()
        ctx.set_profiling(0)
        times, stamped, k = [], [], warmup
        n_st_max = max(1, 8000 // max(steps, 1))  # the stamp ring holds 8192 launches per pass between two resets
        rep = 0
        while len(times) < min_reps or (sum(times) < min_total_s and len(times) < max_reps):
            instrumented = rep % 3 == 2 and len(stamped) < n_st_max  # every third repetition carries the stamps
            rep += 1
            ctx.set_profiling(2 if instrumented else 0)
            self.sync()
            t0 = time.perf_counter()
            for i in range(steps):
                self.step(k + i)
            self.sync()
            (stamped if instrumented else times).append(time.perf_counter() - t0)
            k += steps
        if not stamped:  # (short runs: min_reps < 3)
            ctx.set_profiling(2)
            self.sync()
            t0 = time.perf_counter()
            for i in range(steps):
                self.step(k + i)
            self.sync()
            stamped.append(time.perf_counter() - t0)
            k += steps
        ctx.set_profiling(2)
        self.clock_us = {name: ctx.kernel_samples(name) for name in ("fft_pass1", "fft_pass2")}
        ctx.set_profiling(0)
        self.times_stamped = stamped
        self.next_step = k
        return times

    def summary(self, times, steps):
        med = float(np.median(times))
        frames = steps * self.F
        ab = algorithmic_bytes_per_frame(self.wl, self.params, self.clients, self.waterfalls)
        out = {"value": round(frames * (self.N // 2) / med / 1e6, 2), "ms_per_step": round(med / steps * 1e3, 4),
               "frames_per_s": round(frames / med, 1), "frac_of_hbm_peak": round(ab["total"] * frames / med / HBM_PEAK, 4),
               "algorithmic_bytes_per_frame": int(ab["total"]), "repetitions": len(times),
               "ms_per_step_min_max": [round(min(times) / steps * 1e3, 4), round(max(times) / steps * 1e3, 4)],
               "timed_s": round(sum(times), 3)}
        # SURVEY 8d, supplementary: what THIS design moves - the compulsory bytes plus the inter-pass array Y written and read
        # once (8 B per point of the N- or N/2-point complex transform) - against the copy rate the survey measured on MI355X
        y_pts = self.N // 2 if self.wl["is_real"] else self.N
        tp = ab["total"] + 16 * y_pts
        out["two_pass_model"] = {"bytes_per_frame": int(tp), "GB_per_s": round(tp * frames / med / 1e9, 1),
                                 "frac_of_measured_copy_6290_GB_per_s": round(tp * frames / med / COPY_CEILING, 4)}
        st = getattr(self, "times_stamped", None)
        if st:
            out["instrumentation"] = {"value_from": "repetitions with psdr_set_profiling(0)",
                                      "ms_per_step_uninstrumented": out["ms_per_step"],
                                      "ms_per_step_with_device_clock_stamps": round(float(np.median(st)) / steps * 1e3, 4),
                                      "stamped_repetitions": len(st)}
        clk = getattr(self, "clock_us", None) or {}
        if all(len(clk.get(k, ())) for k in ("fft_pass1", "fft_pass2")):
            # the two passes on the device clock, from the timed loop itself; pass 2 (IQ and fused real alike)
            # finishes the spectrum and the pyramid: those are its algorithmic bytes
            p1, p2 = float(np.median(clk["fft_pass1"])), float(np.median(clk["fft_pass2"]))
            fused = not self.wl["is_real"] or self.wl["fft_size"] >= (1 << 21)
            out["passes_device_clock_us"] = {"fft_pass1": round(p1, 2), "fft_pass2": round(p2, 2)}
            if fused:
                out["pass2_frac_of_hbm_peak"] = round((ab["spectrum"] + ab["pyramid"]) * self.F / (p2 * 1e-6) / HBM_PEAK, 4)
        # the same block as the headline's: `frac` = B_frame x frames/s / 8 TB/s, the second pass on its own bytes beside it
        out["roofline"] = dict(path_roofline(ab["total"], frames / med), kernel="fft_pass2", kernel_frac=out.get("pass2_frac_of_hbm_peak"))
        return out

    def close(self):
        self.eng.close()
        self.ring = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=0,
                    help="frames per step (F); default 512 (DEFAULT_BATCH): a step of the two persistent passes has ~60 us of "
                         "fixed cost (ramp, prologue, tail, launch gaps) whatever F is (docs/history.md section 5, batch-size table)")
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="after the headline, everything else the line can carry: repetitions with device-clock stamps, "
                         "per-kernel replay, post chain, served end, the other workloads, client scaling, the C group leg, "
                         "the CPU baseline (N > 1: every sharding); without it a run sets up, warms up, times --steps steps "
                         "and prints the headline")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last step computed as DIR/<name>.npy (float32; N = 1 only)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-post-chain", action="store_true",
                    help="skip the separate post-demodulation-chain measurement (used for the rocprofv3 kernel stats: "
                         "its passes overlap the long chain kernels and would skew the per-kernel averages)")
    ap.add_argument("--no-extra", action="store_true",
                    help="skip the clients256 / cfg3 sub-objects (profiling runs of one workload)")
    ap.add_argument("--ring-mib", type=int, default=512)
    ap.add_argument("--shard", default=None, choices=["clients", "clients_pipelined", "time", "raw", "band"],
                    help="N > 1: which sharding `value` reports (default: clients = BASELINE.json configs[3], RCCL spectrum broadcast; "
                         "every other sharding is measured and reported beside it): "
                         "shard the clients with a spectrum broadcast (BASELINE.json configs[3]), "
                         "the clients with a RAW half-frame broadcast + replicated FFT, the clients by frequency band "
                         "with a scatter of one band per rank, or the stream (no collective)")
    ap.add_argument("--force-sharded", action="store_true",
                    help="run the multi-GPU code path even with one rank (testing)")
    ap.add_argument("--cpu-baseline-only", default=None, metavar="WORKLOAD",
                    help="(internal) run only the CPU baseline leg of a workload and print its JSON")
    ap.add_argument("--cpu-builtin-fft", action="store_true", help="(internal) CPU leg with the oracle's own FFT")
    ap.add_argument("--cpu-threaded-only", default=None, metavar="WORKLOAD",
                    help="(internal) one CPU pipeline with the FFT library's own threads (--cpu-threads)")
    ap.add_argument("--cpu-threads", type=int, default=8)
    ap.add_argument("--cpu-clients", type=int, default=None, help="(internal) audio clients of the CPU leg (N > 1: the whole job's)")
    ap.add_argument("--c-group-only", type=int, default=0, metavar="NGPUS",
                    help="(internal) ONE process over NGPUS devices through psdr_group_* (RCCL called by the library): prints its JSON")
    args = ap.parse_args()

    if args.cpu_baseline_only:
        from phantomsdr_amd.core import derived_params
        wl = WORKLOADS[args.cpu_baseline_only]
        p = derived_params(wl["sps"], wl["fft_size"], wl["is_real"])
        cl = make_clients(wl, p, seed=0x5D5D0002, count=args.cpu_clients)
        wf = make_waterfalls(wl, p, seed=0x5D5D0002)
        # (PSDR_BENCH_CPU_BUDGET_S: the orchestration tests shorten the sample; the default is the ~20 s the contract asks for)
        print(json.dumps(cpu_baseline(wl, p, cl, wf, budget_s=float(os.environ.get("PSDR_BENCH_CPU_BUDGET_S", "22")),
                                      fft_library="" if args.cpu_builtin_fft else None)), flush=True)
        return

    if args.cpu_threaded_only:
        from oracle import oracle as O
        wl = WORKLOADS[args.cpu_threaded_only]
        p = O.derived_params(wl["sps"], wl["fft_size"], wl["is_real"])
        print(json.dumps(cpu_threaded_pipeline(wl, p, args.cpu_threads)), flush=True)
        return

    if args.c_group_only:
        print(json.dumps(c_group_bench(args.c_group_only, max(args.steps, 1), args.warmup, args.batch or DEFAULT_BATCH, args.ring_mib)), flush=True)
        return

    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    if args.dump_outputs and (args.gpus > 1 or args.force_sharded):
        raise SystemExit("--dump-outputs writes the one-GPU path's outputs: use it with --gpus 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: become N ranks (one process per GPU over RCCL) by re-executing
        # under torch.distributed.run, exactly the command line the driver would have written
        return self_launch(args.gpus)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world > 1 and args.gpus == 1:
            args.gpus = world  # launched by torchrun without --gpus: the launcher's world size is the run
        else:
            raise SystemExit(f"--gpus {args.gpus} but the launcher started {world} rank(s): refusing to report a "
                             f"{world}-GPU run as a {args.gpus}-GPU one")
    if args.batch <= 0:
        args.batch = DEFAULT_BATCH
    if args.dump_outputs and world > 1:
        raise SystemExit("--dump-outputs writes the one-GPU path's outputs: use it with --gpus 1")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    if os.environ.get("PSDR_BENCH_ONE_DEVICE") == "1":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)

    if world > 1 or args.force_sharded:
        return run_sharded_bench(args, torch, rank, world, local_rank)

    wl_name = args.workload or "cfg2"
    wl = WORKLOADS[wl_name]
    F = args.batch
    run = SingleGpuRun(torch, device, local_rank, wl_name, wl, F, args.ring_mib)
    eng, params, clients, waterfalls, N = run.eng, run.params, run.clients, run.waterfalls, run.N
    # `value` and `ms_per_step`: ONE uninstrumented block of exactly --steps steps after --warmup
    head = run.summary([run.timed_block(args.steps, args.warmup)], args.steps)
    dumped = run.dump_outputs(args.dump_outputs) if args.dump_outputs else None
    timing = (f"one uninstrumented block of exactly {args.steps} steps after {args.warmup} warm-up steps, bracketed by full "
              "synchronisations; inputs resident in HBM before, results (spectrum, pyramid, audio, waterfall rows) resident in "
              "HBM after: the device-to-host copy of the results is NOT in the timed region")
    if not args.full:
        out = {
            "metric": "ingest MSamples/s + concurrent audio clients at 2^20-pt FFT",
            "value": head["value"], "unit": "MSamples/s", "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": head["ms_per_step"], "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": wl_name + ": " + wl["desc"], "frames_per_step": F,
                       "fft_size": N, "audio_clients": len(clients), "waterfall_clients": len(waterfalls),
                       "audio_fft_size": params["audio_fft_size"], "ring_MiB": round(run.nhalves * run.hb / 2 ** 20, 1),
                       "realtime_factor": round(head["value"] * 1e6 / wl["sps"], 1), "timing": timing},
            "roofline": head["roofline"],
            "path": {"algorithmic_bytes_per_frame": head["algorithmic_bytes_per_frame"], "frames_per_s": head["frames_per_s"],
                     "frac_of_hbm_peak": head["frac_of_hbm_peak"], "two_pass_model": head.get("two_pass_model")},
            "dumped_outputs": dumped,
        }
        run.close()
        emit(out)
        return

    # --full: repetitions of exactly K steps, >= 3 s of them (a 5-second utilisation sampler around the run should see the
    # GPU busy at least once); every third carries the passes' device-clock stamps
    times = run.timed(args.steps, args.warmup, min_total_s=3.0, max_reps=400)
    reps = run.summary(times, args.steps)

    # per-kernel durations: profiled replay of the same steps (the events do not perturb `value`)
    roofline, kernels, ab = kernel_roofline(eng.ctx, run.step, run.next_step, 50, wl, wl_name, params,
                                            clients, waterfalls, F, clock_us=run.clock_us, ms_per_step=reps["ms_per_step"],
                                            ms_per_step_stamped=(reps.get("instrumentation") or {}).get("ms_per_step_with_device_clock_stamps"),
                                            frames_per_s=head["frames_per_s"])

    # SURVEY 8f-2 (widened row): the optional post-demodulation chain (DC blocker + AGC + int16),
    # measured separately - it is NOT part of `value` (the metric's clients end at float audio)
    post = None
    if clients and not args.no_post_chain:
        post = post_chain_measure(run, eng, params, wl, F, N, len(clients), reps["ms_per_step"])
    served = None
    if clients and not args.no_extra:
        served = with_fetch_measure(run, eng, params, wl, F, N, len(clients), reps["ms_per_step"], post)
    nhalves, hb = run.nhalves, run.hb
    run.close()
    del run

    # more of BASELINE.json's single-GPU shapes, each with its own value and whole-path fraction:
    # the target's own wording (256 concurrent audio clients on one MI355X), configs[2] and one GPU's
    # share of configs[4] (2^22-point real frames, 128 of the 1024 clients + 8 of the 64 waterfalls)
    extra = {}
    if not args.no_extra and wl_name == "cfg2":
        for key, name, nc in (("clients256", "cfg2", 256), ("cfg3", "cfg3", None), ("cfg5_share", "cfg5", None)):
            try:
                w2 = WORKLOADS[name] if nc is None else dict(WORKLOADS[name], modes=("USB", "LSB", "AM", "FM"))
                r2 = SingleGpuRun(torch, device, local_rank, name, w2, F, args.ring_mib, nclients=nc)
                st = min(args.steps, 25 if name == "cfg5" else 50)
                sm = r2.summary(r2.timed(st, min(args.warmup, 5), min_reps=3, min_total_s=0.3), st)
                sm.update({"workload": (name + ": " + w2["desc"]) if nc is None else
                           f"cfg2 shape with {nc} mixed USB/LSB/AM/FM audio clients + {w2['waterfall']} waterfall clients on one GPU",
                           "audio_clients": len(r2.clients), "steps": st,
                           "realtime_factor": round(sm["value"] * 1e6 / w2["sps"], 1)})
                if nc is not None and not args.no_post_chain:  # the chain with all 64 lanes of four waves in use
                    sm["post_chain"] = post_chain_measure(r2, r2.eng, r2.eng.params, w2, F, w2["fft_size"], len(r2.clients), sm["ms_per_step"])
                if nc is not None:  # the served end at the target's 256 clients: ~95 MB of results per step to the host
                    sm["with_fetch"] = with_fetch_measure(r2, r2.eng, r2.eng.params, w2, F, w2["fft_size"], len(r2.clients), sm["ms_per_step"],
                                                          sm.get("post_chain"))
                extra[key] = sm
                r2.close()
                del r2
            except Exception as e:
                extra[key] = {"error": repr(e)}

    # Where does demodulation overtake the passes on REAL input?  cfg3's stream (2^21-point R2C) with 1024 mixed clients
    # attached, of which all but the first k sit out (psdr_client_set_paused): the same context, ring and launch shapes
    # for every k.  (The consumers of a batch run beside the next batch's passes; alone on the chip the demodulation of
    # 64 / 128 clients x 256 frames takes 75 / 205 us - tools/consumers_alone.py, profiles/r04_consumers_*.)
    scaling = None
    if not args.no_extra and wl_name == "cfg2":
        try:
            w3 = dict(WORKLOADS["cfg3"])
            r3 = SingleGpuRun(torch, device, local_rank, "cfg3", w3, F, args.ring_mib, nclients=1024)
            all_clients = list(r3.clients)
            scaling = {"workload": "cfg3 stream (70 MSPS real s16, 2^21-pt R2C), k of 1024 attached mixed AM/FM/SSB clients demodulated, the rest paused",
                       "frames_per_step": F, "by_clients": {}}
            for k in (64, 256, 512, 1024):
                for i, c in enumerate(r3.eng.audio_clients):
                    c.set_paused(i >= k)
                r3.clients = all_clients[:k]
                sm = r3.summary(r3.timed(20, 3, min_reps=3, min_total_s=0.25), 20)
                scaling["by_clients"][str(k)] = {kk: sm[kk] for kk in ("value", "ms_per_step", "frac_of_hbm_peak", "passes_device_clock_us") if kk in sm}
            r3.close()
            del r3
        except Exception as e:
            scaling = {"error": repr(e)}

    # SURVEY 8e from C on this box's one GPU: psdr_group_* with the communicator and the collectives forced (a child
    # process: RCCL stays out of this one) - shows that the library's own RCCL path runs here; its rates mean nothing
    # (a broadcast to oneself).  The N > 1 line carries the real thing (`c_group`).
    c_group = None
    if not args.no_extra and wl_name == "cfg2":
        import subprocess
        try:
            rr = subprocess.run([sys.executable, os.path.abspath(__file__), "--c-group-only", "1", "--steps", "5", "--warmup", "2",
                                 "--batch", str(F)], capture_output=True, text=True, timeout=180)
            line = [ln for ln in rr.stdout.splitlines() if ln.startswith("{")]
            c_group = json.loads(line[-1]) if line else {"error": (rr.stderr or "")[-400:]}
        except Exception as e:
            c_group = {"error": repr(e)}

    cpu = None
    if not args.no_cpu_baseline:
        cpu = cpu_baseline_subprocess(wl_name)

    out = {
        "metric": "ingest MSamples/s + concurrent audio clients at 2^20-pt FFT",
        "value": head["value"], "unit": "MSamples/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": head["ms_per_step"], "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": wl_name + ": " + wl["desc"], "frames_per_step": F,
                   "fft_size": N, "audio_clients": len(clients), "waterfall_clients": len(waterfalls),
                   "audio_fft_size": params["audio_fft_size"], "ring_MiB": round(nhalves * hb / 2 ** 20, 1),
                   "realtime_factor": round(head["value"] * 1e6 / wl["sps"], 1),
                   "timing": timing + " - `with_fetch` (and clients256.with_fetch) time the same step WITH it, overlapped "
                             "with the next step; path.repetitions: the same step in repetitions of exactly that many steps "
                             f"({reps['repetitions']} UNINSTRUMENTED ones, {reps['timed_s']} s timed), every third repetition of "
                             "that loop carrying the passes' device-clock stamps instead (mode 2; path.instrumentation has both "
                             "medians)"},
        "roofline": roofline,
        "path": {"algorithmic_bytes_per_frame": head["algorithmic_bytes_per_frame"], "frames_per_s": head["frames_per_s"],
                 "frac_of_hbm_peak": head["frac_of_hbm_peak"], "two_pass_model": head.get("two_pass_model"),
                 "repetitions": {"ms_per_step_median": reps["ms_per_step"], "count": reps["repetitions"],
                                 "timed_s": reps["timed_s"], "value": reps["value"]},
                 "ms_per_step_min_max": reps["ms_per_step_min_max"],
                 "instrumentation": reps.get("instrumentation"), "kernels": kernels},
        "dumped_outputs": dumped,
        "clients256": extra.get("clients256"),
        "cfg3": extra.get("cfg3"),
        "cfg5_share": extra.get("cfg5_share"),
        "real_input_client_scaling": scaling,
        "c_group_single_device_plumbing": c_group,
        "post_chain": post,
        "with_fetch": served,
        "cpu_baseline": cpu,
    }
    emit(out)


if __name__ == "__main__":
    main()

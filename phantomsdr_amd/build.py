"""Builds libpsdr_hip.so (gfx950) in-tree with hipcc: one object per translation unit of csrc/ (compiled in parallel),
one link.  Cross-compiles without a GPU."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# context: lifetime / Level 1 / ingest / instrumentation; pass1, pass2: the FFT pass launchers; forward: the frame loop,
# read-back, band layout, waterfall; demod: audio clients; fetch: the served end, results to host memory; postchain: DC blocker /
# AGC / int16; audiofilter: the per-client biquad cascade behind the detector; group: n GPUs from one process over RCCL; wire: packet formats; blanker: the impulse blanker on the ingest ring
UNITS = ["context", "pass1", "pass2", "forward", "demod", "fetch", "postchain", "group", "wire", "blanker", "audiofilter", "nr", "anb", "scan", "tone", "cw", "rtty", "psk", "fax"]  # fax: the per-client radiofax decoder at the same reading point; psk: the per-client PSK31 decoder at the same reading point; rtty: the per-client RTTY decoder at the same reading point; cw: the per-client CW decoder at the tone decoder's reading point; tone: the per-client tone decoder on the rows as the demodulator wrote them; scan: the band scan behind a batch (trace, segment floors, list of signals); nr: the per-client noise reduction in front of the audio filter; anb: the per-client audio blanker in front of it
OUT = os.path.join(_HERE, "libpsdr_hip.so")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-fPIC"]


def sources():
    inc = os.path.join(_HERE, "..", "include", "psdr.h")
    return [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))] + [inc]


def is_stale():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(s) > t for s in sources())


def build_extension(force=False, verbose=False, out=None, defines=(), extra=()):
    """hipcc --offload-arch=gfx950 ... -> phantomsdr_amd/libpsdr_hip.so (or `out`, e.g. a tuning variant)"""
    out = out or OUT
    if not force and out == OUT and not is_stale():
        return OUT
    objdir = os.path.join(_HERE, "..", "build", "obj", os.path.splitext(os.path.basename(out))[0])
    os.makedirs(objdir, exist_ok=True)
    dflags = [f"-D{d}" for d in defines] + list(extra)

    def one(u):
        obj = os.path.join(objdir, u + ".o")
        cmd = [HIPCC] + FLAGS + dflags + ["-c", os.path.join(CSRC, u + ".hip"), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        return obj

    with ThreadPoolExecutor(min(len(UNITS), os.cpu_count() or 4)) as ex:
        objs = list(ex.map(one, UNITS))
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    print(build_extension(force=True, verbose=True))

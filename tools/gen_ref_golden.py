#!/usr/bin/env python
"""Records what the reference's own compiled helpers (oracle/_ref/libref_dsp.so, built by `make -C oracle ref` where the
reference tree exists) return for the inputs of tests/test_oracle_ref.py, as SHA-256 digests of their output bytes, in
tests/golden/ref_dsp_sha256.json - so that the oracle stays pinned to them on machines without the reference tree.

  python tools/gen_ref_golden.py        # rewrites tests/golden/ref_dsp_sha256.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_oracle_ref as T  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    R = O.ref()
    if R is None:
        raise SystemExit("oracle/_ref/libref_dsp.so is not built (make -C oracle ref needs the reference tree)")
    rec = {"source": "oracle/_ref/libref_dsp.so: the reference's src/utils/dsp.cpp + audioprocessing.cpp, "
                     "inputs as drawn in tests/test_oracle_ref.py; sha256 of each output array's bytes",
           "inputs": T.input_digests(),
           "outputs": {k: T.digest(v) for k, v in T.ref_outputs(R).items()}}
    with open(T.GOLDEN_PATH, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{T.GOLDEN_PATH}: {len(rec['outputs'])} outputs")


if __name__ == "__main__":
    main()

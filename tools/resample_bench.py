"""Time of the launch an admission issues in its staging step (hipEvents around the launch, median of --iters after three
warm-up launches: sc_stage_bench) for 128 chunks of 640 ms each: the sample-rate conversion at 48000, 44100 and 8000 Hz
(streams in mid-utterance: the history is read and left) and, beside them, the plain scatter copy a 16 kHz admission pays
for the same 128 x 10240 output samples.  One JSON line per case with the bytes the launch has to move (input + output +
coefficient table).  Kernel times: run it under `rocprofv3 --kernel-trace --stats` in a run of its own.

    python tools/resample_bench.py [--iters 20] [--jobs 128] [--rates 48000 44100 8000]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechcatcher_amd import _abi  # noqa: E402
from speechcatcher_amd.resample import out_count, rate_params  # noqa: E402


def bench(lib, rate, jobs, iters):
    n_in = int(0.64 * rate)
    ms = np.zeros(iters, np.float64)
    _abi.check(lib.sc_stage_bench(rate, jobs, n_in, iters, ms.ctypes.data_as(_abi.c_double_p)), "sc_stage_bench")
    L, M, Wc = rate_params(rate)
    n_out = n_in if rate == 16000 else out_count(rate, 4 * n_in, False) - out_count(rate, 3 * n_in, False)
    table = 0 if rate == 16000 else L * 2 * Wc * 4
    nbytes = jobs * (n_in + n_out) * 4 + table
    med = float(np.median(ms))
    return {"rate": rate, "kernel": "scatter_f32_kernel" if rate == 16000 else "resample_kernel", "jobs": jobs,
            "n_in": n_in, "n_out": n_out, "taps": 0 if rate == 16000 else 2 * Wc, "phases": L,
            "ms_median": round(med, 4), "ms_min": round(float(ms.min()), 4), "ms_max": round(float(ms.max()), 4),
            "bytes": nbytes, "table_bytes": table, "GB_per_s": round(nbytes / (med * 1e-3) / 1e9, 1),
            "iters": iters, "source": "hipEvent around the launch (sc_stage_bench)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--jobs", type=int, default=128)
    ap.add_argument("--rates", type=int, nargs="*", default=[48000, 44100, 8000])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs a ROCm GPU")
    lib = _abi.load()
    for rate in list(args.rates) + [16000]:
        print(json.dumps(bench(lib, rate, args.jobs, args.iters)), flush=True)


if __name__ == "__main__":
    main()

"""Time of one sc_ctc_align launch pair (per-row logsumexp + one wave per job) for a batch of alignments, by hipEvents
around the launches.  The two shapes of the alignment feature's measurements: 128 jobs at T = 790, L = 400 (a
stream of the headline window, best hypothesis) and 128 jobs at T = 4800, L = 1000 (a three-minute CLI segment).
Prints one JSON line per shape.  Kernel times: run it under `rocprofv3 --kernel-trace --stats` in a run of its own.

    python tools/align_bench.py [--iters 20] [--jobs 128]
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


def bench(n, T, L, V, iters, lib):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(T * 7 + L)
    emis = (torch.randn((n, T, V), generator=g) * 4).to(dev)
    labels = (torch.randint(1, V, (n, L), generator=g, dtype=torch.int32)).to(dev)
    ws_b = (int(lib.sc_ctc_align_ws_bytes(T)) + 255) // 256 * 256
    ws = torch.empty(n * ws_b, dtype=torch.uint8, device=dev)
    out_i = torch.empty((n, 2, L), dtype=torch.int32, device=dev)
    out_f = torch.empty((n, L), dtype=torch.float32, device=dev)
    ps = torch.empty(n, dtype=torch.float32, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    tab = (_abi.AlignJob * n)()
    for k in range(n):
        j = tab[k]
        j.emis, j.labels, j.ws = emis[k].data_ptr(), labels[k].data_ptr(), ws.data_ptr() + k * ws_b
        j.start, j.end, j.logp_mean = out_i[k, 0].data_ptr(), out_i[k, 1].data_ptr(), out_f[k].data_ptr()
        j.path_score, j.status = ps[k].data_ptr(), st[k].data_ptr()
        j.stride, j.T, j.L, j.V, j.blank = V, T, L, V, 0
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
    s = torch.cuda.current_stream(dev)

    def launch():
        _abi.check(lib.sc_ctc_align(tab_dev.data_ptr(), n, T, L, s.cuda_stream), "sc_ctc_align")

    for _ in range(3):
        launch()
    torch.cuda.synchronize(dev)
    assert int((st != 0).sum()) == 0, st.cpu().numpy()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        launch()
        b.record(s)
        b.synchronize()
        times.append(a.elapsed_time(b))
    t = np.array(times)
    return {"jobs": n, "T": T, "L": L, "V": V, "ms_median": round(float(np.median(t)), 4),
            "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4), "iters": iters,
            "source": "hipEvent around sc_ctc_align (both launches)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--jobs", type=int, default=128)
    ap.add_argument("--vocab", type=int, default=1024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("align_bench needs a ROCm GPU")
    lib = _abi.load()
    for T, L in ((790, 400), (4800, 1000)):
        print(json.dumps(bench(args.jobs, T, L, args.vocab, args.iters, lib)), flush=True)


if __name__ == "__main__":
    main()

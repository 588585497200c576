"""Time of one sc_ctc_activity launch (one workgroup per job: float64 blank posteriors of the job's CTC rows, then the
speech / silence scan) by hipEvents around the launch.  The shapes are the headline regime's admission groups: 58 and 128
jobs of 16 rows at V = 1024.  Before every timed launch the rows are written again by a device copy, as the CTC GEMM
of the group would have just done: the launch reads them from L2 / Infinity Cache.  Prints one JSON line per shape,
with the median duration of an empty event pair on the same stream (the bias of the bracketing).

    python tools/activity_bench.py [--iters 20] [--rows 16] [--vocab 1024]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechcatcher_amd import _abi  # noqa: E402


def bench(n, rows, V, iters, lib, tcap=256):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(n * 131 + rows)
    src = (torch.randn((n, rows, V), generator=g) * 4)
    src[:, :, 0] += 9.0                                  # blank posteriors on both sides of the threshold
    src = src.to(dev)
    table = torch.zeros((n, tcap, V), dtype=torch.float32, device=dev)
    t0 = 40
    state = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    after = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    track = torch.zeros((n, tcap), dtype=torch.float64, device=dev)
    tab = (_abi.ActivityJob * n)()
    for k in range(n):
        j = tab[k]
        j.table, j.state, j.track, j.state_after = table[k].data_ptr(), state[k].data_ptr(), track[k].data_ptr(), after[k].data_ptr()
        j.stride, j.thr, j.V, j.blank, j.t0, j.t1, j.restart = V, 0.8, V, 0, t0, t0 + rows, 1
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
    s = torch.cuda.current_stream(dev)

    def launch():
        _abi.check(lib.sc_ctc_activity(tab_dev.data_ptr(), n, s.cuda_stream), "sc_ctc_activity")

    for _ in range(3):
        table[:, t0:t0 + rows].copy_(src)
        launch()
    torch.cuda.synchronize(dev)
    st = after.cpu().numpy()
    assert (st[:, 0] == rows).all() and (st[:, 2] == 0).all(), st
    times = []
    for _ in range(iters):
        table[:, t0:t0 + rows].copy_(src)                # the rows have just been written
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        launch()
        b.record(s)
        b.synchronize()
        times.append(a.elapsed_time(b))
    t = np.array(times)
    return {"jobs": n, "rows_per_job": rows, "V": V, "us_median": round(float(np.median(t)) * 1e3, 2),
            "us_min": round(float(t.min()) * 1e3, 2), "us_max": round(float(t.max()) * 1e3, 2), "iters": iters,
            "speech_frames": int(st[:, 1].sum()), "frames": int(st[:, 0].sum()),
            "us_empty_event_pair": round(float(lib.sc_prof_event_overhead_ms(s.cuda_stream)) * 1e3, 2),
            "source": "hipEvent around one sc_ctc_activity launch, rows rewritten before it"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--vocab", type=int, default=1024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("activity_bench needs a ROCm GPU")
    lib = _abi.load()
    for n in (58, 128):
        print(json.dumps(bench(n, args.rows, args.vocab, args.iters, lib)), flush=True)


if __name__ == "__main__":
    main()

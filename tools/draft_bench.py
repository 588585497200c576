"""Time of one sc_ctc_draft launch (one workgroup per job: label and float64 posterior of the job's CTC rows, then the
greedy collapse) by hipEvents around the launch, with the sc_ctc_activity launch over the same rows and an empty event
pair beside it in the same session.  The shapes are the headline regime's admission groups: 58 and 128 jobs of 16 rows
at V = 1024.  Before every timed launch the rows are written again by a device copy, as the CTC GEMM of the group would
have just done: the launch reads them from L2 / Infinity Cache.  Prints one JSON line per shape.

    python tools/draft_bench.py [--iters 20] [--rows 16] [--vocab 1024]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechcatcher_amd import _abi  # noqa: E402


def _timed(launch, rewrite, iters, s):
    times = []
    for _ in range(iters):
        rewrite()                                            # the rows have just been written
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        launch()
        b.record(s)
        b.synchronize()
        times.append(a.elapsed_time(b))
    t = np.array(times) * 1e3
    return round(float(np.median(t)), 2), round(float(t.min()), 2), round(float(t.max()), 2)


def bench(n, rows, V, iters, lib, tcap=256):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(n * 131 + rows)
    src = (torch.randn((n, rows, V), generator=g) * 4)
    src[:, :, 0] += 9.0                                  # the blank leads about half of the frames: tokens open and close
    src = src.to(dev)
    table = torch.zeros((n, tcap, V), dtype=torch.float32, device=dev)
    t0 = 40
    # draft: state 32 bytes, tokens 24 bytes each
    d_state = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    d_after = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    d_tokens = torch.zeros((n, tcap, 24), dtype=torch.uint8, device=dev)
    dtab = (_abi.DraftJob * n)()
    for k in range(n):
        j = dtab[k]
        j.table, j.state, j.tokens, j.state_after = (table[k].data_ptr(), d_state[k].data_ptr(), d_tokens[k].data_ptr(),
                                                     d_after[k].data_ptr())
        j.stride, j.V, j.blank, j.t0, j.t1, j.restart, j.capacity = V, V, 0, t0, t0 + rows, 1, tcap
    dtab_dev = torch.frombuffer(bytearray(bytes(dtab)), dtype=torch.uint8).to(dev)
    # activity over the same rows
    a_state = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    a_after = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    track = torch.zeros((n, tcap), dtype=torch.float64, device=dev)
    atab = (_abi.ActivityJob * n)()
    for k in range(n):
        j = atab[k]
        j.table, j.state, j.track, j.state_after = table[k].data_ptr(), a_state[k].data_ptr(), track[k].data_ptr(), a_after[k].data_ptr()
        j.stride, j.thr, j.V, j.blank, j.t0, j.t1, j.restart = V, 0.8, V, 0, t0, t0 + rows, 1
    atab_dev = torch.frombuffer(bytearray(bytes(atab)), dtype=torch.uint8).to(dev)
    s = torch.cuda.current_stream(dev)

    def draft():
        _abi.check(lib.sc_ctc_draft(dtab_dev.data_ptr(), n, s.cuda_stream), "sc_ctc_draft")

    def activity():
        _abi.check(lib.sc_ctc_activity(atab_dev.data_ptr(), n, s.cuda_stream), "sc_ctc_activity")

    def rewrite():
        table[:, t0:t0 + rows].copy_(src)

    for _ in range(3):
        rewrite()
        draft()
        activity()
    torch.cuda.synchronize(dev)
    st = d_after.cpu().numpy().view(np.int32).reshape(n, 8)
    assert (st[:, 0] == rows).all() and (st[:, 2] == 0).all(), st
    assert (a_after.cpu().numpy()[:, 0] == rows).all()
    d = _timed(draft, rewrite, iters, s)
    a = _timed(activity, rewrite, iters, s)
    return {"jobs": n, "rows_per_job": rows, "V": V, "us_median": d[0], "us_min": d[1], "us_max": d[2],
            "us_activity_median": a[0], "us_activity_min": a[1], "us_activity_max": a[2], "iters": iters,
            "tokens": int(st[:, 1].sum() + (st[:, 3] >= 0).sum()), "frames": int(st[:, 0].sum()),
            "us_empty_event_pair": round(float(lib.sc_prof_event_overhead_ms(s.cuda_stream)) * 1e3, 2),
            "source": "hipEvent around one sc_ctc_draft / sc_ctc_activity launch, rows rewritten before it"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--vocab", type=int, default=1024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("draft_bench needs a ROCm GPU")
    lib = _abi.load()
    for n in (58, 128):
        print(json.dumps(bench(n, args.rows, args.vocab, args.iters, lib)), flush=True)


if __name__ == "__main__":
    main()

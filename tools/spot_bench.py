"""Time of one sc_ctc_spot launch (one workgroup per job: row maxima, the phrase recurrences, the event merge) by
hipEvents around the launch.  The shapes are the headline regime's admission groups: 58 and 128 jobs of 16 rows at
V = 1024, with P = 1, 16 and 64 phrases of L = 8 tokens.  Before every timed launch the rows are written again by a
device copy, as the CTC GEMM of the group would have just done: the launch reads them from L2 / Infinity Cache.  Prints
one JSON line per shape, with the median duration of an empty event pair on the same stream (the bias of the bracketing).
Compare with tools/activity_bench.py (the sc_ctc_activity launch over the same rows) run in the same session.

    python tools/spot_bench.py [--iters 20] [--rows 16] [--vocab 1024] [--len 8]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechcatcher_amd import _abi  # noqa: E402
from speechcatcher_amd.spotting import PhraseSet  # noqa: E402


def bench(n, rows, V, P, L, iters, lib, tcap=256):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(n * 131 + P)
    g = torch.Generator(device="cpu").manual_seed(n * 131 + rows)
    src = (torch.randn((n, rows, V), generator=g) * 4)
    phrases = [[int(t) for t in rng.choice(np.arange(1, V), size=L, replace=False)] for _ in range(P)]   # (blank 0)
    y = phrases[0]                                       # phrase 0 is said in every job: one event each
    for i in range(min(rows, L)):
        src[:, rows - min(rows, L) + i, y[L - min(rows, L) + i]] += 40.0
    src = src.to(dev)
    ps = PhraseSet(phrases, None, V, 0)
    lab, lens, flo = (torch.as_tensor(a).to(dev) for a in (ps.labels, ps.lens, ps.floors))
    table = torch.zeros((n, tcap, V), dtype=torch.float32, device=dev)
    t0 = 40
    NS, NE = _abi.SPOT_STATES, _abi.SPOT_MAX_EVENTS
    counters = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    after = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    values = torch.zeros((n, P, NS), dtype=torch.float64, device=dev)
    starts = torch.zeros((n, P, NS), dtype=torch.int32, device=dev)
    events = torch.zeros((n, NE, 6), dtype=torch.int32, device=dev)
    tab = (_abi.SpotJob * n)()
    for k in range(n):
        j = tab[k]
        j.table, j.labels, j.lens, j.floors = table[k].data_ptr(), lab.data_ptr(), lens.data_ptr(), flo.data_ptr()
        j.counters, j.values, j.starts = counters[k].data_ptr(), values[k].data_ptr(), starts[k].data_ptr()
        j.events, j.state_after = events[k].data_ptr(), after[k].data_ptr()
        j.stride, j.mask, j.V, j.blank, j.t0, j.t1, j.restart, j.P = V, (1 << 64) - 1, V, 0, t0, t0 + rows, 1, P
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
    s = torch.cuda.current_stream(dev)

    def launch():
        _abi.check(lib.sc_ctc_spot(tab_dev.data_ptr(), n, s.cuda_stream), "sc_ctc_spot")

    for _ in range(3):
        table[:, t0:t0 + rows].copy_(src)
        launch()
    torch.cuda.synchronize(dev)
    st = after.cpu().numpy()
    assert (st[:, 0] == rows).all(), st
    if rows >= L:
        assert (st[:, 1] >= 1).all(), st
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
    return {"jobs": n, "rows_per_job": rows, "V": V, "P": P, "L": L, "us_median": round(float(np.median(t)) * 1e3, 2),
            "us_min": round(float(t.min()) * 1e3, 2), "us_max": round(float(t.max()) * 1e3, 2), "iters": iters,
            "events": int(st[:, 1].sum()), "frames": int(st[:, 0].sum()),
            "us_empty_event_pair": round(float(lib.sc_prof_event_overhead_ms(s.cuda_stream)) * 1e3, 2),
            "source": "hipEvent around one sc_ctc_spot launch, rows rewritten before it"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--vocab", type=int, default=1024)
    ap.add_argument("--len", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spot_bench needs a ROCm GPU")
    lib = _abi.load()
    for n in (58, 128):
        for P in (1, 16, 64):
            print(json.dumps(bench(n, args.rows, args.vocab, P, args.len, args.iters, lib)), flush=True)


if __name__ == "__main__":
    main()

"""Time of one sc_ctc_beam launch (one workgroup per job: float64 lse and the C candidates of the job's CTC rows, then
the prefix beam search over them) by hipEvents around the launch, at (B, C) = (8, 8) and (16, 16), with the sc_ctc_draft
launch over the same rows and an empty event pair beside it in the same session.  The shapes are the headline regime's
admission groups: 58 and 128 jobs of 16 rows at V = 1024.  The jobs carry a beam in: a state of B entries from a first
launch over 40 earlier rows.  Before every timed launch the rows are written again by a device copy, as the CTC GEMM of
the group would have just done, and the carried states are put back.  Prints one JSON line per shape.

    python tools/ctc_beam_bench.py [--iters 20] [--rows 16] [--vocab 1024]
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
    t0 = 40
    src = (torch.randn((n, t0 + rows, V), generator=g) * 4)
    src[:, :, 0] += 9.0                                  # the blank leads about half of the frames: stays, extensions, merges
    src = src.to(dev)
    table = torch.zeros((n, tcap, V), dtype=torch.float32, device=dev)
    table[:, :t0 + rows].copy_(src)
    s = torch.cuda.current_stream(dev)
    SB, SN = 528, 16                                     # sizeof sc_beam_t, sc_beam_node
    out = {"jobs": n, "rows_per_job": rows, "V": V, "iters": iters}

    def jobs(B, C, a, b, restart, state, after, nodes, cap):
        tab = (_abi.BeamJob * n)()
        for k in range(n):
            j = tab[k]
            j.table, j.state, j.nodes, j.state_after = (table[k].data_ptr(), state[k].data_ptr(), nodes[k].data_ptr(),
                                                        after[k].data_ptr())
            j.stride, j.V, j.blank, j.t0, j.t1, j.restart, j.capacity, j.B, j.C = V, V, 0, a, b, restart, cap, B, C
        return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)

    for B, C in ((8, 8), (16, 16)):
        cap = 1 + B * tcap
        state = torch.zeros((n, SB), dtype=torch.uint8, device=dev)
        after = torch.zeros((n, SB), dtype=torch.uint8, device=dev)
        nodes = torch.zeros((n, cap * SN), dtype=torch.uint8, device=dev)
        first = jobs(B, C, 0, t0, 1, state, after, nodes, cap)
        span = jobs(B, C, t0, t0 + rows, 0, state, after, nodes, cap)
        _abi.check(lib.sc_ctc_beam(first.data_ptr(), n, s.cuda_stream), "sc_ctc_beam")
        torch.cuda.synchronize(dev)
        carried = state.clone()

        def launch():
            _abi.check(lib.sc_ctc_beam(span.data_ptr(), n, s.cuda_stream), "sc_ctc_beam")

        def rewrite():
            table[:, t0:t0 + rows].copy_(src[:, t0:])
            state.copy_(carried)

        for _ in range(3):
            rewrite()
            launch()
        torch.cuda.synchronize(dev)
        st = after.cpu().numpy().view(np.int32).reshape(n, SB // 4)
        assert (st[:, 0] == t0 + rows).all() and (st[:, 1] == 0).all() and (st[:, 3] == B).all(), st[:, :4]
        t = _timed(launch, rewrite, iters, s)
        out[f"us_B{B}C{C}_median"], out[f"us_B{B}C{C}_min"], out[f"us_B{B}C{C}_max"] = t
        out[f"nodes_B{B}C{C}"] = int(st[:, 2].sum())
    # the draft over the same rows
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

    def draft():
        _abi.check(lib.sc_ctc_draft(dtab_dev.data_ptr(), n, s.cuda_stream), "sc_ctc_draft")

    def rewrite_rows():
        table[:, t0:t0 + rows].copy_(src[:, t0:])

    for _ in range(3):
        rewrite_rows()
        draft()
    torch.cuda.synchronize(dev)
    d = _timed(draft, rewrite_rows, iters, s)
    out.update(us_draft_median=d[0], us_draft_min=d[1], us_draft_max=d[2],
               us_empty_event_pair=round(float(lib.sc_prof_event_overhead_ms(s.cuda_stream)) * 1e3, 2),
               source="hipEvent around one sc_ctc_beam / sc_ctc_draft launch, rows rewritten and states put back before it")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--vocab", type=int, default=1024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_beam_bench needs a ROCm GPU")
    lib = _abi.load()
    for n in (58, 128):
        print(json.dumps(bench(n, args.rows, args.vocab, args.iters, lib)), flush=True)


if __name__ == "__main__":
    main()

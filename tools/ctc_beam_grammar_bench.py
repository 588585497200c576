"""Time of one sc_ctc_beam_grammar launch (one workgroup per job: float64 lse of the job's CTC rows, then per frame the
candidates of every entry's grammar state - one wave per entry - and the prefix beam step) by hipEvents around the launch,
at (B, C) = (8, 8) and (16, 16), for three grammars: a 10-phrase menu, a looped trie of 1000 phrases (a start state of
several hundred arcs) and the free grammar (out-degree V - 1, the worst case).  The plain sc_ctc_beam launch over the same
rows and an empty event pair are timed in the same session; the ratios to the plain launch are reported.  The shapes are
those of tools/ctc_beam_bench.py: 58 and 128 jobs of 16 rows at V = 1024, the jobs carrying a beam in from a first launch
over 40 earlier rows; before every timed launch the rows are written again and the carried states are put back.  Prints
one JSON line per shape; the median of --iters launches.

    python tools/ctc_beam_grammar_bench.py [--iters 30] [--rows 16] [--vocab 1024]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechcatcher_amd import _abi, grammar  # noqa: E402
from speechcatcher_amd.hip_backend import DeviceGrammar  # noqa: E402
from tools.ctc_beam_bench import _timed  # noqa: E402


def grammars(V, seed=1):
    rng = np.random.default_rng(seed)
    toks = np.arange(1, V)
    phrases = lambda n: [[int(t) for t in rng.choice(toks, int(rng.integers(1, 7)))] for _ in range(n)]   # noqa: E731
    return {"menu10": grammar.compile(phrases(10), V, 0), "trie1000": grammar.compile(phrases(1000), V, 0),
            "free": grammar.free(V, 0)}


def bench(n, rows, V, iters, lib, blobs, tcap=256):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(n * 131 + rows)
    t0 = 40
    src = (torch.randn((n, t0 + rows, V), generator=g) * 4)
    src[:, :, 0] += 9.0                                  # the blank leads about half of the frames: stays, extensions, merges
    src = src.to(dev)
    table = torch.zeros((n, tcap, V), dtype=torch.float32, device=dev)
    table[:, :t0 + rows].copy_(src)
    s = torch.cuda.current_stream(dev)
    SB, SN, SG = 528, 16, 64                             # sizeof sc_beam_t, sc_beam_node, sc_beam_gr_t
    out = {"jobs": n, "rows_per_job": rows, "V": V, "iters": iters}
    devs = {name: DeviceGrammar(lib, blob) for name, blob in blobs.items()}
    for name, blob in blobs.items():
        gr = grammar.Grammar(blob)
        out[f"{name}_states"], out[f"{name}_start_arcs"] = gr.n_states, len(gr.arcs(gr.start_state))

    def fill(j, k, B, C, a, b, restart, state, after, nodes, cap):
        j.table, j.state, j.nodes, j.state_after = (table[k].data_ptr(), state[k].data_ptr(), nodes[k].data_ptr(),
                                                    after[k].data_ptr())
        j.stride, j.V, j.blank, j.t0, j.t1, j.restart, j.capacity, j.B, j.C = V, V, 0, a, b, restart, cap, B, C

    for B, C in ((8, 8), (16, 16)):
        cap = 1 + B * tcap
        state = torch.zeros((n, SB), dtype=torch.uint8, device=dev)
        after = torch.zeros((n, SB), dtype=torch.uint8, device=dev)
        nodes = torch.zeros((n, cap * SN), dtype=torch.uint8, device=dev)
        gstate = torch.zeros((n, SG), dtype=torch.uint8, device=dev)
        gafter = torch.zeros((n, SG), dtype=torch.uint8, device=dev)

        def plain_jobs(a, b, restart):
            tab = (_abi.BeamJob * n)()
            for k in range(n):
                fill(tab[k], k, B, C, a, b, restart, state, after, nodes, cap)
            return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)

        def grammar_jobs(a, b, restart, view):
            tab = (_abi.BeamGrJob * n)()
            for k in range(n):
                fill(tab[k].beam, k, B, C, a, b, restart, state, after, nodes, cap)
                tab[k].grammar, tab[k].gr_state, tab[k].gr_state_after = view, gstate[k].data_ptr(), gafter[k].data_ptr()
            return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)

        def one(fn, first, span, what):
            _abi.check(fn(first.data_ptr(), n, s.cuda_stream), what)
            torch.cuda.synchronize(dev)
            carried, gcarried = state.clone(), gstate.clone()

            def launch():
                _abi.check(fn(span.data_ptr(), n, s.cuda_stream), what)

            def rewrite():
                table[:, t0:t0 + rows].copy_(src[:, t0:])
                state.copy_(carried)
                gstate.copy_(gcarried)

            for _ in range(3):
                rewrite()
                launch()
            torch.cuda.synchronize(dev)
            st = after.cpu().numpy().view(np.int32).reshape(n, SB // 4)
            assert (st[:, 0] == t0 + rows).all() and (st[:, 1] == 0).all() and (st[:, 3] >= 1).all(), st[:, :4]
            return _timed(launch, rewrite, iters, s), float(st[:, 3].mean())

        (med, lo, hi), _ = one(lib.sc_ctc_beam, plain_jobs(0, t0, 1), plain_jobs(t0, t0 + rows, 0), "sc_ctc_beam")
        out[f"us_B{B}C{C}_plain_median"], out[f"us_B{B}C{C}_plain_min"], out[f"us_B{B}C{C}_plain_max"] = med, lo, hi
        for name, dg in devs.items():
            (m, lo, hi), ne = one(lib.sc_ctc_beam_grammar, grammar_jobs(0, t0, 1, dg.view),
                                  grammar_jobs(t0, t0 + rows, 0, dg.view), "sc_ctc_beam_grammar")
            key = f"us_B{B}C{C}_{name}"
            out[key + "_median"], out[key + "_min"], out[key + "_max"] = m, lo, hi
            out[f"ratio_B{B}C{C}_{name}"] = round(m / med, 2)
            out[f"entries_B{B}C{C}_{name}"] = round(ne, 1)
    out.update(us_empty_event_pair=round(float(lib.sc_prof_event_overhead_ms(s.cuda_stream)) * 1e3, 2),
               form="one wave per entry picks its state's candidates; two workgroup barriers per frame",
               source="hipEvent around one launch, rows rewritten and states put back before it")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--vocab", type=int, default=1024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_beam_grammar_bench needs a ROCm GPU")
    lib = _abi.load()
    blobs = grammars(args.vocab)
    for n in (58, 128):
        print(json.dumps(bench(n, args.rows, args.vocab, args.iters, lib, blobs)), flush=True)


if __name__ == "__main__":
    main()

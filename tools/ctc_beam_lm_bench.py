"""Time of one sc_ctc_beam_lm launch (the CTC prefix beam search with an n-gram model fused in) by hipEvents
around the launch, beside the plain sc_ctc_beam launch, the fused entry point without a model (lm == NULL) and an empty
event pair in the same session, at tools/ctc_beam_bench.py's shapes: 58 and 128 jobs of 16 rows at V = 1024, (B, C) =
(8, 8) and (16, 16), the jobs carrying a beam in from a first launch over 40 earlier rows; before every timed launch the
rows are written again by a device copy and the carried states are put back.  The model is synthetic: every unigram, and
the bigrams and trigrams of random sentences over the vocabulary, packed at the default load.

--lib PATH --plain-only times the plain launch of ANOTHER build of the library (the parent commit's, which has no fused
entry point) with the same code, for a before / after comparison of the kernel's LM = false instantiation.

    python tools/ctc_beam_lm_bench.py [--iters 30] [--order 3] [--sentences 4000] [--lib PATH --plain-only]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechcatcher_amd import _abi, ngram  # noqa: E402


def synthetic_model(V, order, sentences, length, seed):
    rng = np.random.default_rng(seed)
    model = {(w,): (-float(np.log(V)), -0.3) for w in range(V)}
    for _ in range(sentences):
        s = [int(t) for t in rng.integers(1, V, length)]
        for n in range(2, order + 1):
            for k in range(len(s) - n + 1):
                model[tuple(s[k:k + n])] = (-float(rng.uniform(0.5, 3.0)), -float(rng.uniform(0.1, 1.0)))
    return model


def _timed(launch, rewrite, iters, s):
    times = []
    for _ in range(iters):
        rewrite()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        launch()
        b.record(s)
        b.synchronize()
        times.append(a.elapsed_time(b))
    t = np.array(times) * 1e3
    return [round(float(np.median(t)), 2), round(float(t.min()), 2), round(float(t.max()), 2)]


def bench(n, rows, V, iters, lib, view, plain_only, tcap=256):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(n * 131 + rows)
    t0 = 40
    src = (torch.randn((n, t0 + rows, V), generator=g) * 4)
    src[:, :, 0] += 9.0                                  # the blank leads about half of the frames (ctc_beam_bench.py)
    src = src.to(dev)
    table = torch.zeros((n, tcap, V), dtype=torch.float32, device=dev)
    table[:, :t0 + rows].copy_(src)
    s = torch.cuda.current_stream(dev)
    SB, SN, SL = 528, 16, 192                            # sizeof sc_beam_t, sc_beam_node, sc_beam_lm_t
    out = {"jobs": n, "rows_per_job": rows, "V": V, "iters": iters}

    def check(rc, what):
        if rc != 0:
            raise SystemExit(f"{what} failed ({rc}): {lib.sc_last_error().decode()}")

    for B, Cn in ((8, 8), (16, 16)):
        cap = 1 + B * tcap
        kinds = ["plain"] if plain_only else ["plain", "no_model", "model"]
        for kind in kinds:
            state = torch.zeros((n, SB), dtype=torch.uint8, device=dev)
            after = torch.zeros((n, SB), dtype=torch.uint8, device=dev)
            nodes = torch.zeros((n, cap * SN), dtype=torch.uint8, device=dev)
            lms = torch.zeros((n, SL), dtype=torch.uint8, device=dev)
            lms_after = torch.zeros((n, SL), dtype=torch.uint8, device=dev)

            def jobs(a, b, restart):
                tab = ((_abi.BeamJob if kind == "plain" else _abi.BeamLmJob) * n)()
                for k in range(n):
                    j = tab[k] if kind == "plain" else tab[k].beam
                    j.table, j.state, j.nodes, j.state_after = (table[k].data_ptr(), state[k].data_ptr(),
                                                                nodes[k].data_ptr(), after[k].data_ptr())
                    j.stride, j.V, j.blank, j.t0, j.t1, j.restart, j.capacity, j.B, j.C = V, V, 0, a, b, restart, cap, B, Cn
                    if kind != "plain":
                        tab[k].lm = view if kind == "model" else None
                        tab[k].lm_state, tab[k].lm_state_after = lms[k].data_ptr(), lms_after[k].data_ptr()
                        tab[k].alpha, tab[k].beta = 0.5, 0.3
                return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)

            fn = lib.sc_ctc_beam if kind == "plain" else lib.sc_ctc_beam_lm
            first, span = jobs(0, t0, 1), jobs(t0, t0 + rows, 0)
            check(fn(first.data_ptr(), n, s.cuda_stream), kind)
            torch.cuda.synchronize(dev)
            carried, carried_lm = state.clone(), lms.clone()

            def launch():
                check(fn(span.data_ptr(), n, s.cuda_stream), kind)

            def rewrite():
                table[:, t0:t0 + rows].copy_(src[:, t0:])
                state.copy_(carried)
                lms.copy_(carried_lm)

            for _ in range(3):
                rewrite()
                launch()
            torch.cuda.synchronize(dev)
            st = after.cpu().numpy().view(np.int32).reshape(n, SB // 4)
            assert (st[:, 0] == t0 + rows).all() and (st[:, 1] == 0).all() and (st[:, 3] == B).all(), st[:, :4]
            out[f"us_B{B}C{Cn}_{kind}_median_min_max"] = _timed(launch, rewrite, iters, s)
            out[f"nodes_B{B}C{Cn}_{kind}"] = int(st[:, 2].sum())
    out["us_empty_event_pair"] = round(float(lib.sc_prof_event_overhead_ms(s.cuda_stream)) * 1e3, 2)
    out["source"] = "hipEvent around one launch, rows rewritten and states put back before it"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--vocab", type=int, default=1024)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--sentences", type=int, default=4000)
    ap.add_argument("--lib", default="", help="another build of libscasr.so (default: this tree's)")
    ap.add_argument("--plain-only", action="store_true", help="the plain launch alone (a library without sc_ctc_beam_lm)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_beam_lm_bench needs a ROCm GPU")
    if args.lib:
        lib = C.CDLL(os.path.abspath(args.lib))          # (torch is imported: the library binds to its HIP runtime)
        lib.sc_ctc_beam.restype, lib.sc_ctc_beam.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p]
        lib.sc_last_error.restype = C.c_char_p
        lib.sc_prof_event_overhead_ms.restype, lib.sc_prof_event_overhead_ms.argtypes = C.c_double, [C.c_void_p]
        if not args.plain_only:
            lib.sc_ctc_beam_lm.restype, lib.sc_ctc_beam_lm.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p]
    else:
        lib = _abi.load()
    view, info = None, {"library": args.lib or "in-tree", "plain_only": args.plain_only}
    if not args.plain_only:
        from speechcatcher_amd.hip_backend import DeviceLm
        blob = ngram.pack(synthetic_model(args.vocab, args.order, args.sentences, 8, 1), args.vocab, args.order)
        lm = DeviceLm(_abi.load(), blob)
        view = lm.view
        info.update(model_bytes=len(blob), order=lm.info.order, states=lm.info.n_states, slots=lm.info.n_slots,
                    arcs=ngram.Blob(blob).n_arcs)
    print(json.dumps(info), flush=True)
    for n in (58, 128):
        print(json.dumps(bench(n, args.rows, args.vocab, args.iters, lib, view, args.plain_only)), flush=True)


if __name__ == "__main__":
    main()

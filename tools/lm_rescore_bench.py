"""Time of one sc_lm_rescore launch (n-gram rescoring of n-best lists) by hipEvents around the launch:
the speculate-and-verify form against the SAME kernel with SC_RESCORE_FORCE_SERIAL (every row walked label by label by
one lane), beside one sc_hyp_commit launch over lists of the same shape and an empty event pair in the same session.
Shapes: 128 jobs x 10 rows x 400 labels and 128 x 10 x 34, V = 1024; the model is the synthetic order-3 model of
tools/ctc_beam_lm_bench.py; the rows follow the model's trigrams where it has any, with 15 % of the tokens replaced at
random, so lookups hit at the full context and back off.  Median, min and max of --iters launches in microseconds.

Before anything is timed the two forms are compared: every float64 and int32 equal, no row of the speculative run carries
SC_RESCORE_SERIAL, every row of the forced run does.

    python tools/lm_rescore_bench.py [--iters 30] [--order 3] [--sentences 4000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechcatcher_amd import _abi, ngram  # noqa: E402
from tools.ctc_beam_lm_bench import synthetic_model  # noqa: E402


def model_rows(model, V, n_rows, length, swap, seed):
    rng = np.random.default_rng(seed)
    follow = {}
    for g in model:
        if len(g) == 3:
            follow.setdefault(g[:2], []).append(g[2])
    starts = [g for g in model if len(g) == 2]
    rows = np.zeros((n_rows, length), np.int32)
    for r in range(n_rows):
        y = list(starts[int(rng.integers(len(starts)))])
        while len(y) < length:
            nxt = follow.get((y[-2], y[-1]))
            y.append(int(nxt[int(rng.integers(len(nxt)))]) if nxt else int(rng.integers(1, V)))
        rows[r] = y[:length]
    hit = rng.random(rows.shape) < swap
    rows[hit] = rng.integers(1, V, int(hit.sum()))
    return rows


def _timed(launch, iters, s):
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        launch()
        b.record(s)
        b.synchronize()
        times.append(a.elapsed_time(b))
    t = np.array(times) * 1e3
    return [round(float(np.median(t)), 2), round(float(t.min()), 2), round(float(t.max()), 2)]


def bench(lib, lm, model, n, n_hyp, labels, iters):
    dev = torch.device("cuda:0")
    V = lm.info.V
    s = torch.cuda.current_stream(dev)
    L = labels + 2                                        # <sos> labels <eos>
    body = model_rows(model, V, n * n_hyp, labels, 0.15, n + labels)
    rows = np.concatenate([np.full((n * n_hyp, 1), V - 1, np.int32), body, np.full((n * n_hyp, 1), V - 1, np.int32)], 1)
    yseq = torch.from_numpy(rows).to(dev).reshape(n, n_hyp, L)
    xpos = torch.zeros_like(yseq)
    score = torch.from_numpy(np.random.default_rng(1).uniform(-80.0, -20.0, (n, n_hyp, 3))).to(dev)
    H = _abi.RESCORE_MAX_HYPS
    out = {"jobs": n, "rows_per_job": n_hyp, "labels_per_row": labels, "V": V, "iters": iters}

    def check(rc, what):
        if rc != 0:
            raise SystemExit(f"{what} failed ({rc}): {lib.sc_last_error().decode()}")

    runs = {}
    for kind, flags in (("speculative", 0), ("forced_serial", _abi.RESCORE_FORCE_SERIAL)):
        f64 = torch.zeros((n, 3, H), dtype=torch.float64, device=dev)
        i32 = torch.zeros((n, 3, H), dtype=torch.int32, device=dev)
        tab = (_abi.RescoreJob * n)()
        for k in range(n):
            j = tab[k]
            j.model, j.yseq, j.score = lm.view, yseq[k].data_ptr(), score[k].data_ptr()
            j.fused, j.lm, j.eos_lm = (f64[k, c].data_ptr() for c in range(3))
            j.end_state, j.order, j.status = (i32[k, c].data_ptr() for c in range(3))
            j.row_stride, j.score_stride, j.alpha, j.beta = L, 3, 0.5, 0.3
            j.n_hyp, j.L, j.skip, j.strip, j.state0, j.lm_eos, j.V, j.flags = n_hyp, L, 1, V - 1, -1, V - 1, V, flags
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)

        def launch(tab_dev=tab_dev, kind=kind):
            check(lib.sc_lm_rescore(tab_dev.data_ptr(), n, s.cuda_stream), kind)

        for _ in range(3):
            launch()
        torch.cuda.synchronize(dev)
        runs[kind] = (f64.cpu().numpy()[:, :, :n_hyp].copy(), i32.cpu().numpy()[:, :, :n_hyp].copy())
        out[f"us_{kind}_median_min_max"] = _timed(launch, iters, s)
    (fa, ia), (fb, ib) = runs["speculative"], runs["forced_serial"]
    assert fa.tobytes() == fb.tobytes() and (ia[:, :2] == ib[:, :2]).all(), "the two forms differ"
    assert (ia[:, 2] == 0).all() and (ib[:, 2] == _abi.RESCORE_SERIAL).all(), (np.unique(ia[:, 2]), np.unique(ib[:, 2]))
    out["mean_lm_per_label"] = round(float(fa[:, 1].mean() / labels), 3)

    # one sc_hyp_commit launch over lists of the same shape
    head = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    agree = torch.zeros((n, _abi.COMMIT_MAX_HYPS), dtype=torch.int32, device=dev)
    tot = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    ids, pos = torch.zeros((n, L), dtype=torch.int32, device=dev), torch.zeros((n, L), dtype=torch.int32, device=dev)
    stab = torch.zeros((n, L), dtype=torch.float64, device=dev)
    ctab = (_abi.CommitJob * n)()
    for k in range(n):
        j = ctab[k]
        j.yseq, j.xpos, j.row_stride = yseq[k].data_ptr(), xpos[k].data_ptr(), L
        j.score, j.score_dec, j.score_ctc = (score[k].data_ptr() + 8 * c for c in range(3))
        j.score_stride = 3
        j.header, j.agree, j.totals = head[k].data_ptr(), agree[k].data_ptr(), tot[k].data_ptr()
        j.ids, j.pos, j.stability = ids[k].data_ptr(), pos[k].data_ptr(), stab[k].data_ptr()
        j.n_hyp, j.L, j.frm, j.flags = n_hyp, L, 0, 0
    ctab_dev = torch.frombuffer(bytearray(bytes(ctab)), dtype=torch.uint8).to(dev)

    def commit():
        check(lib.sc_hyp_commit(ctab_dev.data_ptr(), n, s.cuda_stream), "sc_hyp_commit")

    for _ in range(3):
        commit()
    torch.cuda.synchronize(dev)
    out["us_hyp_commit_median_min_max"] = _timed(commit, iters, s)
    out["us_empty_event_pair"] = round(float(lib.sc_prof_event_overhead_ms(s.cuda_stream)) * 1e3, 2)
    out["source"] = "hipEvent around one launch"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--vocab", type=int, default=1024)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--sentences", type=int, default=4000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lm_rescore_bench needs a ROCm GPU")
    from speechcatcher_amd.hip_backend import DeviceLm
    lib = _abi.load()
    model = synthetic_model(args.vocab, args.order, args.sentences, 8, 1)
    blob = ngram.pack(model, args.vocab, args.order)
    lm = DeviceLm(lib, blob)
    print(json.dumps({"model_bytes": len(blob), "order": lm.info.order, "states": lm.info.n_states, "slots": lm.info.n_slots,
                      "arcs": ngram.Blob(blob).n_arcs}), flush=True)
    for labels in (400, 34):
        print(json.dumps(bench(lib, lm, model, 128, 10, labels, args.iters)), flush=True)


if __name__ == "__main__":
    main()

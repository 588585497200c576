"""Time of one sc_mbr call (consensus of n-best lists) by hipEvents around the call, with a split by
launches (``split`` below), beside one sc_lm_rescore launch over the same lists, an empty event pair in the same
session, and the numpy contract's wall time for ONE such list on the host.  Shapes: 32 lists x 10 rows x 34 labels and 128 x 10 x 400, V = 1024; the rows are mutated copies of one
base row per list (tests/mbr_ref.py: family), the totals uniform in [-6, 0].  Median, min and max of --iters calls in
microseconds.

split: "pairs_only" = the call on lists whose named pivot is out (launch 1 does all its work, launch 2 finds no pivot,
launch 3 returns at once); "full" - "pairs_only" is what the risk launch and the backtraces add.

Before anything is timed the outputs of the first list are compared with the contract (integers equal).

    python tools/mbr_bench.py [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mbr_ref as M  # noqa: E402
from speechcatcher_amd import _abi, ngram  # noqa: E402


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


def bench(lib, lm, n, n_hyp, labels, iters):
    dev = torch.device("cuda:0")
    V = lm.info.V
    s = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(n + labels)
    fam = [M.family(rng, n_hyp, labels, V - 1) for _ in range(n)]
    L = max(len(y) for f in fam for y in f)
    rows = np.zeros((n, n_hyp, L), np.int32)
    lens = np.zeros((n, n_hyp), np.int32)
    for k, f in enumerate(fam):
        for h, y in enumerate(f):
            rows[k, h, :len(y)], lens[k, h] = y, len(y)
    score = rng.uniform(-6.0, 0.0, (n, n_hyp))
    yseq, lens_d, score_d = (torch.from_numpy(a).to(dev) for a in (rows, lens, score))
    H = _abi.MBR_MAX_HYPS
    out = {"lists": n, "rows_per_list": n_hyp, "labels_per_row": labels, "L": L, "V": V, "iters": iters}

    def check(rc, what):
        if rc != 0:
            raise SystemExit(f"{what} failed ({rc}): {lib.sc_last_error().decode()}")

    f64 = torch.zeros((n, 2, H), dtype=torch.float64, device=dev)
    i32 = torch.zeros((n, 2, H), dtype=torch.int32, device=dev)
    dist = torch.zeros((n, H * H), dtype=torch.int32, device=dev)
    head = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    pos = torch.zeros((n, 3, L + 1), dtype=torch.float64, device=dev)
    atok = torch.zeros((n, L + 1), dtype=torch.int32, device=dev)
    bad = score_d.clone()
    bad[:, 0] = float("nan")                                     # row 0 is out: a named pivot 0 leaves the list without one
    ws_bytes = int(lib.sc_mbr_ws_bytes(n, L))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    out["workspace_bytes"] = ws_bytes

    def table(scores, pivot):
        tab = (_abi.MbrJob * n)()
        for k in range(n):
            j = tab[k]
            j.yseq, j.score, j.lens = yseq[k].data_ptr(), scores[k].data_ptr(), lens_d[k].data_ptr()
            j.weight_out, j.risk = f64[k, 0].data_ptr(), f64[k, 1].data_ptr()
            j.order, j.status, j.dist, j.header = i32[k, 0].data_ptr(), i32[k, 1].data_ptr(), dist[k].data_ptr(), head[k].data_ptr()
            j.conf, j.alt_mass, j.gap_mass = (pos[k, c].data_ptr() for c in range(3))
            j.alt_tok = atok[k].data_ptr()
            j.row_stride, j.score_stride, j.scale = L, 1, 1.0
            j.n_hyp, j.L, j.skip, j.strip, j.V, j.pivot = n_hyp, L, 0, -1, V, pivot
        return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)

    full, pairs = table(score_d, -1), table(bad, 0)

    def run(tab):
        check(lib.sc_mbr(tab.data_ptr(), n, ws.data_ptr(), ws_bytes, s.cuda_stream), "sc_mbr")

    for _ in range(3):
        run(full)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    want = M.mbr(rows[0], score=score[0], lens=lens[0], L=L, V=V)
    out["ms_numpy_contract_one_list"] = round((time.perf_counter() - t0) * 1e3, 1)
    assert i32[0, 0, :n_hyp].cpu().tolist() == want["order"].tolist() and head[0].cpu().tolist() == want["header"].tolist()
    assert dist[0].cpu().reshape(H, H)[:n_hyp, :n_hyp].tolist() == want["dist"][:n_hyp, :n_hyp].tolist()
    mp = int(want["header"][1])
    assert atok[0, :mp].cpu().tolist() == want["alt_tok"].tolist()
    out["us_sc_mbr_median_min_max"] = _timed(lambda: run(full), iters, s)
    for _ in range(3):
        run(pairs)
    out["us_sc_mbr_pairs_only_median_min_max"] = _timed(lambda: run(pairs), iters, s)

    # one sc_lm_rescore launch over the same lists
    r64 = torch.zeros((n, 3, H), dtype=torch.float64, device=dev)
    r32 = torch.zeros((n, 3, H), dtype=torch.int32, device=dev)
    rtab = (_abi.RescoreJob * n)()
    for k in range(n):
        j = rtab[k]
        j.model, j.yseq, j.score, j.lens = lm.view, yseq[k].data_ptr(), score_d[k].data_ptr(), lens_d[k].data_ptr()
        j.fused, j.lm, j.eos_lm = (r64[k, c].data_ptr() for c in range(3))
        j.end_state, j.order, j.status = (r32[k, c].data_ptr() for c in range(3))
        j.row_stride, j.score_stride, j.alpha, j.beta = L, 1, 0.5, 0.3
        j.n_hyp, j.L, j.skip, j.strip, j.state0, j.lm_eos, j.V, j.flags = n_hyp, L, 0, -1, -1, V - 1, V, 0
    rtab_dev = torch.frombuffer(bytearray(bytes(rtab)), dtype=torch.uint8).to(dev)

    def rescore():
        check(lib.sc_lm_rescore(rtab_dev.data_ptr(), n, s.cuda_stream), "sc_lm_rescore")

    for _ in range(3):
        rescore()
    torch.cuda.synchronize(dev)
    out["us_lm_rescore_median_min_max"] = _timed(rescore, iters, s)
    out["us_empty_event_pair"] = round(float(lib.sc_prof_event_overhead_ms(s.cuda_stream)) * 1e3, 2)
    out["source"] = "hipEvent around one call"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--vocab", type=int, default=1024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mbr_bench needs a ROCm GPU")
    from speechcatcher_amd.hip_backend import DeviceLm
    lib = _abi.load()
    V = args.vocab
    rng = np.random.default_rng(0)
    model = {(t,): (float(-rng.uniform(1.0, 8.0)), float(-rng.uniform(0.0, 1.0))) for t in range(V)}
    for _ in range(20000):
        a, b = (int(v) for v in rng.integers(0, V, 2))
        model[(a, b)] = (float(-rng.uniform(0.1, 5.0)), 0.0)
    lm = DeviceLm(lib, ngram.pack(model, V, 2))
    for n, labels in ((32, 34), (128, 400)):
        print(json.dumps(bench(lib, lm, n, 10, labels, args.iters)), flush=True)


if __name__ == "__main__":
    main()

"""Time of one sc_dec_rescore call (attention rescoring of n-best lists) at XL dims by hipEvents around
the call: 32 lists x 8 rows x 34 labels against T = 70 encoder rows each, and 128 lists x 8 rows x 400 labels against
T = 790; beside each, sc_lm_rescore over the same lists (a synthetic order-3 model) and an empty event pair in the same
session.  Median, min and max of --iters calls in microseconds.  The weights are the synthetic XL model's; the workspace is
what the call needs at once unless --ws-mib limits it (the call then runs in slabs of whole lists).

    python tools/dec_rescore_bench.py [--iters 20] [--ws-mib 0] [--shapes small,large]

--once: one call per shape and nothing else, for a kernel trace of the call (e.g. under rocprofv3 --kernel-trace --stats,
whose per-kernel totals give the share of seq_attention_kernel).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechcatcher_amd import _abi, ngram, synth  # noqa: E402
from speechcatcher_amd.config import XL  # noqa: E402
from tools.ctc_beam_lm_bench import synthetic_model  # noqa: E402
from tools.lm_rescore_bench import _timed  # noqa: E402

SHAPES = {"small": (32, 8, 34, 70), "large": (128, 8, 400, 790)}


def bench(be, model, lm, name, iters, ws_mib, once):
    n, n_hyp, labels, T = SHAPES[name]
    dev, lib = be.device, be.lib
    V, d = XL.vocab_size, XL.d_model
    rng = np.random.default_rng(n + labels)
    s = torch.cuda.current_stream(dev)
    yseq = torch.from_numpy(rng.integers(1, V - 1, (n, n_hyp, labels)).astype(np.int32)).to(dev)
    score = torch.from_numpy(rng.uniform(-80.0, -20.0, (n, n_hyp))).to(dev)
    E = torch.from_numpy(rng.standard_normal((n, T, d)).astype(np.float32)).to(dev)
    f64 = torch.zeros((n, 2, 16), dtype=torch.float64, device=dev)
    i32 = torch.zeros((n, 2, 16), dtype=torch.int32, device=dev)
    tab = (_abi.DecRescoreJob * n)()
    for k in range(n):
        j = tab[k]
        j.E, j.e_stride, j.T = E[k].data_ptr(), d, T
        j.yseq, j.row_stride, j.score, j.score_stride = yseq[k].data_ptr(), labels, score[k].data_ptr(), 1
        j.wkv, j.bkv = model.wkv.data_ptr(), model.bkv.data_ptr()
        j.att, j.fused = (f64[k, c].data_ptr() for c in range(2))
        j.order, j.status = (i32[k, c].data_ptr() for c in range(2))
        j.w_att, j.w_ctc, j.beta = 1.0, 0.5, 0.0
        j.n_hyp, j.L, j.pe_rows = n_hyp, labels, model.pe_rows
    rows = n * n_hyp * (labels + 1)
    need = int(lib.sc_dec_rescore_ws_bytes(C.addressof(model.struct), rows, n * T, n * n_hyp, n))
    ws = torch.empty(min(need, ws_mib << 20) if ws_mib else need, dtype=torch.uint8, device=dev)

    def call():
        rc = lib.sc_dec_rescore(C.cast(tab, C.c_void_p), n, C.addressof(model.struct), ws.data_ptr(), ws.numel(), s.cuda_stream)
        if rc != 0:
            raise SystemExit(f"sc_dec_rescore failed ({rc}): {lib.sc_last_error().decode()}")

    call()
    torch.cuda.synchronize(dev)
    st = i32.cpu().numpy()[:, 1, :n_hyp]
    assert not st.any(), np.unique(st)
    out = {"shape": name, "lists": n, "rows_per_list": n_hyp, "labels_per_row": labels, "T": T, "token_rows": rows,
           "workspace_mib": round(ws.numel() / 2 ** 20, 1), "needed_mib": round(need / 2 ** 20, 1),
           "mean_att_per_token": round(float(f64.cpu().numpy()[:, 0, :n_hyp].mean() / (labels + 1)), 3)}
    if once:
        return out
    out["iters"] = iters
    out["us_dec_rescore_median_min_max"] = _timed(call, iters, s)

    # sc_lm_rescore over the same lists
    g64 = torch.zeros((n, 3, 16), dtype=torch.float64, device=dev)
    j32 = torch.zeros((n, 3, 16), dtype=torch.int32, device=dev)
    ltab = (_abi.RescoreJob * n)()
    for k in range(n):
        j = ltab[k]
        j.model, j.yseq, j.score = lm.view, yseq[k].data_ptr(), score[k].data_ptr()
        j.fused, j.lm, j.eos_lm = (g64[k, c].data_ptr() for c in range(3))
        j.end_state, j.order, j.status = (j32[k, c].data_ptr() for c in range(3))
        j.row_stride, j.score_stride, j.alpha, j.beta = labels, 1, 0.5, 0.0
        j.n_hyp, j.L, j.skip, j.strip, j.state0, j.lm_eos, j.V, j.flags = n_hyp, labels, 0, -1, -1, V - 1, V, 0
    ltab_dev = torch.frombuffer(bytearray(bytes(ltab)), dtype=torch.uint8).to(dev)

    def lm_call():
        if lib.sc_lm_rescore(ltab_dev.data_ptr(), n, s.cuda_stream) != 0:
            raise SystemExit(f"sc_lm_rescore failed: {lib.sc_last_error().decode()}")

    for _ in range(3):
        lm_call()
    torch.cuda.synchronize(dev)
    out["us_lm_rescore_median_min_max"] = _timed(lm_call, iters, s)
    out["us_empty_event_pair"] = round(float(lib.sc_prof_event_overhead_ms(s.cuda_stream)) * 1e3, 2)
    out["source"] = "hipEvent around one call"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ws-mib", type=int, default=0, help="limit of the workspace in MiB (0: what the call needs at once)")
    ap.add_argument("--shapes", default="small,large")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dec_rescore_bench needs a ROCm GPU")
    from speechcatcher_amd.hip_backend import DeviceLm, HipBackend
    from speechcatcher_amd.weights import PackedWeights
    be = HipBackend("cuda:0", use_graphs=False)
    model = be.decoder_model(PackedWeights(synth.make_state_dict(XL, 1234), XL, "cuda:0"), LCAP=512)
    lm = DeviceLm(be.lib, ngram.pack(synthetic_model(XL.vocab_size, 3, 4000, 8, 1), XL.vocab_size, 3))
    for name in args.shapes.split(","):
        print(json.dumps(bench(be, model, lm, name, args.iters, args.ws_mib, args.once)), flush=True)


if __name__ == "__main__":
    main()

"""Time of the sc_ctc_alternates launch (one workgroup per token span: float64 sums of the span's rows, the per-row
logsumexp, K rounds of arg-max) by hipEvents around the launch, with the sc_ctc_align launch pair over the same jobs and the
two back to back - the device work of sc_align_hyps and of sc_alternates_hyps - in the same session.  The two shapes of
the alignment's measurements: 128 jobs at T = 790, L = 400 (a stream of the headline window, best hypothesis) and 128 jobs
at T = 4800, L = 1000 (a three-minute CLI segment), V = 1024.  The alternates read the spans the alignment left on the
device.  Then the stream-level calls themselves on a batch of the XL synthetic model at a final: host time around
sc_align_hyps and sc_alternates_hyps (upload, launches, one copy back, the wait) for the same hypotheses.  Prints one JSON
line per shape.  Kernel times: run it under `rocprofv3 --kernel-trace --stats` in a run of its own.

    python tools/alt_bench.py [--iters 20] [--jobs 128] [--k 3] [--no-streams]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechcatcher_amd import _abi  # noqa: E402


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
    return {"median": round(float(np.median(t)), 1), "min": round(float(t.min()), 1), "max": round(float(t.max()), 1)}


def bench(n, T, L, V, K, iters, lib):
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
    alt_ids = torch.empty((n, L, K), dtype=torch.int32, device=dev)
    alt_lp = torch.empty((n, L, K), dtype=torch.float64, device=dev)
    rank = torch.empty((n, L), dtype=torch.int32, device=dev)
    sst = torch.empty((n, L), dtype=torch.int32, device=dev)
    tab, atab = (_abi.AlignJob * n)(), (_abi.AltJob * n)()
    for k in range(n):
        j = tab[k]
        j.emis, j.labels, j.ws = emis[k].data_ptr(), labels[k].data_ptr(), ws.data_ptr() + k * ws_b
        j.start, j.end, j.logp_mean = out_i[k, 0].data_ptr(), out_i[k, 1].data_ptr(), out_f[k].data_ptr()
        j.path_score, j.status = ps[k].data_ptr(), st[k].data_ptr()
        j.stride, j.T, j.L, j.V, j.blank = V, T, L, V, 0
        a = atab[k]
        a.emis, a.labels, a.start, a.end = j.emis, j.labels, j.start, j.end
        a.alt_ids, a.alt_logp = alt_ids[k].data_ptr(), alt_lp[k].data_ptr()
        a.own_rank, a.status = rank[k].data_ptr(), sst[k].data_ptr()
        a.stride, a.T, a.V, a.blank, a.L = V, T, V, 0, L
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
    atab_dev = torch.frombuffer(bytearray(bytes(atab)), dtype=torch.uint8).to(dev)
    s = torch.cuda.current_stream(dev)

    def align():
        _abi.check(lib.sc_ctc_align(tab_dev.data_ptr(), n, T, L, s.cuda_stream), "sc_ctc_align")

    def alternates():
        _abi.check(lib.sc_ctc_alternates(atab_dev.data_ptr(), n, L, K, s.cuda_stream), "sc_ctc_alternates")

    def both():
        align()
        alternates()

    for _ in range(3):
        both()
    torch.cuda.synchronize(dev)
    assert int((st != 0).sum()) == 0 and int((sst != 0).sum()) == 0
    span = (out_i[:, 1] - out_i[:, 0]).cpu().numpy()
    assert (rank.cpu().numpy() >= 0).all()
    return {"jobs": n, "T": T, "L": L, "V": V, "K": K, "iters": iters,
            "us_alternates": _timed(alternates, iters, s), "us_align": _timed(align, iters, s),
            "us_align_then_alternates": _timed(both, iters, s),
            "rows_covered_per_job": int(span.sum() // n), "longest_span": int(span.max()),
            "own_rank_0_share": round(float((rank.cpu().numpy() == 0).mean()), 3),
            "us_empty_event_pair": round(float(lib.sc_prof_event_overhead_ms(s.cuda_stream)) * 1e3, 2),
            "source": "hipEvent around the launches (sc_ctc_alternates: one; sc_ctc_align: two)"}


def bench_streams(S, chunks, K, iters):
    """sc_align_hyps against sc_alternates_hyps on the hypotheses of S streams of the XL synthetic model at their final"""
    from speechcatcher_amd import synth
    from speechcatcher_amd.config import XL, SearchConfig
    from speechcatcher_amd.native import NativeStreamBatch
    from speechcatcher_amd.weights import PackedWeights
    sd = synth.make_state_dict(XL, 1234)
    mean, std = synth.stats_to_mean_std(synth.make_stats(XL, kind="meanstd"))
    w = PackedWeights(sd, XL, "cuda:0", mean, std)
    sb = NativeStreamBatch(w, S, SearchConfig(beam_size=5), max_frames=256, max_tokens=256, pcm_capacity=1 << 18)
    chunk = 10240
    audio = [synth.synth_audio(500 + s, chunk * chunks) for s in range(S)]
    for k in range(chunks):
        sb.push([(s, audio[s][k * chunk:(k + 1) * chunk], k == chunks - 1) for s in range(S)])
    ids = list(range(S))

    def host(fn):
        t = []
        for _ in range(iters):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        t = np.array(t)
        return {"median": round(float(np.median(t)), 1), "min": round(float(t.min()), 1), "max": round(float(t.max()), 1)}

    out = {"streams": S, "frames": int(sb.read_ctc(0).shape[0]), "K": K, "iters": iters}
    for nb in (1, 5):
        for _ in range(3):
            al, alt = sb.align(ids, nb), sb.alternates(ids, nb, K)
        assert all(al[k].tobytes() == alt[k].tobytes() for k in ("start", "end", "logp_mean", "path_score", "status"))
        h = sb.hypotheses_arrays(ids)
        out[f"nbest_{nb}"] = {"hypotheses": int(al["n_hyps"].sum()),
                              "tokens": int(sum(int(h["lens"][i, j]) - 2 for i in range(S) for j in range(int(al["n_hyps"][i])))),
                              "us_host_align_hyps": host(lambda: sb.align(ids, nb)),
                              "us_host_alternates_hyps": host(lambda: sb.alternates(ids, nb, K))}
    out["source"] = "host clock around NativeStreamBatch.align / .alternates (upload, launches, one copy back, the wait)"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--jobs", type=int, default=128)
    ap.add_argument("--vocab", type=int, default=1024)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--no-streams", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("alt_bench needs a ROCm GPU")
    lib = _abi.load()
    for T, L in ((790, 400), (4800, 1000)):
        print(json.dumps(bench(args.jobs, T, L, args.vocab, args.k, args.iters, lib)), flush=True)
    if not args.no_streams:
        print(json.dumps(bench_streams(32, 6, args.k, args.iters)), flush=True)


if __name__ == "__main__":
    main()

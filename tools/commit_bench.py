"""Time of the sc_hyp_commit launch (one workgroup per beam: first mismatch of every hypothesis against the best one, the
beam's weights in float64, the tail's ids, positions and stability) by hipEvents around the launch: 128 beams of 10
hypotheses of 400 tokens in rows 500 apart, with from = 0 (the whole best hypothesis travels) and with from = commit and
a tail of 8 (what a client that holds the committed prefix asks for), beside an empty event pair.  Then the stream-level
calls themselves on a batch of the XL synthetic model (beam 10) after a few chunks: host time around sc_get_hyps_delta
(from = 0, and from = what a StablePrefix holds) and around sc_get_hyps_batch at nbest = 1 and nbest = 10 for the same
streams in the same session, with the bytes each call copies back.  Prints one JSON line per part.

    python tools/commit_bench.py [--iters 50] [--jobs 128] [--no-streams]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechcatcher_amd import _abi, commit  # noqa: E402


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


def bench_kernel(n, L, W, stride, tail, iters, lib):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(L)
    y = np.tile(rng.integers(2, 1000, size=(n, 1, stride), dtype=np.int32), (1, W, 1))
    commit_at = L - tail
    for h in range(1, W):                                   # the rivals leave the best hypothesis inside the tail
        y[:, h, commit_at + (h - 1) % tail:] += 1 + h
    yd = torch.from_numpy(y).to(dev)
    xd = torch.from_numpy(np.tile(np.arange(stride, dtype=np.int32), (n, W, 1))).to(dev)
    sc = torch.from_numpy(-np.sort(rng.random((n, W, 3)) * 5.0, 1)).to(dev)
    head = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    agree = torch.zeros((n, 16), dtype=torch.int32, device=dev)
    ids, pos = (torch.zeros((n, L), dtype=torch.int32, device=dev) for _ in range(2))
    stab = torch.zeros((n, L), dtype=torch.float64, device=dev)
    tot = torch.zeros((n, 3), dtype=torch.float64, device=dev)

    def table(frm):
        tab = (_abi.CommitJob * n)()
        for k in range(n):
            j = tab[k]
            j.yseq, j.xpos, j.row_stride = yd[k].data_ptr(), xd[k].data_ptr(), stride
            j.score, j.score_dec, j.score_ctc = (sc[k].data_ptr() + 8 * c for c in range(3))
            j.score_stride = 3
            j.header, j.agree, j.totals = head[k].data_ptr(), agree[k].data_ptr(), tot[k].data_ptr()
            j.ids, j.pos, j.stability = ids[k].data_ptr(), pos[k].data_ptr(), stab[k].data_ptr()
            j.n_hyp, j.L, j.frm, j.flags = W, L, frm, 0
        return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)

    s = torch.cuda.current_stream(dev)
    out = {"jobs": n, "L": L, "n_hyp": W, "row_stride": stride, "iters": iters}
    for name, frm in (("from_0", 0), (f"from_commit_tail_{tail}", commit_at)):
        tab_dev = table(frm)

        def launch():
            _abi.check(lib.sc_hyp_commit(tab_dev.data_ptr(), n, s.cuda_stream), "sc_hyp_commit")

        for _ in range(3):
            launch()
        torch.cuda.synchronize(dev)
        assert (head[:, 0] == L).all() and (head[:, 1] == commit_at).all()
        out[f"us_{name}"] = _timed(launch, iters, s)
        out[f"bytes_back_{name}"] = n * (26 + 4 * (L - frm)) * 4
    out["bytes_back_get_hyps_batch_nbest_1"] = n * (2 * L + 6) * 4
    out[f"bytes_back_get_hyps_batch_nbest_{W}"] = n * W * (2 * L + 6) * 4
    out["us_empty_event_pair"] = round(float(lib.sc_prof_event_overhead_ms(s.cuda_stream)) * 1e3, 2)
    out["source"] = "hipEvent around the sc_hyp_commit launch"
    return out


def bench_streams(S, chunks, W, iters):
    """sc_get_hyps_delta against sc_get_hyps_batch on the live beams of S streams of the XL synthetic model"""
    from speechcatcher_amd import synth
    from speechcatcher_amd.config import XL, SearchConfig
    from speechcatcher_amd.native import NativeStreamBatch
    from speechcatcher_amd.weights import PackedWeights
    sd = synth.make_state_dict(XL, 1234)
    mean, std = synth.stats_to_mean_std(synth.make_stats(XL, kind="meanstd"))
    w = PackedWeights(sd, XL, "cuda:0", mean, std)
    sb = NativeStreamBatch(w, S, SearchConfig(beam_size=W), max_frames=256, max_tokens=256, pcm_capacity=1 << 18)
    chunk = 10240
    audio = [synth.synth_audio(500 + s, chunk * chunks) for s in range(S)]
    ids = list(range(S))
    held = [commit.StablePrefix() for _ in ids]
    for k in range(chunks):
        if k == chunks - 1:                                 # what the clients hold when the last reply arrives
            frm = [sp.next_from for sp in held]
        sb.push([(s, audio[s][k * chunk:(k + 1) * chunk], False) for s in ids])
        d = sb.hyps_delta(ids, [sp.next_from for sp in held])
        for s in ids:
            held[s].update(d[s])

    def host(fn):
        t = []
        for _ in range(iters):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        t = np.array(t)
        return {"median": round(float(np.median(t)), 1), "min": round(float(t.min()), 1), "max": round(float(t.max()), 1)}

    whole = sb.hyps_delta(ids, [0] * S)
    tail = sb.hyps_delta(ids, frm)
    Ls = [whole[s]["L"] for s in ids]
    out = {"streams": S, "beam": W, "chunks": chunks, "iters": iters, "L_mean": round(float(np.mean(Ls)), 1),
           "commit_mean": round(float(np.mean([whole[s]["commit"] for s in ids])), 1),
           "tail_mean": round(float(np.mean([len(tail[s]["tokens"]) for s in ids])), 1)}
    for _ in range(3):
        sb.hyps_delta(ids, frm), sb.hypotheses_arrays(ids, 1), sb.hypotheses_arrays(ids, W)
    out["us_host_hyps_delta_arrays_from_0"] = host(lambda: sb.hyps_delta_arrays(ids, [0] * S))
    out["us_host_hyps_delta_arrays_from_held"] = host(lambda: sb.hyps_delta_arrays(ids, frm))
    out["us_host_hyps_delta_dicts_from_held"] = host(lambda: sb.hyps_delta(ids, frm))
    out["us_host_hypotheses_batch_dicts_nbest_1"] = host(lambda: sb.hypotheses_batch(ids, 1))
    out["us_host_hypotheses_arrays_nbest_1"] = host(lambda: sb.hypotheses_arrays(ids, 1))
    out[f"us_host_hypotheses_arrays_nbest_{W}"] = host(lambda: sb.hypotheses_arrays(ids, W))
    out["bytes_back_hyps_delta_from_0"] = int(sum((26 + 4 * L) * 4 for L in Ls))
    out["bytes_back_hyps_delta_from_held"] = int(sum((26 + 4 * len(tail[s]["tokens"])) * 4 for s in ids))
    out["bytes_back_get_hyps_batch_nbest_1"] = int(sum((((2 * L + 1) & ~1) + 6) * 4 for L in Ls))
    out[f"bytes_back_get_hyps_batch_nbest_{W}"] = int(sum(whole[s]["n_hyp"] * (((2 * L + 1) & ~1) + 6) * 4
                                                          for s, L in zip(ids, Ls)))
    out["source"] = ("host clock around NativeStreamBatch.hyps_delta_arrays / .hypotheses_arrays (upload, one launch, one "
                     "copy back, the wait, the numpy arrays of the reply) and around the calls that turn them into dicts")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--jobs", type=int, default=128)
    ap.add_argument("--no-streams", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("commit_bench needs a ROCm GPU")
    lib = _abi.load()
    print(json.dumps(bench_kernel(args.jobs, 400, 10, 500, 8, args.iters, lib)), flush=True)
    if not args.no_streams:
        print(json.dumps(bench_streams(32, 6, 10, args.iters)), flush=True)


if __name__ == "__main__":
    main()

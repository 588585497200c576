"""bench.py's headline around the CTC prefix beam search (sc_streams_set_ctc_beam) and decoder-free streams
(sc_stream_set_decoder), measured in ONE session with alternating runs, every run a process of its own:

    off      `python bench.py --legs none` of this tree: the option off
    parent   the same of another checkout (--parent DIR: the parent commit, built), when one is given
    on       bench.py's headline with the option on at (B, C): every admission group of the measured window issues its
             one sc_ctc_beam launch behind the CTC projection
    on_lm    (--lm-order N > 0) the same with a synthetic n-gram model of order N fused into the beam
             (sc_streams_set_ctc_beam_lm; tools/ctc_beam_lm_bench.py's model): the group issues sc_ctc_beam_lm instead
    served   the served throughput of the headline's closed loop (bench.measure) with every stream SC_DECODER_NONE against
             every stream FULL, the option on in both - fresh batches of one process

Prints one JSON line: per kind the values of its runs (audio seconds per second), in the order they were taken.

    python tools/ctc_beam_headline.py --rounds 2 --steps 20 --warmup 5 [--parent build_ab/parent] [--beam 8 --candidates 8]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _with_beam(B, C, none=False, lm_order=0):
    import bench
    build = bench.build_native
    blob = None
    if lm_order:
        from speechcatcher_amd import ngram
        from tools.ctc_beam_lm_bench import synthetic_model

    def build_with_beam(*a, **kw):
        sb = build(*a, **kw)
        if none:
            for s in range(sb.S):
                sb.set_decoder(s, "ctc")
        sb.set_ctc_beam(B, C)
        if lm_order:
            nonlocal blob
            if blob is None:
                V = sb.cfg.vocab_size
                blob = ngram.pack(synthetic_model(V, lm_order, 4000, 8, 1), V, lm_order)
            sb.set_ctc_beam_lm(blob, 0.5, 0.3)
        return sb

    bench.build_native = build_with_beam
    return bench, build


def child_on(args, rest):
    bench, _ = _with_beam(args.beam, args.candidates, lm_order=args.lm_order if args.child == "on_lm" else 0)
    sys.argv = [sys.argv[0]] + rest + ["--steps", str(args.steps), "--warmup", str(args.warmup), "--streams", str(args.streams)]
    bench.main()


def child_served(args):
    """every stream decoder-free against every stream FULL: bench.py's continuous headline loop on fresh batches"""
    import torch
    bench, plain = _with_beam(args.beam, args.candidates)
    S, pre, warm, steps = args.streams, 21, args.warmup, args.steps
    total = pre + warm + steps + bench.SERVED_SPARE
    w = bench.make_weights("cuda:0")
    audio = bench.make_audio(S, total)
    out = {}
    for kind in ("full", "none", "full", "none"):
        bench.build_native = plain
        _with_beam(args.beam, args.candidates, none=kind == "none")
        sb, r = bench.measure(w, audio, S, 10, False, pre, warm, steps, max(1, S // 8), "continuous", total)
        steps_run = sum(int(st.n_steps_total) for st in sb.st)
        assert (steps_run == 0) == (kind == "none"), (kind, steps_run)
        frames = [b["n_frames"] for b in sb.ctc_beam(list(range(S)))]
        assert min(frames) > 0, frames
        out.setdefault(kind, []).append(round(float(r["value"]), 1))
        del sb
        torch.cuda.empty_cache()
    print(json.dumps({"served": out, "streams": S, "steps": steps, "unit": "audio_s/s"}), flush=True)


def _value(cmd, cwd, key="value"):
    res = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed:\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])[key]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["on", "on_lm", "served"], default=None)
    ap.add_argument("--lm-order", type=int, default=0, help="> 0: also the option on with a synthetic model of this order")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--parent", default="", help="a checkout of the parent commit with its library built")
    args, rest = ap.parse_known_args()
    if args.child in ("on", "on_lm"):
        return child_on(args, rest)
    if args.child == "served":
        return child_served(args)
    py = sys.executable
    bench_args = ["--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup), "--legs", "none"]
    me = [py, os.path.abspath(__file__), "--beam", str(args.beam), "--candidates", str(args.candidates),
          "--steps", str(args.steps), "--warmup", str(args.warmup), "--streams", str(args.streams)]
    out = {"off": [], "parent": [], "on": [], "on_lm": [], "served": None, "B": args.beam, "C": args.candidates, "unit": "audio_s/s"}
    for _ in range(args.rounds):
        if args.parent:
            out["parent"].append(_value([py, "bench.py"] + bench_args, os.path.abspath(args.parent)))
        out["off"].append(_value([py, "bench.py"] + bench_args, ROOT))
        out["on"].append(_value(me + ["--child", "on"] + bench_args, ROOT))
        if args.lm_order:
            out["on_lm"].append(_value(me + ["--child", "on_lm", "--lm-order", str(args.lm_order)] + bench_args, ROOT))
        print(json.dumps(out), file=sys.stderr, flush=True)
    out["served"] = _value(me + ["--child", "served"], ROOT, key="served")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

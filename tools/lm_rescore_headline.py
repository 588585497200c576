"""bench.py's headline before and after n-gram rescoring of finals was added, measured in ONE session with
alternating runs, every run a process of its own:

    parent   `python bench.py --legs none` of another checkout (--parent DIR: the parent commit, built with its own library)
    this     the same of this tree

The rescoring calls are opt-in and sit outside the timed path (no call: no allocation, no launch), so the two are expected
to overlap; this writes down that they do.  Prints one JSON line: per kind the values of its runs (audio seconds per
second), in the order they were taken.

    python tools/lm_rescore_headline.py --rounds 2 --steps 20 --warmup 5 --parent build_ab/parent
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _value(cmd, cwd):
    res = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed:\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])["value"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent", required=True, help="a checkout of the parent commit with its library built")
    args = ap.parse_args()
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup), "--legs", "none"]
    out = {"parent": [], "this": [], "unit": "audio_s/s", "steps": args.steps, "warmup": args.warmup}
    for _ in range(args.rounds):
        out["parent"].append(_value(cmd, os.path.abspath(args.parent)))
        out["this"].append(_value(cmd, ROOT))
        print(json.dumps(out), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

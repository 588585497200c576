"""bench.py's headline with the acoustic-activity option switched ON (sc_streams_set_activity): every admission group of
the measured window issues its one sc_ctc_activity launch behind the CTC projection.  Takes bench.py's arguments and
prints bench.py's JSON line; compare `value` with a plain `python bench.py` run of the same session (option off).

    python tools/activity_headline.py --gpus 1 --steps 20 --warmup 5 [--blank-threshold 0.8]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    thr = 0.8
    if "--blank-threshold" in sys.argv:
        i = sys.argv.index("--blank-threshold")
        thr = float(sys.argv[i + 1])
        del sys.argv[i:i + 2]
    build = bench.build_native

    def build_with_activity(*a, **kw):
        sb = build(*a, **kw)
        sb.set_activity(True, thr)
        return sb

    bench.build_native = build_with_activity
    bench.main()


if __name__ == "__main__":
    main()

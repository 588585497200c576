"""bench.py's headline with the draft-transcript option switched ON (sc_streams_set_draft): every admission group of the
measured window issues its one sc_ctc_draft launch behind the CTC projection.  Takes bench.py's arguments and prints
bench.py's JSON line; compare `value` with a plain `python bench.py` run of the same session (option off).

    python tools/draft_headline.py --gpus 1 --steps 20 --warmup 5
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    build = bench.build_native

    def build_with_draft(*a, **kw):
        sb = build(*a, **kw)
        sb.set_draft(True)
        return sb

    bench.build_native = build_with_draft
    bench.main()


if __name__ == "__main__":
    main()

"""bench.py's headline with the phrase-spotting option switched ON (sc_streams_set_phrases): every admission group of
the measured window issues its one sc_ctc_spot launch behind the CTC projection.  Takes bench.py's arguments and
prints bench.py's JSON line; compare `value` with a plain `python bench.py` run of the same session (option off).

    python tools/spot_headline.py --gpus 1 --steps 20 --warmup 5 [--phrases 16] [--len 8]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _take(flag, default):
    if flag not in sys.argv:
        return default
    i = sys.argv.index(flag)
    v = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
    return v


def main():
    P, L = _take("--phrases", 16), _take("--len", 8)
    build = bench.build_native

    def build_with_phrases(*a, **kw):
        sb = build(*a, **kw)
        rng = np.random.default_rng(7)
        labels = [v for v in range(sb.cfg.vocab_size) if v != sb.cfg.blank_id]
        sb.set_phrases([[int(t) for t in rng.choice(labels, size=L)] for _ in range(P)])
        return sb

    bench.build_native = build_with_phrases
    bench.main()


if __name__ == "__main__":
    main()

"""The read-back services of one handle share ONE scratch area and one round trip (csrc/stream_readback.hip; DESIGN.md
section 5, "Read-back calls"): every call lays its own tables out from offset 0 of the area and keeps nothing there, so
what a call returns must not depend on which service used the area before it, nor on the area having been reallocated in
between.

On the tiny synthetic model, 2 streams (stream 1 decoder-free), a CTC beam of 8, 6 chunks pushed: one handle runs
ctc_beam_hyps, rescore_lists (2 lists of 16 rows of 500 labels: 64 KB of ids, more than twice what ctc_beam_hyps needed,
so the area is freed and allocated again), align, alternates, attention_rescore_beam, hyps_delta and rescore_hyps, then
all of them again in reverse order.  Every result of the second pass equals the first pass bit for bit (float64 compared
as uint64), and every first-pass result equals the same call made on a fresh handle where it is the only read-back
call."""
import numpy as np
import pytest

import ngram_ref as NR
from draft_helpers import make_batch, packed_weights
from speechcatcher_amd import ngram, synth
from test_gpu_ctc_beam_streams import CHUNK, KW, _chunks

pytestmark = pytest.mark.gpu

S, N, W, B = 2, 6, 5, 8
ALPHA, BETA = 0.5, 0.3
W_ATT, W_CTC = 1.0, 0.5
ROWS, LABELS = 16, 500
BOTH = [0, 1]


def _bits(x):
    """a result as plain Python values that compare exactly: float64 as uint64, arrays with dtype and shape"""
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_bits(v) for v in x]
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        return (str(a.dtype), a.shape, (a.view(np.uint64) if a.dtype == np.float64 else a).tolist())
    if isinstance(x, (float, np.floating)):
        return ("f64", int(np.float64(x).view(np.uint64)))
    return x


def _handle(p):
    """stream 0 with the decoder, stream 1 decoder-free, every chunk pushed: both idle, the last chunk was the final"""
    sb = make_batch("mixed", "TINY", "native", S, beam=W, weights=p["w"], **dict(KW, **p["share"]))
    p["share"]["engine"] = sb.engine                                 # (the weights are uploaded once)
    sb.set_decoder(1, "ctc")
    sb.set_ctc_beam(B, B)
    for k in range(N):
        sb.push(_chunks(p, k))
    return sb


def _calls(p, sb, dev):
    return [
        ("ctc_beam_hyps", lambda: sb.ctc_beam_hyps(BOTH, B)),
        ("rescore_lists", lambda: sb.rescore_lists(p["lists"], p["scores"], dev, ALPHA, BETA, lm_eos=p["eos"])),
        ("align", lambda: sb.align(BOTH)),
        ("alternates", lambda: sb.alternates(BOTH, k=3)),
        ("attention_rescore_beam", lambda: sb.attention_rescore_beam(BOTH, B, W_ATT, W_CTC, BETA)),
        ("hyps_delta", lambda: sb.hyps_delta(BOTH, [0, 0], final=[0])),
        ("rescore_hyps", lambda: sb.rescore_hyps(BOTH, dev, ALPHA, BETA, lm_eos=p["eos"], final=[0])),
    ]


NAMES = ["ctc_beam_hyps", "rescore_lists", "align", "alternates", "attention_rescore_beam", "hyps_delta", "rescore_hyps"]


@pytest.fixture(scope="module")
def probe():
    p = {"w": packed_weights("mixed", "TINY", "cuda:0"), "S": S, "n": N, "share": {}}
    p["audio"] = [synth.synth_audio([7, 10][s], CHUNK * N - 1000 * s) for s in range(S)]
    sb = _handle(p)
    p["eos"], V = sb.cfg.eos_id, sb.cfg.vocab_size
    rng = np.random.default_rng(5)
    labels = [t for t in range(V) if t not in (sb.cfg.blank_id, sb.cfg.sos_id, sb.cfg.eos_id)]
    p["lists"] = [[rng.choice(labels, LABELS - r).tolist() for r in range(ROWS)] for _ in range(2)]
    p["scores"] = [(-rng.random(ROWS) * 50.0).tolist() for _ in range(2)]
    # the small model of test_gpu_lm_rescore_streams: order 3, estimated from sentences over the same vocabulary
    sents = [row[:12] + [p["eos"]] for li in p["lists"] for row in li]
    p["blob"] = ngram.pack(NR.estimate(sents, V, 3), V, 3)
    dev = sb.language_model(p["blob"])
    calls = _calls(p, sb, dev)
    assert [name for name, _ in calls] == NAMES
    p["first"] = {name: _bits(call()) for name, call in calls}
    p["second"] = {name: _bits(call()) for name, call in reversed(calls)}
    dev.close()
    return p


def test_the_calls_report_something(probe):
    """(the comparisons below are about real results: hypotheses on the full stream, entries on both beams)"""
    first = probe["first"]
    assert first["align"]["n_hyps"][2] == [first["rescore_hyps"][s]["order"][1][0] for s in BOTH]
    assert first["align"]["n_hyps"][2][0] >= 2                       # (the decoder-free stream holds its initial hypothesis)
    assert all(len(first["ctc_beam_hyps"][s]) >= 2 for s in BOTH)
    assert all(first["attention_rescore_beam"][s]["order"][1][0] >= 2 for s in BOTH)
    assert first["hyps_delta"][0]["L"] > 1
    assert [r["order"][1][0] for r in first["rescore_lists"]] == [ROWS, ROWS]


@pytest.mark.parametrize("name", NAMES)
def test_second_pass_in_reverse_order_equals_the_first_bit_for_bit(probe, name):
    assert probe["second"][name] == probe["first"][name]


@pytest.mark.parametrize("name", NAMES)
def test_first_pass_equals_the_call_alone_on_a_fresh_handle(probe, name):
    p = probe
    sb = _handle(p)
    dev = sb.language_model(p["blob"])
    alone = _bits(dict(_calls(p, sb, dev))[name]())
    dev.close()
    assert alone == p["first"][name]

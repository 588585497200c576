"""All five CTC-row options of the C++ engine on together - acoustic activity, phrase spotting, draft transcript, input
level and the CTC prefix beam search (sc_streams_set_ctc_beam, OPT_BEAM of csrc/streams.hip) - against handles with
exactly one option on, across a reset: the run of tests/test_gpu_side_states.py with the beam as a fifth option.  Its
probe and its test body are used as they are; this file adds how the fifth option is switched on, how its state is read
in a form that compares bit for bit, and its state before anything of an utterance has been scanned."""
import numpy as np
import pytest

import test_gpu_side_states as base

pytestmark = pytest.mark.gpu

BC = (4, 4)
NEG = -np.inf


def _switch_on(sb, opts, p, _base=base._switch_on):
    _base(sb, opts, p)
    if "beam" in opts:
        sb.set_ctc_beam(*BC)


def _read(sb, s, opt, _base=base._read):
    if opt != "beam":
        return _base(sb, s, opt)
    st = sb.ctc_beam([s])[0]
    hy = sb.ctc_beam_hyps([s], BC[0])[s]
    floats = [v for e in st["entries"] for v in e[4:]] + [v for h in hy for v in (h["pb"], h["pnb"])]
    return ((st["n_frames"], st["n_bad"], st["n_nodes"]), tuple(e[:4] for e in st["entries"]),
            tuple((tuple(h["ids"]), tuple(h["frames"])) for h in hy), np.asarray(floats, np.float64).tobytes())


INITIAL_BEAM = ((0, 0, 1), ((0, -1, 0, -1),), (((), ()),), np.asarray([0.0, NEG, 0.0, NEG], np.float64).tobytes())


@pytest.fixture(scope="module")
def five():
    """the base module with the fifth option patched in while this module's tests run"""
    mp = pytest.MonkeyPatch()
    mp.setattr(base, "OPTIONS", base.OPTIONS + ("beam",))
    mp.setattr(base, "_switch_on", _switch_on)
    mp.setattr(base, "_read", _read)
    mp.setattr(base, "INITIAL", dict(base.INITIAL, beam=INITIAL_BEAM))
    try:
        yield base.build_probe()
    finally:
        mp.undo()


def test_all_five_options_on_at_queue_depth_2_equal_the_single_option_handles_across_a_reset(five):
    p = five
    assert "beam" in base.OPTIONS and "beam" in p["ref"] and "beam" in p["ref2"]
    last = p["ref"]["beam"][base.N - 1]
    assert all(last[s][0][0] > 50 and len(last[s][1]) == BC[0] and len(last[s][2][0][0]) >= 8 for s in range(base.S)), last
    base.test_all_options_on_at_queue_depth_2_equal_the_single_option_handles_across_a_reset(p)

"""Shared by the speech-activity tests: a synthetic model whose blank posterior MOVES, and the threshold choice.

The seeded synthetic models give every CTC row a blank posterior of about 1 / vocabulary: nothing for a threshold to
separate.  Here the blank row of the CTC projection is scaled by 8 and its bias raised by 7, which spreads the blank
posterior of the encoder frames over (0, 1) - the rest of the model, and so everything the search does with the
other tokens' logits relative to each other, is the seeded model."""
import numpy as np

from speechcatcher_amd import synth
from speechcatcher_amd.config import SearchConfig
from speechcatcher_amd.weights import PackedWeights
from helpers import CFGS

BLANK_GAIN, BLANK_BIAS = 8.0, 7.0


def activity_state_dict(cfg, seed=1234):
    sd = synth.make_state_dict(cfg, seed)
    w, b = sd["ctc.ctc_lo.weight"].clone(), sd["ctc.ctc_lo.bias"].clone()
    w[cfg.blank_id] *= BLANK_GAIN
    b[cfg.blank_id] += BLANK_BIAS
    sd["ctc.ctc_lo.weight"], sd["ctc.ctc_lo.bias"] = w, b
    return sd


def packed_weights(cfg_name, device, seed=1234):
    cfg = CFGS[cfg_name]
    mean, std = synth.stats_to_mean_std(synth.make_stats(cfg, kind="meanstd"))
    return PackedWeights(activity_state_dict(cfg, seed), cfg, device, mean, std)


def make_batch(cfg_name, backend, n_streams, beam=3, device="cpu", weights=None, **kw):
    """backend: "native" = the C++ engine, else a backend object for the Python engine"""
    w = weights if weights is not None else packed_weights(cfg_name, device)
    sc = SearchConfig(beam_size=beam, use_bbd=True)
    if isinstance(backend, str) and backend == "native":
        from speechcatcher_amd.native import NativeStreamBatch
        return NativeStreamBatch(w, n_streams, sc, **kw)
    from speechcatcher_amd.engine import StreamBatch
    return StreamBatch(w, backend, n_streams, sc, **kw)


def pick_threshold(p_blank, lo=0.2, hi=0.9):
    """(thr, gap): the midpoint of the widest gap between consecutive sorted p_blank values in [lo, hi]"""
    s = np.sort(np.asarray(p_blank, np.float64))
    s = s[(s >= lo) & (s <= hi)]
    assert s.size >= 2, "the table must hold blank posteriors inside [0.2, 0.9]"
    d = np.diff(s)
    i = int(np.argmax(d))
    return float(0.5 * (s[i] + s[i + 1])), float(d[i])

"""Shared by the draft-transcript tests: the synthetic models the draft is run with.

"plain"   the seeded synthetic model (spot_helpers.packed_weights): its CTC arg-max path is tokens, never the blank.
"blanks"  the model of the activity tests (activity_helpers.packed_weights): blank row scaled by 8, bias + 7.  Its blank
          posterior moves over (0, 1), but with about 1 / vocabulary left for every other token the blank stays the
          arg-max of EVERY frame: the draft of this model is empty, the all-blank case at stream level.
"mixed"   blank row scaled by 4, bias + 1: the blank wins a third to a half of the frames (TINY 0.31, XL 0.48 on the
          spec engine with audio seed 5), so tokens open, close at blanks and repeat across them - the mix of tokens and
          blanks the draft is about.
What the three paths look like is asserted on the reference (path_mix) wherever they are used."""
import numpy as np

import activity_helpers
import ctc_draft_ref as R
import spot_helpers
from speechcatcher_amd import synth
from speechcatcher_amd.weights import PackedWeights
from helpers import CFGS

MIXED_GAIN, MIXED_BIAS = 4.0, 1.0
MODELS = ("plain", "blanks", "mixed")


def mixed_state_dict(cfg, seed=1234):
    sd = synth.make_state_dict(cfg, seed)
    w, b = sd["ctc.ctc_lo.weight"].clone(), sd["ctc.ctc_lo.bias"].clone()
    w[cfg.blank_id] *= MIXED_GAIN
    b[cfg.blank_id] += MIXED_BIAS
    sd["ctc.ctc_lo.weight"], sd["ctc.ctc_lo.bias"] = w, b
    return sd


def packed_weights(model, cfg_name, device, seed=1234):
    if model == "plain":
        return spot_helpers.packed_weights(cfg_name, device, seed)
    if model == "blanks":
        return activity_helpers.packed_weights(cfg_name, device, seed)
    cfg = CFGS[cfg_name]
    mean, std = synth.stats_to_mean_std(synth.make_stats(cfg, kind="meanstd"))
    return PackedWeights(mixed_state_dict(cfg, seed), cfg, device, mean, std)


def make_batch(model, cfg_name, backend, n_streams, beam=3, device="cpu", weights=None, **kw):
    """backend: "native" = the C++ engine, else a backend object for the Python engine"""
    w = weights if weights is not None else packed_weights(model, cfg_name, device)
    return spot_helpers.make_batch(cfg_name, backend, n_streams, beam, device, w, **kw)


def path_mix(model, table, blank):
    """asserts on the contract's labels of `table` what the model stands for; returns the labels"""
    lab, _ = R.rows(table, blank)
    assert (lab != R.BAD).all()
    if model == "plain":
        assert (lab != blank).all()
    elif model == "blanks":
        assert (lab == blank).all()
    else:
        frac = float((lab == blank).mean())
        assert 0.1 < frac < 0.9, frac
        assert int((np.diff((lab == blank).astype(int)) != 0).sum()) >= 6      # tokens close at blanks again and again
    return lab

"""N-gram rescoring of final n-best lists (sc_rescore_hyps / sc_lm_rescore_lists; csrc/lm_rescore.hip): the
host side of the scheduler's ``final_lm`` option.  The lists are scored and ranked on the GPU
(NativeStreamBatch.rescore_hyps); here the arrays of ``hypotheses_arrays`` are put into that order."""
import numpy as np

from . import _abi

MAX_HYPS = _abi.RESCORE_MAX_HYPS
NONFINITE, BAD_TOKEN, SERIAL = _abi.RESCORE_NONFINITE, _abi.RESCORE_BAD_TOKEN, _abi.RESCORE_SERIAL

_ROWS = ("ids", "xpos", "lens", "score", "score_dec", "score_ctc")


def rerank_arrays(arrays: dict, i: int, got: dict):
    """put the hypotheses of row ``i`` of ``hypotheses_arrays`` into the order ``got`` (one stream's entry of
    ``rescore_hyps``) gives, in place, and note per hypothesis "lm" (the model's log probability of its labels, the
    </s> term included), "fused" and "am_rank" (its row in the engine's list) in arrays of those names.  Returns the
    order: row q of the arrays is now the engine's row order[q]."""
    order = np.asarray(got["order"], np.int64)
    nh = len(order)
    n, nb = arrays["lens"].shape
    if "am_rank" not in arrays:
        arrays["lm"], arrays["fused"] = np.full((n, nb), np.nan), np.full((n, nb), np.nan)
        arrays["am_rank"] = np.full((n, nb), -1, np.int32)
    if nh:
        moved = {k: arrays[k][i, order] for k in _ROWS}   # (all read before any is written: two names may share an array)
        for k in _ROWS:
            arrays[k][i, :nh] = moved[k]
        arrays["lm"][i, :nh] = (np.asarray(got["lm"]) + np.asarray(got["eos_lm"]))[order]
        arrays["fused"][i, :nh] = np.asarray(got["fused"])[order]
        arrays["am_rank"][i, :nh] = order
    return order

"""Contract of one row of the CTC table (csrc/ctc_row.h), numpy float64: the rule the contracts of the table's scanners
share (ctc_activity_ref, ctc_spot_ref, ctc_draft_ref, ctc_alt_ref, ctc_beam_ref).

A row x[0..V) that holds a NaN or +inf, or nothing but -inf (an empty row included), is BAD.  For any other row, with x
promoted to float64:
    m = max_v x[v];  lse = m + log(sum_v exp(x[v] - m))  (v ascending)
-inf entries contribute 0.  The formula is taken as written: for logits beyond about 1e16 the term log(sum) is absorbed
when it is added to m.
"""
import numpy as np


def is_bad(row) -> bool:
    row = np.asarray(row)
    return bool(row.size == 0 or np.isnan(row).any() or (row == np.inf).any() or row.max() == -np.inf)


def lse(row) -> float:
    """m + log(sum_v exp(x[v] - m)) of a good row (any float dtype; promoted to float64), v ascending"""
    x = np.asarray(row).astype(np.float64)
    m = x.max()
    with np.errstate(under="ignore"):
        s = np.cumsum(np.exp(x - m))[-1]   # cumsum adds one element after the other: v ascending
    return float(m + np.log(s))

"""One row of the CTC table on the host, numpy float64: the rule the Python side of the table's scanners shares
(draft.py, spotting.py; csrc/ctc_row.h is the device's side, tests/ctc_row_ref.py the contract).

A row x[0..V) that holds a NaN or +inf, or nothing but -inf (an empty row included), is bad.  For any other row, with x
promoted to float64: m = max_v x[v], lse = m + log(sum_v exp(x[v] - m)), v ascending.
"""
import numpy as np


def is_bad(row) -> bool:
    row = np.asarray(row)
    return bool(row.size == 0 or np.isnan(row).any() or (row == np.inf).any() or row.max() == -np.inf)


def lse(row) -> float:
    x = np.asarray(row).astype(np.float64)
    m = x.max()
    with np.errstate(under="ignore"):
        s = np.cumsum(np.exp(x - m))[-1]   # cumsum adds one element after the other: v ascending
    return float(m + np.log(s))

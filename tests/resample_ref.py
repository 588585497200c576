"""The sample-rate conversion contract in plain numpy, written independently of csrc/resample.hip:
the float64 filter design, the output-count formulas, a float64 evaluation, and the fp32 evaluation in the canonical
order over a given f32 table (what the kernel must reproduce bit for bit).

    g = gcd(rate, 16000);  L = 16000 / g;  M = rate / g          (output m sits at input time m*M/L)
    fc = 0.94 * min(1, L/M);  W = 24 / fc;  Wc = ceil(W);  K = 2*Wc
    h(x) = fc * sinc(fc*x) * I0(10*sqrt(1-(x/W)^2)) / I0(10)   for |x| <= W, else 0
    coef[p][k] = h((k - Wc + 1) - p/L), each phase row divided by its float64 sum
    y[m] = sum_k coef[p][k] * x[n0 - Wc + 1 + k],   n0 = (m*M) div L,  p = (m*M) mod L,  x = 0 outside [0, N)
"""
import math

import numpy as np

RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000)
MAX_L = 640


def params(rate: int):
    """-> (L, M, Wc) or None for an unsupported rate"""
    if not 8000 <= rate <= 48000:
        return None
    g = math.gcd(rate, 16000)
    L, M = 16000 // g, rate // g
    if L > MAX_L:
        return None
    fc = 0.94 * min(1.0, L / M)
    return L, M, int(math.ceil(24.0 / fc))


def design(rate: int) -> np.ndarray:
    """float64 table [L][K], every phase row normalised to sum 1"""
    L, M, Wc = params(rate)
    fc = 0.94 * min(1.0, L / M)
    W = 24.0 / fc
    k = np.arange(2 * Wc, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    x = (k - Wc + 1) - p / L
    inside = np.abs(x) <= W
    r = np.where(inside, x / W, 0.0)
    h = fc * np.sinc(fc * x) * np.i0(10.0 * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / np.i0(10.0)
    h = np.where(inside, h, 0.0)
    return h / h.sum(axis=1, keepdims=True)


def out_count(rate: int, n_in_total: int, final: bool) -> int:
    L, M, Wc = params(rate)
    n = n_in_total if final else n_in_total - Wc
    return 0 if n <= 0 else -((-n * L) // M)


def _gather(x, rate, n_out, dtype):
    """-> (rows [n_out] phase of every output, taps [n_out][K] the input samples under the filter, zero padded)"""
    L, M, Wc = params(rate)
    K = 2 * Wc
    m = np.arange(n_out, dtype=np.int64)
    n0, p = (m * M) // L, (m * M) % L
    idx = n0[:, None] - Wc + 1 + np.arange(K, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    xs = np.zeros(idx.shape, dtype)
    xs[ok] = np.asarray(x, dtype)[idx[ok]]
    return p, xs


def eval_f64(x, rate: int, coef: np.ndarray, n_out=None) -> np.ndarray:
    """the whole signal, flushed, in float64 over `coef` [L][K] (any float type)"""
    n_out = out_count(rate, len(x), True) if n_out is None else n_out
    p, xs = _gather(x, rate, n_out, np.float64)
    return np.einsum("mk,mk->m", np.asarray(coef, np.float64)[p], xs)


def abs_products_f64(x, rate: int, coef: np.ndarray) -> np.ndarray:
    """sum_k |coef_k x_k| per output: the scale of the rounding-error bound of a K-term sum"""
    p, xs = _gather(x, rate, out_count(rate, len(x), True), np.float64)
    return np.einsum("mk,mk->m", np.abs(np.asarray(coef, np.float64))[p], np.abs(xs))


def eval_f32(x, rate: int, coef32: np.ndarray) -> np.ndarray:
    """the whole signal, flushed, in fp32 and the canonical order: four partial sums over k = 0, 1, 2, 3 (mod 4), each in
    ascending k, every product rounded to f32 before it is added, combined as (s0 + s1) + (s2 + s3)"""
    assert coef32.dtype == np.float32
    p, xs = _gather(np.asarray(x, np.float32), rate, out_count(rate, len(x), True), np.float32)
    c = coef32[p]
    s = [np.zeros(len(p), np.float32) for _ in range(4)]
    for k in range(c.shape[1]):
        prod = c[:, k] * xs[:, k]          # f32 * f32 -> rounded f32
        s[k % 4] = s[k % 4] + prod         # f32 + f32 -> rounded f32
    return (s[0] + s[1]) + (s[2] + s[3])

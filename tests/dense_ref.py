"""Cases, float64 references and fp32 transcriptions for the dense kernels of csrc/gemm.hip and csrc/decoder_panel.hip:
sc_gemm, sc_gemm_ln, sc_rowtile_proj, sc_ffn_ln, sc_proj_ln_proj and sc_ffn_ln_proj (fp32 forms).  numpy float64 throughout, no
GPU, and none of the arithmetic of oracle/kernel_spec.py: tests/test_dense_ref_spec.py holds these references to the torch spec
on the CPU, tests/test_gpu_dense.py holds the HIP kernels to them.

A CASE is one launch, written identically for the spec (SpecBackend, CPU) and the kernels (HipBackend).  Its buffers are larger
than what the launch names.  NaN: rows of the input that no table entry names, the columns [K, lda) of every input row, and row 0
of A in every case with a "-1 = row of zeros" gather entry (no entry names row 0 there: the kernels clamp the load of a -1 entry
onto row 0).  SENTINEL: every element of an output that the launch must not write - rows no table entry names, the columns
[N, ldc), the rows of c_rows = -1.  The torch spec reads a -1 table entry as Python does, the LAST row of the buffer: a case with
such an entry keeps one more row behind everything it names, zeros in A (so that the spec states the same operation: a row of
zeros) and nobody's in C (the spec may write it; only named rows of the spec are compared).

ERROR MODEL (dec_attn_ref.py): every reference value y comes with A(y), the sum of the absolute values of the terms a rounding
error of its computation is proportional to; a result has kappa = max |result - y| / (2^-24 A).  ReLU is 1-Lipschitz: A passes.
The constant is NOT chosen here.  kappa_ref of a case and output is the larger of the kappa the fp32 torch spec needs and the
kappa an fp32 TRANSCRIPTION of the documented summation order needs (a k-ordered chain is legitimately noisier than torch's
blocked sums); the GPU test allows a kernel 4 x kappa_ref.  The transcription of the tiled GEMM is the canonical order of
DESIGN.md section 4 itself (K < 2560: one chain; else 8 slices of ceil((K/32)/8)*32, added as a tree; bias, ReLU, residual);
the row-tile, feed-forward and panel kernels permute k inside a tile, so theirs is a plain sequential chain (per 128-wide hidden
chunk for the feed-forward, chunk results added as the aligned tree).  One rounding per term: the product is evaluated in
float64 and the sum rounded once.  It is there to MEASURE the tolerance, not to be compared for bits."""
import functools

import numpy as np
import torch

import dec_attn_ref
from dec_attn_ref import EPS, SENTINEL, layer_norm_ref, linear_ref   # noqa: F401  (EPS: re-exported)

F32, F64 = np.float32, np.float64
LN_EPS = 1e-12
FAMILIES = ("unit", "rows", "offset", "dead", "constant", "nobias")
MODES = ("plain", "relu", "residual")
KERNELS = ("gemm", "gemm_ln", "rowtile", "ffn", "panel", "ffn_proj")
MISTAKES = ("drop_k_tile", "clamped_row", "bias_tile", "relu_first", "one_pass_var", "fp16_operand", "drop_chunk", "residual_twice")

# ---------------------------------------------------------------------------------------------------------------------
# the case list (fixed; tests/test_dense_ref_spec.py asserts its coverage)
GEMM_TILE_EDGES = [(1, 4, 32), (31, 60, 64), (32, 64, 32), (33, 68, 64), (63, 128, 64), (64, 64, 64), (65, 132, 96), (127, 60, 64),
                   (128, 128, 64), (129, 68, 64), (65, 130, 64)]
GEMM_K_EDGES = [2528, 2560, 2592, 4864]
ROWTILE_M = (1, 15, 16, 17, 31, 33, 47, 49, 63, 64, 65)
FFN_M = (1, 15, 16, 17, 47, 48, 49, 79, 80, 81)
FFN_F = (128, 256, 384, 2048)
PANEL_M = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33)
FFN_PROJ_SHAPES = [(17, 128, 256, 384), (49, 256, 2048, 768), (81, 256, 384, 1024)]
GEMM_LN_SHAPES = [(1, 64, 64), (3, 256, 64), (4, 1024, 64), (5, 1028, 64), (65, 64, 2560), (65, 256, 64), (1, 256, 2560),
                  (3, 1028, 2560), (4, 1024, 2560), (5, 64, 64), (33, 256, 40)]


def case_params():
    """the parameter sets of all cases, in a fixed order: (kernel, dict)"""
    out, fam = [], 0

    def add(kernel, **p):
        nonlocal fam
        p.setdefault("family", FAMILIES[fam % len(FAMILIES)])
        fam += 1
        out.append((kernel, p))

    # sc_gemm: every tile edge twice (two families; the mode rotates; the second visit takes a row table where M allows)
    for rep in range(2):
        for i, (M, N, K) in enumerate(GEMM_TILE_EDGES):
            tables = ("", "gather", "scatter", "both")[(i + 1) % 4] if rep == 1 and M >= 31 else ""
            add("gemm", M=M, N=N, K=K, mode=MODES[(i + 2 * rep) % 3], tables=tables)
        fam += 2
    for rep in range(2):                 # K edges: the last single chain, 8 x 320, a short last slice, the subsampling Linear
        for i, K in enumerate(GEMM_K_EDGES):
            add("gemm", M=65, N=68, K=K, mode=MODES[(i + 2 * rep) % 3], tables="gather" if rep == 1 and K in (2560, 2592) else "")
        fam += 1
    for rep in range(2):                 # scalar fallbacks (K % 32 != 0; lda % 4 != 0), leading dimensions, implicit conv
        add("gemm", M=33, N=68, K=40, mode=MODES[rep], tables="both" if rep else "")
        add("gemm", M=33, N=68, K=64, lda=66, mode=MODES[1 + rep])
        add("gemm", M=65, N=68, K=64, lda=68, ldc=72, mode=MODES[2 * rep], tables="gather" if rep else "scatter")
        add("gemm", M=6, N=36, K=288, lda=32, conv=(7, 5), mode=MODES[1 - rep])
    fam = 0
    # sc_gemm_ln: residual on; with a row table, ln_out by row number and by table entry.  N = 1028 is beyond the LayerNorm
    # kernels (one wave per row, <= 1024): the call is REFUSED, and must be refused before anything is written (Case.refused;
    # the spec and the references cover it all the same).  K = 40: the scalar kernel and a LayerNorm launch of its own
    for rep in range(2):
        for i, (M, N, K) in enumerate(GEMM_LN_SHAPES):
            if rep == 0 or (M, N, K) in ((65, 256, 64), (65, 64, 2560), (5, 1028, 64), (5, 64, 64)):
                add("gemm_ln", M=M, N=N, K=K, tables="both" if rep else "", at_crows=bool(i % 2) if rep else False)
    fam = 0
    # sc_rowtile_proj: norm1 -> Linear (N = D or 3 D) and Linear + residual in place -> norm2 (N = D); lda = D + 4, ldc = N + 4
    for rep in range(2):
        for i, M in enumerate(ROWTILE_M):
            D = (128, 256)[(i + rep) % 2]
            form = ("qkv", "out", "qkv3")[(i + 2 * rep) % 3]
            add("rowtile", M=M, D=D, N=3 * D if form == "qkv3" else D, form=form[:3], ld=bool((i + rep) % 3 == 0))
        fam += 2
    fam = 0
    # sc_ffn_ln
    for rep in range(2):
        for i, M in enumerate(FFN_M):
            add("ffn", M=M, D=(128, 256)[(i + rep) % 2], F=FFN_F[(i + 3 * rep) % 4], ln=bool((i + rep) % 2 == 0),
                table=bool((i // 2 + rep) % 2))
        fam += 1
    fam = 0
    # sc_proj_ln_proj
    for i, M in enumerate(PANEL_M + (33, 17, 5)):
        add("panel", M=M, D=(64, 128, 256)[i % 3], second=bool(i % 2), table=bool((i // 2) % 2))
    fam = 0
    # sc_ffn_ln_proj
    for rep in range(2):
        for i, (M, D, F, N) in enumerate(FFN_PROJ_SHAPES):
            add("ffn_proj", M=M, D=D, F=F, N=N, table=bool((i + rep) % 2))
    return out


def kappa(got, ref, A):
    """dec_attn_ref.kappa; where A = 0 (a row of zeros without a bias: no term, no rounding) the result must be the reference
    itself"""
    got, live = np.asarray(got, F64), A > 0
    if not np.array_equal(got[~live], ref[~live]):
        return float("inf")
    return dec_attn_ref.kappa(got[live], ref[live], A[live])


# ---------------------------------------------------------------------------------------------------------------------
# float32 transcriptions
def f16(a):
    return np.asarray(a, F32).astype(np.float16).astype(F32)


def chain32(a, W):
    """[M][K] . [N][K]^T as one k-ordered chain per element from zero: acc = fl32(acc + a_k w_k)"""
    a64, W64 = a.astype(F64), W.astype(F64)
    acc = np.zeros((a.shape[0], W.shape[0]), F32)
    for k in range(a.shape[1]):
        acc = (acc + a64[:, k, None] * W64[None, :, k]).astype(F32)
    return acc


def tree8_32(parts):
    """partials added as ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)) per batch of 8 (missing ones are zeros), the batches in order"""
    acc = None
    for z0 in range(0, len(parts), 8):
        p = list(parts[z0:z0 + 8]) + [np.zeros_like(parts[0])] * (8 - len(parts[z0:z0 + 8]))
        t = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))
        acc = t if acc is None else acc + t
    return acc


def gemm32(a, W, K):
    """the canonical K cut of the tiled GEMM"""
    if K < 2560:
        return chain32(a[:, :K], W[:, :K])
    ks = -(-(K // 32) // 8) * 32
    return tree8_32([chain32(a[:, s:min(s + ks, K)], W[:, s:min(s + ks, K)]) for s in range(0, K, ks)])


def layer_norm32(x, g, b, eps, one_pass=False):
    x = x.astype(F32)
    n = F32(x.shape[-1])
    mean = x.sum(-1, keepdims=True, dtype=F32) / n
    xc = x - mean
    if one_pass:
        var = (x * x).sum(-1, keepdims=True, dtype=F32) / n - mean * mean
    else:
        var = (xc * xc).sum(-1, keepdims=True, dtype=F32) / n
    with np.errstate(invalid="ignore", divide="ignore"):
        rstd = F32(1.0) / np.sqrt(var + F32(eps))
    return xc * rstd * g.astype(F32) + b.astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """One launch.  inputs / tables: what the launch reads (name -> array); init: the content of every buffer it writes before
    the launch; ref, A: the float64 reference of every output over the WHOLE buffer and its error scale (NaN where the launch
    writes nothing); named: the mask of the elements it writes."""

    def __init__(self, kernel, idx=0, **p):
        self.kernel, self.p, self.family = kernel, dict(p), p["family"]
        self.rng = np.random.default_rng([KERNELS.index(kernel), idx, FAMILIES.index(self.family)])
        self.inputs, self.tables, self.init, self.ref, self.A, self.named = {}, {}, {}, {}, {}, {}
        self.name = kernel + ":" + ",".join(f"{k}={v}" for k, v in p.items())
        self.refused = kernel == "gemm_ln" and p["N"] > 1024
        getattr(self, "_build_" + kernel)()

    # -- data
    def _data(self, n, width, lnorm=False, scale=1.0):
        """n rows of input by family; returns the rows and the indices of the family's special rows (dead / constant)"""
        rng, fam = self.rng, self.family
        x = rng.standard_normal((n, width)) * scale
        special = np.zeros(n, bool)
        if fam == "rows":
            x *= np.logspace(-3, 2, n)[rng.permutation(n)][:, None]
        elif fam == "offset":
            x += 100.0
        elif fam in ("dead", "constant"):
            special[::3] = True
            x[special] = 0.0                                   # a zero row: the Linear returns its bias
            x[~special] *= 3.0
            if lnorm and fam == "constant":                    # the row feeds a LayerNorm directly: one value, variance 0
                x[special] = rng.choice([-3.0, 0.5, 2.0, 0.0], (int(special.sum()), 1))
        return x.astype(F32), special

    def _weight(self, N, K, unscale=False):
        """N(0, 1/K); unscale: a Linear that takes the offset family's 100 + N(0,1) and feeds a residual add in front of a
        LayerNorm is scaled by 1/100 - its products still cancel, and the LayerNorm sees |mean| >> deviation"""
        W = self.rng.standard_normal((N, K)) / np.sqrt(K)
        return (W / 100.0 if unscale and self.family == "offset" else W).astype(F32)

    def _bias(self, N, feeds_relu=False, feeds_ln=False):
        if self.family == "nobias":
            return None
        b = self.rng.standard_normal(N)
        if self.family in ("dead", "constant") and feeds_relu:
            b = -np.abs(b) - 0.5                               # zero rows: every pre-activation negative, ReLU gives exact zeros
        elif self.family == "constant" and feeds_ln:
            b = np.full(N, 0.25)                               # zero rows + a constant residual: a constant row for the LayerNorm
        return b.astype(F32)

    def _residual_rows(self, n, N, special):
        x = self.rng.standard_normal((n, N))
        if self.family == "rows":
            x *= np.logspace(-2, 2, n)[:, None]
        elif self.family == "offset":
            x += 100.0
        elif self.family == "constant":
            x[special] = self.rng.choice([-3.0, 0.5, 2.0], (int(special.sum()), 1))
        return x.astype(F32)

    def _ln_params(self, N):
        return (1.0 + 0.1 * self.rng.standard_normal(N)).astype(F32), self.rng.standard_normal(N).astype(F32)

    def _table(self, M, n_buf, lo=0, minus=0, dup=False):
        """M distinct entries of lo .. n_buf - 1 in random order; `dup`: two of them repeated; `minus` of them -1"""
        t = self.rng.permutation(np.arange(lo, n_buf))[:M].astype(np.int32)
        if dup and M >= 8:
            t[5], t[M - 2] = t[1], t[2]
        for j in range(minus):
            t[(3 + 11 * j) % M] = -1
        return t

    def _out(self, name, n_rows, ld, rows, N, val, A, init_rows=None):
        """registers an output buffer [n_rows][ld]: rows[m] >= 0 receives val[m] in its first N columns"""
        init = np.full((n_rows, ld), SENTINEL, F32)
        ref, Ar, named = np.full((n_rows, ld), np.nan), np.full((n_rows, ld), np.nan), np.zeros((n_rows, ld), bool)
        ok = rows >= 0
        if init_rows is not None:
            init[rows[ok], :N] = init_rows[ok]
        ref[rows[ok], :N], Ar[rows[ok], :N], named[rows[ok], :N] = val[ok], A[ok], True
        self.init[name], self.ref[name], self.A[name], self.named[name] = init, ref, Ar, named

    def _in(self, name, n_rows, ld, rows, width, val):
        """registers an input buffer [n_rows][ld], NaN except the first `width` columns of rows[m] >= 0"""
        buf = np.full((n_rows, ld), np.nan, F32)
        ok = rows >= 0
        buf[rows[ok], :width] = val[ok]
        self.inputs[name] = buf
        return buf

    # -- sc_gemm / sc_gemm_ln
    def _gemm_operands(self, feeds_ln=False):
        p = self.p
        M, N, K = p["M"], p["N"], p["K"]
        lda, ldc, tables, conv = p.get("lda", K), p.get("ldc", N), p.get("tables", ""), p.get("conv")
        mode = p.get("mode", "residual")
        gather, scatter = tables in ("gather", "both"), tables in ("scatter", "both")
        self.poisoned = gather
        if conv:                                               # second Conv2d of the subsampling as an implicit GEMM
            F1, T1 = conv
            F2, T2 = (F1 - 3) // 2 + 1, (T1 - 3) // 2 + 1
            assert M == T2 * F2 and K == 9 * lda
            tt, ff = np.meshgrid(np.arange(T2), np.arange(F2), indexing="ij")
            a_rows = (2 * tt * F1 + 2 * ff).reshape(-1).astype(np.int32)
            tap = np.arange(K) // lda
            kofs = ((tap // 3) * F1 + tap % 3) * lda + np.arange(K) % lda
            n_named = T1 * F1
            x, special = self._data(n_named, lda)
            Abuf = np.full((n_named + 5, lda), np.nan, F32)
            Abuf[:n_named] = x
            self.tables["a_rows"] = a_rows
        else:
            kofs = np.arange(K)
            nA = M + 7 + (1 if gather else 0)
            a_rows = self._table(M, nA - 1, lo=1, minus=2, dup=True) if gather else np.arange(M, dtype=np.int32)
            x, _ = self._data(M, K)
            Abuf = self._in("A", nA, lda, a_rows, K, x)        # (a row named twice holds the data of its last entry)
            if gather:
                Abuf[nA - 1] = 0.0                             # (the torch spec's reading of -1, see the module docstring)
                self.tables["a_rows"] = a_rows
        self.inputs["A"] = Abuf
        flat = Abuf.reshape(-1).astype(F64)
        a = np.where((a_rows >= 0)[:, None], flat[np.maximum(a_rows, 0)[:, None].astype(np.int64) * lda + kofs[None, :]], 0.0)
        a_clamped = flat[np.maximum(a_rows, 0)[:, None].astype(np.int64) * lda + kofs[None, :]]      # a planted mistake reads this
        special = (a == 0).all(1)                              # zero rows (and -1 entries): the Linear returns its bias
        W = self._weight(N, K, unscale=feeds_ln)
        bias = self._bias(N, feeds_relu=mode == "relu", feeds_ln=feeds_ln)
        self.inputs["W"] = W
        if bias is not None:
            self.inputs["bias"] = bias
        nC = M + 6 + (1 if scatter else 0)
        c_rows = self._table(M, nC - 1, minus=0 if self.kernel == "gemm_ln" else 1) if scatter else np.arange(M, dtype=np.int32)
        if scatter:
            self.tables["c_rows"] = c_rows
        old = self._residual_rows(M, N, special) if mode == "residual" else None
        self._g = dict(a=a, a_clamped=a_clamped, W=W, bias=bias, old=old, c_rows=c_rows, nC=nC, ldc=ldc, mode=mode)
        y, Ay = linear_ref(a, np.zeros_like(a), W.astype(F64), 0.0 if bias is None else bias.astype(F64))
        if mode == "relu":
            y = np.maximum(y, 0.0)
        if mode == "residual":
            y, Ay = old + y, np.abs(old) + Ay
        self._out("C", nC, ldc, c_rows, N, y, Ay, init_rows=old)
        return y, Ay

    def _build_gemm(self):
        self._gemm_operands()

    def _build_gemm_ln(self):
        p = self.p
        y, Ay = self._gemm_operands(feeds_ln=True)
        g, b = self._ln_params(p["N"])
        self.inputs["ln_g"], self.inputs["ln_b"] = g, b
        ln, Aln = layer_norm_ref(y, Ay, g.astype(F64), b.astype(F64), LN_EPS)
        rows = self._g["c_rows"] if p["at_crows"] else np.arange(p["M"], dtype=np.int32)
        self._out("ln_out", self._g["nC"] if p["at_crows"] else p["M"] + 3, p["N"], rows, p["N"], ln, Aln)

    def _gemm32(self, mistake):
        g, p = self._g, self.p
        N, K = p["N"], p["K"]
        a = (g["a_clamped"] if mistake == "clamped_row" else g["a"]).astype(F32)
        if mistake == "fp16_operand":
            a = f16(a)
        acc = gemm32(a, g["W"], K - 32 if mistake == "drop_k_tile" else K)
        if g["bias"] is not None:
            b = g["bias"].copy()
            if mistake == "bias_tile":
                b[(N - 1) // 64 * 64:] = 0.0
            acc = (np.maximum(acc, F32(0)) + b) if mistake == "relu_first" else acc + b
        if g["mode"] == "relu" and mistake != "relu_first":
            acc = np.maximum(acc, F32(0))
        if g["mode"] == "residual":
            acc = g["old"] + acc
            if mistake == "residual_twice":
                acc = g["old"] + acc
        return acc

    # -- sc_rowtile_proj
    def _build_rowtile(self):
        p = self.p
        M, D, N, form = p["M"], p["D"], p["N"], p["form"]
        lda, ldc = (D + 4, N + 4) if p["ld"] else (D, N)
        self.poisoned = False
        rows = np.arange(M, dtype=np.int32)
        x, special = self._data(M, D, lnorm=form == "qkv")
        self._in("A", M + 5, lda, rows, D, x)
        W, bias = self._weight(N, D, unscale=form == "out"), self._bias(N, feeds_ln=form == "out")
        self.inputs["W"] = W
        if bias is not None:
            self.inputs["bias"] = bias
        g, b = self._ln_params(D)
        self.inputs["ln_g"], self.inputs["ln_b"] = g, b
        b64 = 0.0 if bias is None else bias.astype(F64)
        self._r = dict(x=x, W=W, bias=bias, g=g, b=b)
        if form == "qkv":
            xn, Axn = layer_norm_ref(x.astype(F64), np.zeros((M, D)), g.astype(F64), b.astype(F64), LN_EPS)
            y, Ay = linear_ref(xn, Axn, W.astype(F64), b64)
            self._out("C", M + 3, ldc, rows, N, y, Ay)
        else:
            old = self._residual_rows(M, D, special)
            self._r["old"] = old
            y, Ay = linear_ref(x.astype(F64), np.zeros((M, D)), W.astype(F64), b64)
            y, Ay = old + y, np.abs(old) + Ay
            self._out("C", M + 3, ldc, rows, N, y, Ay, init_rows=old)
            self._out("LN2", M + 3, D, rows, D, *layer_norm_ref(y, Ay, g.astype(F64), b.astype(F64), LN_EPS))

    def _rowtile32(self, mistake):
        r, form = self._r, self.p["form"]
        one_pass = mistake == "one_pass_var"
        x = r["x"]
        if form == "qkv":
            x = layer_norm32(x, r["g"], r["b"], LN_EPS, one_pass)
        if mistake == "fp16_operand":
            x = f16(x)
        K = x.shape[1] - (32 if mistake == "drop_k_tile" else 0)
        c = chain32(x[:, :K], r["W"][:, :K])
        if r["bias"] is not None:
            c = c + r["bias"]
        if form == "qkv":
            return {"C": c}
        c = r["old"] + c
        if mistake == "residual_twice":
            c = r["old"] + c
        return {"C": c, "LN2": layer_norm32(c, r["g"], r["b"], LN_EPS, one_pass)}

    # -- sc_ffn_ln / sc_ffn_ln_proj / sc_proj_ln_proj share the row addressing: rows of XN, X, ln_out, Q through ONE table
    def _row_table(self, M, table):
        n = M + 5
        rows = self._table(M, n) if table else np.arange(M, dtype=np.int32)
        if table:
            self.tables["rows"] = rows
        return n, rows

    def _ffn_operands(self):
        p = self.p
        M, D, Fd = p["M"], p["D"], p["F"]
        self.poisoned = False
        n, rows = self._row_table(M, p["table"])
        xn, special = self._data(M, D)
        self._in("XN", n, D, rows, D, xn)
        W1, b1 = self._weight(Fd, D, unscale=True), self._bias(Fd, feeds_relu=True)
        W2, b2 = self._weight(D, Fd), self._bias(D, feeds_ln=True)
        x = self._residual_rows(M, D, special)
        self.inputs["W1"], self.inputs["W2"] = W1, W2
        if b1 is not None:
            self.inputs["b1"], self.inputs["b2"] = b1, b2
        z = lambda v: 0.0 if v is None else v.astype(F64)   # noqa: E731
        h, Ah = linear_ref(xn.astype(F64), np.zeros((M, D)), W1.astype(F64), z(b1))
        h = np.maximum(h, 0.0)
        if self.family in ("dead", "constant"):
            assert special.any() and (h[special] == 0).all()   # the family is what it is called
        y, Ay = linear_ref(h, Ah, W2.astype(F64), z(b2))
        y, Ay = x + y, np.abs(x) + Ay
        self._f = dict(xn=xn, W1=W1, b1=b1, W2=W2, b2=b2, x=x, n=n, rows=rows, special=special)
        return n, rows, x, y, Ay

    def _build_ffn(self):
        p = self.p
        n, rows, x, y, Ay = self._ffn_operands()
        self._out("X", n, p["D"], rows, p["D"], y, Ay, init_rows=x)
        g, b = self._ln_params(p["D"])
        self.inputs["ln_g"], self.inputs["ln_b"] = g, b
        self._f.update(g=g, b=b)
        if p["ln"]:
            self._out("ln_out", n, p["D"], rows, p["D"], *layer_norm_ref(y, Ay, g.astype(F64), b.astype(F64), LN_EPS))

    def _ffn32(self, mistake):
        f, Fd = self._f, self.p["F"]
        xn = f16(f["xn"]) if mistake == "fp16_operand" else f["xn"]
        h = chain32(xn, f["W1"])
        if f["b1"] is not None:
            h = (np.maximum(h, F32(0)) + f["b1"]) if mistake == "relu_first" else h + f["b1"]
        if mistake != "relu_first":
            h = np.maximum(h, F32(0))
        nch = Fd // 128 - (1 if mistake == "drop_chunk" else 0)
        acc = tree8_32([chain32(h[:, c * 128:(c + 1) * 128], f["W2"][:, c * 128:(c + 1) * 128]) for c in range(nch)]) \
            if nch else np.zeros_like(f["x"])
        if f["b2"] is not None:
            acc = acc + f["b2"]
        x = f["x"] + acc
        if mistake == "residual_twice":
            x = f["x"] + x
        return x

    def _build_ffn_proj(self):
        p = self.p
        D, N = p["D"], p["N"]
        n, rows, x, y, Ay = self._ffn_operands()
        self._in("Xin", n, D, rows, D, x)                      # read-only; Xout is another buffer
        self._out("Xout", n, D, rows, D, y, Ay)
        g, b = self._ln_params(D)
        Wq, bq = self._weight(N, D), self._bias(N)
        self.inputs["ln_g"], self.inputs["ln_b"], self.inputs["Wq"] = g, b, Wq
        if bq is not None:
            self.inputs["bq"] = bq
        self._f.update(g=g, b=b, Wq=Wq, bq=bq)
        xn, Axn = layer_norm_ref(y, Ay, g.astype(F64), b.astype(F64), LN_EPS)
        self._out("Q", n, N, rows, N, *linear_ref(xn, Axn, Wq.astype(F64), 0.0 if bq is None else bq.astype(F64)))

    # -- sc_proj_ln_proj
    def _build_panel(self):
        p = self.p
        M, D = p["M"], p["D"]
        self.poisoned = False
        n, rows = self._row_table(M, p["table"])
        a, special = self._data(M, D)
        self._in("A", n, D, rows, D, a)
        W1, b1 = self._weight(D, D, unscale=True), self._bias(D, feeds_ln=True)
        x = self._residual_rows(M, D, special)
        g, b = self._ln_params(D)
        self.inputs["W1"], self.inputs["ln_g"], self.inputs["ln_b"] = W1, g, b
        if b1 is not None:
            self.inputs["b1"] = b1
        z = lambda v: 0.0 if v is None else v.astype(F64)   # noqa: E731
        y, Ay = linear_ref(a.astype(F64), np.zeros((M, D)), W1.astype(F64), z(b1))
        y, Ay = x + y, np.abs(x) + Ay
        self._out("X", n, D, rows, D, y, Ay, init_rows=x)
        xn, Axn = layer_norm_ref(y, Ay, g.astype(F64), b.astype(F64), LN_EPS)
        self._p = dict(a=a, W1=W1, b1=b1, x=x, g=g, b=b)
        if p["second"]:
            W2, b2 = self._weight(D, D), self._bias(D)
            self.inputs["W2"] = W2
            if b2 is not None:
                self.inputs["b2"] = b2
            self._p.update(W2=W2, b2=b2)
            self._out("Q", n, D, rows, D, *linear_ref(xn, Axn, W2.astype(F64), z(b2)))
        else:
            self._out("XN", n, D, rows, D, xn, Axn)

    def _panel32(self, mistake):
        q = self._p
        a = f16(q["a"]) if mistake == "fp16_operand" else q["a"]
        K = a.shape[1] - (32 if mistake == "drop_k_tile" else 0)
        y = chain32(a[:, :K], q["W1"][:, :K])
        if q["b1"] is not None:
            y = y + q["b1"]
        x = q["x"] + y
        if mistake == "residual_twice":
            x = q["x"] + x
        xn = layer_norm32(x, q["g"], q["b"], LN_EPS, mistake == "one_pass_var")
        if not self.p["second"]:
            return {"X": x, "XN": xn}
        y = chain32(xn, q["W2"])
        return {"X": x, "Q": y if q["b2"] is None else y + q["b2"]}

    # -- the transcription of the whole launch: output name -> [M][N] float32 rows (in launch order)
    def transcription(self, mistake=None):
        p, k = self.p, self.kernel
        if k in ("gemm", "gemm_ln"):
            out = {"C": self._gemm32(mistake)}
            if k == "gemm_ln":
                out["ln_out"] = layer_norm32(out["C"], self.inputs["ln_g"], self.inputs["ln_b"], LN_EPS, mistake == "one_pass_var")
            return out
        if k == "rowtile":
            return self._rowtile32(mistake)
        if k == "panel":
            return self._panel32(mistake)
        x = self._ffn32(mistake)
        f = self._f
        if k == "ffn":
            out = {"X": x}
            if p["ln"]:
                out["ln_out"] = layer_norm32(x, f["g"], f["b"], LN_EPS, mistake == "one_pass_var")
            return out
        xn = layer_norm32(x, f["g"], f["b"], LN_EPS, mistake == "one_pass_var")
        q = chain32(xn, f["Wq"])
        return {"Xout": x, "Q": q if f["bq"] is None else q + f["bq"]}

    def out_rows(self, name):
        """buffer rows of the launch's rows, in launch order (-1: not written)"""
        if self.kernel in ("gemm", "gemm_ln"):
            if name == "C" or self.p.get("at_crows"):
                return self._g["c_rows"]
            return np.arange(self.p["M"], dtype=np.int32)
        if self.kernel == "rowtile":
            return np.arange(self.p["M"], dtype=np.int32)
        return self.tables.get("rows", np.arange(self.p["M"], dtype=np.int32))

    def output_names(self):
        return tuple(self.ref)

    # -- kappas
    def kappas_of_rows(self, outs):
        """outs: name -> [M][N] rows in launch order (a transcription)"""
        res = {}
        for name, v in outs.items():
            rows = self.out_rows(name)
            ok = rows >= 0
            N = v.shape[1]
            res[name] = kappa(v[ok], self.ref[name][rows[ok], :N], self.A[name][rows[ok], :N])
        return res

    def kappas_of_buffers(self, bufs):
        """bufs: name -> the whole output buffer after a launch"""
        return {name: kappa(np.asarray(bufs[name], F64)[self.named[name]], self.ref[name][self.named[name]],
                            self.A[name][self.named[name]]) for name in self.ref}

    def sentinel_problems(self, bufs):
        bad = []
        for name in self.ref:
            keep = ~self.named[name]
            if not np.array_equal(np.asarray(bufs[name])[keep].view(np.int32), self.init[name][keep].view(np.int32)):
                bad.append(f"{name}: an element the launch does not name was written")
        return bad


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(Case(k, i, **p) for i, (k, p) in enumerate(case_params()))


def cases_of(kernel):
    return [c for c in all_cases() if c.kernel == kernel]


# ---------------------------------------------------------------------------------------------------------------------
# the launches: the same call on a SpecBackend (CPU) and a HipBackend
def tensors(case, device="cpu"):
    """name -> torch tensor of every buffer of the case (weights packed as the kernel wants them)"""
    from speechcatcher_amd.weights import pack_lane_weight, pack_panel_weight
    t = {}
    for name, a in {**case.inputs, **case.tables, **case.init}.items():
        v = torch.from_numpy(np.array(a))                     # (a copy: a CPU launch must not write into the case)
        if case.kernel in ("ffn", "ffn_proj", "rowtile") and name in ("W", "W1", "W2"):
            v = pack_panel_weight(v)
        elif name == "Wq" or (case.kernel == "panel" and name in ("W1", "W2")):
            v = pack_lane_weight(v)
        t[name] = v.to(device)
    return t


def launch(be, case, t, naive=False):
    p, k, g = case.p, case.kernel, t.get
    if k in ("gemm", "gemm_ln"):
        M, N, K = p["M"], p["N"], p["K"]
        lda, ldc, conv = p.get("lda", K), p.get("ldc", N), p.get("conv")
        kw = dict(conv_f1=conv[0] if conv else 0, residual=p.get("mode", "residual") == "residual")
        if k == "gemm":
            if naive:
                kw["naive"] = True
            be.gemm(t["A"], g("a_rows"), lda, t["W"], g("bias"), t["C"], g("c_rows"), ldc, M, N, K, relu=p["mode"] == "relu", **kw)
        else:
            be.gemm_ln(t["A"], g("a_rows"), lda, t["W"], g("bias"), t["C"], g("c_rows"), ldc, M, N, K, t["ln_g"], t["ln_b"],
                       t["ln_out"], ln_at_crows=p["at_crows"], eps=LN_EPS, **kw)
    elif k == "rowtile":
        if p["form"] == "qkv":
            be.rowtile_proj(t["A"], p["M"], p["D"], t["W"], g("bias"), p["N"], t["C"], ln_g=t["ln_g"], ln_b=t["ln_b"], eps=LN_EPS)
        else:
            be.rowtile_proj(t["A"], p["M"], p["D"], t["W"], g("bias"), p["N"], t["C"], R=t["C"], g2=t["ln_g"], b2=t["ln_b"],
                            LN2=t["LN2"], eps=LN_EPS)
    elif k == "ffn":
        be.ffn_ln(t["XN"], g("rows"), p["M"], p["D"], p["F"], t["W1"], g("b1"), t["W2"], g("b2"), t["X"], t["ln_g"], t["ln_b"],
                  g("ln_out"), eps=LN_EPS)
    elif k == "ffn_proj":
        be.ffn_ln_proj(t["XN"], g("rows"), p["M"], p["D"], p["F"], t["W1"], g("b1"), t["W2"], g("b2"), t["Xin"], t["Xout"],
                       t["ln_g"], t["ln_b"], t["Wq"], g("bq"), t["Q"], p["N"], eps=LN_EPS)
    else:
        be.proj_ln_proj(t["A"], p["D"], t["W1"], g("b1"), t["X"], p["D"], t["ln_g"], t["ln_b"], g("XN"), g("W2"), g("b2"), g("Q"),
                        p["M"], p["D"], eps=LN_EPS, rows=g("rows"))


def outputs(case, t):
    return {name: t[name].detach().cpu().numpy() for name in case.ref}


def spec_kappas(case):
    """the kappa the fp32 torch spec needs on this case, per output (inf: the spec read a poisoned element)"""
    from oracle.kernel_spec import SpecBackend
    t = tensors(case)
    launch(SpecBackend(), case, t)
    return case.kappas_of_buffers(outputs(case, t))


@functools.lru_cache(maxsize=None)
def _kappa_ref(i):
    case = all_cases()[i]
    ks, kt = spec_kappas(case), case.kappas_of_rows(case.transcription())
    return {n: (ks[n], kt[n], max(ks[n], kt[n])) for n in ks}


def kappa_ref(case):
    """output name -> (spec kappa, transcription kappa, kappa_ref = the larger); measured once per process"""
    return _kappa_ref(all_cases().index(case))

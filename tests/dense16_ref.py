"""Cases, float64 references, error model and numpy transcriptions for the REDUCED-PRECISION forms of the dense kernels of
csrc/gemm.hip: sc_gemm with SC_GEMM_SPLIT16 (gemm_s), sc_rowtile_proj_s / _h (rowtile_s, rowtile_h) and sc_ffn_ln_s / _h (ffn_s,
ffn_h).  Built on tests/dense_ref.py (Case plumbing, poison, sentinels, tables, kappa); numpy float64 throughout, no GPU, none of
the arithmetic of oracle/kernel_spec.py.  tests/test_dense16_ref_spec.py holds this module to the fp32 spec and to itself on the
CPU, tests/test_gpu_dense16.py holds the HIP kernels to it.

FORMS.  split16 (`_s`): every operand x is split into hi = fp16(x), lo = fp16((x - hi) * 2^11) and a product sum is evaluated as
sum(a_hi b_hi) + 2^-11 (sum(a_hi b_lo) + sum(a_lo b_hi)) with fp32 accumulators.  float16 (`_h`): the weights ARE fp16 numbers
(the reference takes them as given), the activations are rounded to fp16 when staged, fp32 accumulators.

ERROR MODEL.  A(y) and the unit 2^-24 of dense_ref, plus the representation error the form is documented to have:
  split16   E(y) = 2^-24 A(y) + sum_k ( |a_k| rho(w_k) + |w_k| rho(a_k) + r(a_k) r(w_k) ),
            rho(x) = max(2^-22 |x|, 2^-36),  r(x) = max(2^-11 |x|, 2^-25)       (the last summand: the dropped lo . lo term)
  float16   E(y) = 2^-24 A(y) + sum_k |w_k| r(a_k)
with rho(0) = r(0) = 0: a zero splits exactly (stricter than the formula, and what keeps "a row of zeros gives the bias itself").
2^-36 is the floor of the split: below 2^-14 hi is an fp16 subnormal (or zero) and x - hi <= 2^-25 is carried by a lo whose own
quantum is 2^-24 / 2^11.  The feed-forward carries the hidden activation's error through |W2| and adds the hidden activation's
own rounding there; LayerNorm outputs propagate as in dense_ref.  The module keeps E in the units of A (A + 2^24 R), so that
dense_ref.kappa applies unchanged: kappa = max |result - y| / E(y), and where E = 0 the result must be the reference itself.

kappa_ref of a case and output is the kappa the TRANSCRIPTION of the documented arithmetic needs: the splits in np.float16 as
ffn_split4 / split_panel_weight write them, each of the three sums a k-ordered chain with one rounding to fp32 per term, chunk
results added as the aligned tree, the K >= 2560 GEMM as 8 slices (each folds its cross sums), the `_h` forms with operands
rounded to fp16 and fp32 chains.  The GPU test allows a kernel 4 x kappa_ref.  An unaligned sc_gemm call (K = 40) goes to the
fp32 scalar kernel whatever the flag says: that case keeps the fp32 model and the fp32 chain.

ffn_h has a second measure, "X@form": the launch against the float64 evaluation OF THE FORM (xn and the hidden row rounded to
fp16, sums exact) under the fp32 model alone, plus one fp16 ulp for every hidden element that lies within 8 * 2^-24 A(h) of a
rounding boundary (an fp32 sum may fall on the other side).  A kernel that keeps the hidden row in fp32 is CLOSER to the exact
reference, and only this measure sees it (mistake hidden_fp32_in_h)."""
import functools

import numpy as np
import torch

import dense_ref as dr
from dense_ref import F32, F64, LN_EPS, MODES, SENTINEL, chain32, f16, layer_norm32, tree8_32   # noqa: F401
from dec_attn_ref import layer_norm_ref, linear_ref

F16 = np.float16
KERNELS = ("gemm_s", "rowtile_s", "rowtile_h", "ffn_s", "ffn_h")
FAMILIES = dr.FAMILIES + ("small", "mixed", "edge", "neg")
MISTAKES = ("drop_cross_term", "cross_unscaled", "lo_unscaled_before_rounding", "hi_only", "flush_subnormal", "fold_after_relu",
            "clamped_row", "hidden_fp32_in_h")
FFN_M = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 79, 80, 81)
FFN_F = dr.FFN_F
U24 = 2.0 ** 24
FP16_BIG = float(np.nextafter(F32(65520.0), F32(0.0)))          # the largest fp32 that still rounds to 65504
# values on fp16's boundaries: the smallest normal, the smallest subnormal, the tie to zero, +-0, and values whose residual
# (x - hi) * 2^11 lands on 2^-14 (x = 2^-e + 2^-25: hi = 2^-e, lo = the smallest normal)
EDGE_VALUES = np.array([s * v for v in (2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 0.0, 2.0 ** -3 + 2.0 ** -25, 2.0 ** -8 + 2.0 ** -25,
                                        2.0 ** -13 + 2.0 ** -25) for s in (1.0, -1.0)])


def base_kernel(kernel):
    return kernel[:-2]


def form_of(kernel):
    return "split16" if kernel.endswith("_s") else "float16"


# ---------------------------------------------------------------------------------------------------------------------
def case_params():
    """(kernel, dict) of all cases, in a fixed order; the ten families rotate"""
    out, fam = [], 0

    def add(kernel, **p):
        nonlocal fam
        p.setdefault("family", FAMILIES[fam % len(FAMILIES)])
        fam += 1
        out.append((kernel, p))

    edges = [e for e in dr.GEMM_TILE_EDGES if e[2] % 32 == 0]
    for rep in range(2):                 # every tile edge twice; the second visit takes a row table where M allows
        for i, (M, N, K) in enumerate(edges):
            tables = ("", "gather", "scatter", "both")[(i + 1) % 4] if rep == 1 and M >= 31 else ""
            add("gemm_s", M=M, N=N, K=K, mode=MODES[(i + 2 * rep) % 3], tables=tables)
        fam += 3
    for i, K in enumerate(dr.GEMM_K_EDGES):          # the last single chain, 8 x 320, a short last slice, the subsampling Linear
        add("gemm_s", M=65, N=68, K=K, mode=MODES[i % 3], tables="gather" if K in (2560, 2592) else "")
    add("gemm_s", M=6, N=36, K=288, lda=32, conv=(7, 5), mode="relu")
    add("gemm_s", M=65, N=68, K=64, lda=68, ldc=72, mode="plain", tables="both")
    add("gemm_s", M=65, N=68, K=64, lda=68, ldc=72, mode="residual", tables="gather")
    add("gemm_s", M=65, N=68, K=64, lda=68, ldc=72, mode="relu", tables="scatter")
    add("gemm_s", M=33, N=68, K=40, mode="plain", tables="both", family="nobias")       # unaligned: the fp32 scalar kernel
    add("gemm_s", M=33, N=68, K=40, mode="relu", tables="", family="rows")
    for kernel in ("rowtile_s", "rowtile_h"):
        fam = 0
        for rep in range(2):
            for i, M in enumerate(dr.ROWTILE_M):
                D = (128, 256)[(i + rep) % 2]
                form = ("qkv", "out", "qkv3")[(i + 2 * rep) % 3]
                add(kernel, M=M, D=D, N=3 * D if form == "qkv3" else D, form=form[:3], ld=bool((i + rep) % 3 == 0))
            fam += 3
    for kernel in ("ffn_s", "ffn_h"):
        fam = 0
        for rep in range(2):
            for i, M in enumerate(FFN_M):
                add(kernel, M=M, D=(128, 256)[(i + rep + 1) % 2], F=FFN_F[(i + 3 * rep) % 4], ln=bool((i + rep) % 2 == 0),
                    table=bool((i // 2 + rep) % 2))
            fam += 3
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the representation terms of the error model (float64, in the units of the value)
def _rho(x):
    x = np.abs(x)
    return np.where(x == 0, 0.0, np.maximum(2.0 ** -22 * x, 2.0 ** -36))


def _r(x):
    x = np.abs(x)
    return np.where(x == 0, 0.0, np.maximum(2.0 ** -11 * x, 2.0 ** -25))


def rep_term(form, a, W):
    """-> (R, the part of R that the floor contributes) for y = a . W^T, [M][N].  The floor's part: every term in which an
    operand below 2^-14 stands with its constant bound - rho = 2^-36, and r = 2^-25 in the dropped lo . lo product (for such an
    operand r(a) r(w) = 2^-36 |w|, the size of the rho term itself)"""
    a, W = np.asarray(a, F64), np.asarray(W, F64)
    if form == "float16":
        return _r(a) @ np.abs(W).T, np.zeros((a.shape[0], W.shape[0]))
    ra, rw = _rho(a), _rho(W)
    R = np.abs(a) @ rw.T + ra @ np.abs(W).T + _r(a) @ _r(W).T
    fa, fw = ra == 2.0 ** -36, rw == 2.0 ** -36                    # operands below 2^-14: their terms are the floor's
    fl = np.abs(a) @ np.where(fw, rw, 0.0).T + np.where(fa, ra, 0.0) @ np.abs(W).T
    fl += np.where(fa, _r(a), 0.0) @ _r(W).T + np.where(fa, 0.0, _r(a)) @ np.where(fw, _r(W), 0.0).T
    return R, fl


# ---------------------------------------------------------------------------------------------------------------------
# transcriptions
def split16(x, mistake=None):
    """hi = fp16(x), lo = fp16((x - hi) * 2^11), as ffn_split4 and split_panel_weight write them; as float32 values"""
    x = np.asarray(x, F32)
    hi = x.astype(F16).astype(F32)
    d = x - hi                                                   # exact in fp32
    lo = (d if mistake == "lo_unscaled_before_rounding" else d * F32(2048.0)).astype(F16).astype(F32)
    if mistake == "flush_subnormal":
        hi = np.where(np.abs(hi) < F32(2.0 ** -14), F32(0), hi)
        lo = np.where(np.abs(lo) < F32(2.0 ** -14), F32(0), lo)
    return hi, lo


def half(x, mistake=None):
    h = f16(x)
    return np.where(np.abs(h) < F32(2.0 ** -14), F32(0), h) if mistake == "flush_subnormal" else h


def split_sum(a, W, mistake=None):
    """-> (sum a_hi w_hi, the cross term ready to be added), float32 [M][N]"""
    ah, al = split16(a, mistake)
    wh, wl = split16(W, mistake)
    hh = chain32(ah, wh)
    if mistake == "hi_only":
        return hh, np.zeros_like(hh)
    c = chain32(ah, wl)
    if mistake != "drop_cross_term":
        c = c + chain32(al, wh)
    if mistake in ("cross_unscaled", "lo_unscaled_before_rounding"):
        return hh, c
    return hh, c * F32(1.0 / 2048.0)


class Case(dr.Case):
    """One launch of a reduced-precision form.  self.kernel is the name of the fp32 kernel (dense_ref's launch, tensors and
    row addressing apply), self.kernel16 the form's; A: the form's error scale, A32: the fp32 model's (the spec is held to it);
    floor: the floor's part of the direct output's scale."""

    def __init__(self, kernel16, idx=0, **p):
        self.kernel16, self.kernel, self.form = kernel16, base_kernel(kernel16), form_of(kernel16)
        self.p, self.family = dict(p), p["family"]
        self.rng = np.random.default_rng([16, KERNELS.index(kernel16), idx, FAMILIES.index(self.family)])
        self.inputs, self.tables, self.init, self.ref, self.A, self.named = {}, {}, {}, {}, {}, {}
        self.A32, self.floor, self.form_ref, self.tiny_rows = {}, {}, None, None
        self.name = kernel16 + ":" + ",".join(f"{k}={v}" for k, v in p.items())
        self.refused = False
        self.fp32_only = self.kernel == "gemm" and (p["K"] % 32 != 0 or p.get("lda", p["K"]) % 4 != 0)
        getattr(self, "_build_" + self.kernel)()

    # -- data of the families dense_ref does not have
    def _tiny(self, shape):
        """magnitudes in [2^-30, 2^-14]: hi is an fp16 subnormal or zero"""
        return np.exp2(self.rng.uniform(-30.0, -14.0, shape)) * self.rng.choice([-1.0, 1.0], shape)

    def _edge_fill(self, x, p):
        pick = self.rng.random(x.shape) < p
        x[pick] = self.rng.choice(EDGE_VALUES, int(pick.sum()))
        return x

    def _data(self, n, width, lnorm=False, scale=1.0):
        fam, rng = self.family, self.rng
        if fam in dr.FAMILIES:
            return super()._data(n, width, lnorm, scale)
        x = rng.standard_normal((n, width)) * scale
        self.tiny_rows = np.zeros(n, bool)
        if fam in ("small", "mixed") and not lnorm:              # (in front of a LayerNorm the family is made by gamma)
            self.tiny_rows[::1 if fam == "small" else 2] = True   # small: every row, so that the floor sets the case's kappa
            t = self.tiny_rows
            x[t] = self._tiny((int(t.sum()), width))
            if fam == "mixed":
                x[t, rng.integers(0, width, int(t.sum()))] = rng.standard_normal(int(t.sum())) + 2.0
        elif fam == "edge":
            x = self._edge_fill(x, 0.25)
            x[::3] = rng.choice(EDGE_VALUES, x[::3].shape)       # rows of nothing but boundary values
            x[1::3, rng.integers(0, width)] = FP16_BIG           # one element per row at the top of the range
        elif fam == "neg":
            x = np.abs(x)
        return x.astype(F32), np.zeros(n, bool)

    def _weight(self, N, K, unscale=False):
        fam = self.family
        if fam in dr.FAMILIES:
            W = super()._weight(N, K, unscale).astype(F64)
        else:
            W = self.rng.standard_normal((N, K)) / np.sqrt(K)
            if fam in ("small", "mixed"):
                W[:, ::4] = self._tiny((N, W[:, ::4].shape[1]))   # columns of tiny weights
            elif fam == "edge":
                W = self._edge_fill(W, 0.25)
            elif fam == "neg":
                W = -np.abs(W)
        W = W.astype(F32)
        return f16(W) if self.form == "float16" else W          # `_h`: the fp16 weight values are the operands

    def _bias(self, N, feeds_relu=False, feeds_ln=False):
        if self.family in dr.FAMILIES:
            return super()._bias(N, feeds_relu, feeds_ln)
        if self.family == "neg":                                 # with x >= 0 and W <= 0: every pre-activation negative
            return (-np.abs(self.rng.standard_normal(N)) - 0.5).astype(F32)
        return None                                              # small, mixed, edge: nothing but product terms sets the scale

    def _residual_rows(self, n, N, special):
        if self.family in dr.FAMILIES:
            return super()._residual_rows(n, N, special)
        x = self.rng.standard_normal((n, N))
        if self.family in ("small", "mixed") and self.tiny_rows is not None and len(self.tiny_rows) == n:
            x[self.tiny_rows] *= 2.0 ** -24                      # the residual of a tiny row must not hide its products
        return x.astype(F32)

    def _ln_params(self, N, in_front=False):
        if in_front and self.family in ("small", "mixed"):       # LayerNorm in front of the product: outputs of ~1e-5
            g = 1e-5 * (1.0 + 0.1 * self.rng.standard_normal(N))
            if self.family == "mixed":
                g[self.rng.integers(0, N)] = 1.0
            return g.astype(F32), np.zeros(N, F32)
        return super()._ln_params(N)

    def _out2(self, name, n_rows, ld, rows, N, val, A, A32, init_rows=None, floor=None):
        self._out(name, n_rows, ld, rows, N, val, A, init_rows)
        ok = rows >= 0
        self.A32[name] = np.full((n_rows, ld), np.nan)
        self.A32[name][rows[ok], :N] = A32[ok]
        if floor is not None:
            self.floor[name] = np.full((n_rows, ld), np.nan)
            self.floor[name][rows[ok], :N] = floor[ok]

    def _rep(self, a, W):
        R, fl = rep_term(self.form, a, W)
        return U24 * R, U24 * fl

    # -- sc_gemm with SC_GEMM_SPLIT16
    def _build_gemm(self):
        p = self.p
        self._gemm_operands()                                    # buffers, tables, the float64 reference, A of the fp32 model
        self.A32["C"] = self.A["C"].copy()
        if self.fp32_only:
            return
        g = self._g
        R, fl = self._rep(g["a"], g["W"])
        ok = g["c_rows"] >= 0
        self.A["C"][g["c_rows"][ok], :p["N"]] += R[ok]
        self.floor["C"] = np.full(self.A["C"].shape, np.nan)
        self.floor["C"][g["c_rows"][ok], :p["N"]] = fl[ok]

    def _gemm16(self, mistake):
        g, p = self._g, self.p
        K = p["K"]
        a = (g["a_clamped"] if mistake == "clamped_row" else g["a"]).astype(F32)
        with np.errstate(invalid="ignore", over="ignore"):
            if K < 2560:
                hh, c = split_sum(a, g["W"], mistake)
                parts = None
            else:
                ks = -(-(K // 32) // 8) * 32
                parts = [split_sum(a[:, s:min(s + ks, K)], g["W"][:, s:min(s + ks, K)], mistake) for s in range(0, K, ks)]
            late = mistake == "fold_after_relu" and g["mode"] == "relu"
            if parts is None:
                acc, cl = (hh, c) if late else (hh + c, None)
            else:
                acc = tree8_32([h for h, _ in parts] if late else [h + cc for h, cc in parts])
                cl = tree8_32([cc for _, cc in parts]) if late else None
            if g["bias"] is not None:
                acc = acc + g["bias"]
            if g["mode"] == "relu":
                acc = np.maximum(acc, F32(0))
                if late:
                    acc = acc + cl
            if g["mode"] == "residual":
                acc = g["old"] + acc
        return acc

    # -- sc_rowtile_proj_s / _h
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
        g, b = self._ln_params(D, in_front=form == "qkv")
        self.inputs["ln_g"], self.inputs["ln_b"] = g, b
        b64 = 0.0 if bias is None else bias.astype(F64)
        g64, bt64 = g.astype(F64), b.astype(F64)
        self._r = dict(x=x, W=W, bias=bias, g=g, b=b)
        if form == "qkv":
            xn, Axn = layer_norm_ref(x.astype(F64), np.zeros((M, D)), g64, bt64, LN_EPS)
            y, Ay = linear_ref(xn, Axn, W.astype(F64), b64)
            R, fl = self._rep(xn, W)
            self._out2("C", M + 3, ldc, rows, N, y, Ay + R, Ay, floor=fl)
        else:
            old = self._residual_rows(M, D, special)
            self._r["old"] = old
            y, Ay = linear_ref(x.astype(F64), np.zeros((M, D)), W.astype(F64), b64)
            R, fl = self._rep(x, W)
            y, Ay = old + y, np.abs(old) + Ay
            self._out2("C", M + 3, ldc, rows, N, y, Ay + R, Ay, init_rows=old, floor=fl)
            self._out2("LN2", M + 3, D, rows, D, *layer_norm_ref(y, Ay + R, g64, bt64, LN_EPS),
                       layer_norm_ref(y, Ay, g64, bt64, LN_EPS)[1])

    def _rowtile16(self, mistake):
        r, form = self._r, self.p["form"]
        x = r["x"]
        if form == "qkv":
            x = layer_norm32(x, r["g"], r["b"], LN_EPS)
        if self.form == "split16":
            hh, c = split_sum(x, r["W"], mistake)
            acc = hh + c
        else:
            acc = chain32(half(x, mistake), half(r["W"], mistake))
        if r["bias"] is not None:
            acc = acc + r["bias"]
        if form == "qkv":
            return {"C": acc}
        acc = r["old"] + acc
        return {"C": acc, "LN2": layer_norm32(acc, r["g"], r["b"], LN_EPS)}

    # -- sc_ffn_ln_s / _h
    def _build_ffn(self):
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
        g, b = self._ln_params(D)
        self.inputs["ln_g"], self.inputs["ln_b"] = g, b
        self._f = dict(xn=xn, W1=W1, b1=b1, W2=W2, b2=b2, x=x, n=n, rows=rows, special=special, g=g, b=b)
        z = lambda v: 0.0 if v is None else v.astype(F64)   # noqa: E731
        W1d, W2d, xd = W1.astype(F64), W2.astype(F64), x.astype(F64)
        h, Ah = linear_ref(xn.astype(F64), np.zeros((M, D)), W1d, z(b1))
        h = np.maximum(h, 0.0)
        if self.family in ("dead", "constant", "neg"):
            assert (h[special] == 0).all() and (self.family != "neg" or (h == 0).all())   # the family is what it is called
        R1, fl1 = self._rep(xn, W1)
        R2, fl2 = self._rep(h, W2)                               # (the hidden activation's own rounding is in here)
        y, Ay32 = linear_ref(h, Ah, W2d, z(b2))
        _, Ay = linear_ref(h, Ah + R1, W2d, z(b2))
        y, Ay32, Ay = xd + y, np.abs(xd) + Ay32, np.abs(xd) + Ay + R2
        self._out2("X", n, D, rows, D, y, Ay, Ay32, init_rows=x, floor=fl1 @ np.abs(W2d).T + fl2)
        if p["ln"]:
            g64, b64 = g.astype(F64), b.astype(F64)
            self._out2("ln_out", n, D, rows, D, *layer_norm_ref(y, Ay, g64, b64, LN_EPS), layer_norm_ref(y, Ay32, g64, b64, LN_EPS)[1])
        if self.form == "float16":                               # the float64 evaluation of the form itself ("X@form")
            xh = f16(xn).astype(F64)
            hf, Ahf = linear_ref(xh, np.zeros((M, D)), W1d, z(b1))
            hf = np.maximum(hf, 0.0)
            with np.errstate(over="ignore"):
                h16 = hf.astype(F16)
                up, dn = np.nextafter(h16, F16(np.inf)).astype(F64), np.nextafter(h16, F16(-np.inf)).astype(F64)
            v = h16.astype(F64)
            ulp = np.where(np.isfinite(up), up - v, v - dn)
            with np.errstate(invalid="ignore"):
                dist = np.minimum(np.where(np.isfinite(up), (v + up) / 2 - hf, np.inf), hf - (v + dn) / 2)
            flip = np.where(dist <= 8.0 * 2.0 ** -24 * Ahf, ulp, 0.0)
            yf, Af = linear_ref(v, Ahf + U24 * flip, W2d, z(b2))
            self.form_ref = (xd + yf, np.abs(xd) + Af)

    def _ffn16(self, mistake):
        f, Fd = self._f, self.p["F"]
        split = self.form == "split16"
        late = None
        if split:
            hh, c = split_sum(f["xn"], f["W1"], mistake)
            if mistake == "fold_after_relu":
                h, late = hh, c
            else:
                h = hh + c
        else:
            h = chain32(half(f["xn"], mistake), half(f["W1"], mistake))
        if f["b1"] is not None:
            h = h + f["b1"]
        h = np.maximum(h, F32(0))
        if late is not None:
            h = h + late
        parts = []
        for c0 in range(0, Fd, 128):
            hc, wc = h[:, c0:c0 + 128], f["W2"][:, c0:c0 + 128]
            if split:
                hh, c = split_sum(hc, wc, mistake)
                parts.append(hh + c)
            else:
                parts.append(chain32(hc if mistake == "hidden_fp32_in_h" else half(hc, mistake), half(wc, mistake)))
        acc = tree8_32(parts)
        if f["b2"] is not None:
            acc = acc + f["b2"]
        return f["x"] + acc

    # -- the transcription of the whole launch in the form's arithmetic: output name -> [M][N] float32 rows in launch order
    def transcription(self, mistake=None):
        if self.fp32_only:
            return super().transcription("clamped_row" if mistake == "clamped_row" else None)
        if self.kernel == "gemm":
            return {"C": self._gemm16(mistake)}
        if self.kernel == "rowtile":
            return self._rowtile16(mistake)
        x = self._ffn16(mistake)
        out = {"X": x}
        if self.p["ln"]:
            out["ln_out"] = layer_norm32(x, self._f["g"], self._f["b"], LN_EPS)
        return out

    def transcription32(self):
        """the fp32 transcription of dense_ref on the same operands (what the spec is measured against)"""
        return super().transcription(None)

    # -- kappas
    def _swap(self, fp32):
        keep, self.A = self.A, (self.A32 if fp32 else self.A)
        return keep

    def kappas_of_rows(self, outs, fp32=False):
        keep = self._swap(fp32)
        try:
            res = super().kappas_of_rows(outs)
        finally:
            self.A = keep
        if self.form_ref is not None and not fp32:
            res["X@form"] = dr.kappa(outs["X"], *self.form_ref)
        return res

    def kappas_of_buffers(self, bufs, fp32=False):
        keep = self._swap(fp32)
        try:
            res = super().kappas_of_buffers(bufs)
        finally:
            self.A = keep
        if self.form_ref is not None and not fp32:
            res["X@form"] = dr.kappa(np.asarray(bufs["X"], F64)[self.out_rows("X")], *self.form_ref)
        return res

    def floor_share(self, outs):
        """the direct output (C / X) of a transcription: at its worst element (largest error / E), the share of E that the
        2^-36 floor contributes"""
        name = "C" if "C" in outs else "X"
        rows = self.out_rows(name)
        ok = rows >= 0
        N = outs[name].shape[1]
        E, ref, fl = (a[rows[ok], :N] for a in (self.A[name], self.ref[name], self.floor[name]))
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(E > 0, np.abs(outs[name][ok].astype(F64) - ref) / E, 0.0)
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        return float(fl[i] / E[i]), float(ratio[i] * U24)


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(Case(k, i, **p) for i, (k, p) in enumerate(case_params()))


def cases_of(kernel):
    return [c for c in all_cases() if c.kernel16 == kernel]


# ---------------------------------------------------------------------------------------------------------------------
# the launches
def tensors(case, device="cpu"):
    """name -> torch tensor of every buffer, the weights packed and split / halved exactly as PackedWeights does"""
    from speechcatcher_amd.weights import pack_panel_weight, split_panel_weight
    t = {}
    for name, a in {**case.inputs, **case.tables, **case.init}.items():
        v = torch.from_numpy(np.array(a))
        if case.kernel in ("ffn", "rowtile") and name in ("W", "W1", "W2"):
            v = pack_panel_weight(v)
            v = split_panel_weight(v) if case.form == "split16" else v.to(torch.float16).contiguous()
        t[name] = v.to(device)
    return t


def launch(hip, case, t):
    """the launch of the form on a HipBackend"""
    p, k, g = case.p, case.kernel, t.get
    s = case.form == "split16"
    if k == "gemm":
        conv = p.get("conv")
        hip.gemm(t["A"], g("a_rows"), p.get("lda", p["K"]), t["W"], g("bias"), t["C"], g("c_rows"), p.get("ldc", p["N"]), p["M"],
                 p["N"], p["K"], relu=p["mode"] == "relu", conv_f1=conv[0] if conv else 0, residual=p["mode"] == "residual",
                 split16=True)
    elif k == "rowtile":
        fn = hip.rowtile_proj_s if s else hip.rowtile_proj_h
        if p["form"] == "qkv":
            fn(t["A"], p["M"], p["D"], t["W"], g("bias"), p["N"], t["C"], ln_g=t["ln_g"], ln_b=t["ln_b"], eps=LN_EPS)
        else:
            fn(t["A"], p["M"], p["D"], t["W"], g("bias"), p["N"], t["C"], R=t["C"], g2=t["ln_g"], b2=t["ln_b"], LN2=t["LN2"],
               eps=LN_EPS)
    else:
        fn = hip.ffn_ln_s if s else hip.ffn_ln_h
        fn(t["XN"], g("rows"), p["M"], p["D"], p["F"], t["W1"], g("b1"), t["W2"], g("b2"), t["X"], t["ln_g"], t["ln_b"],
           g("ln_out"), eps=LN_EPS)


def outputs(case, t):
    return {name: t[name].detach().cpu().numpy() for name in case.ref}


def spec_kappas(case):
    """the kappa the fp32 torch spec (on the unsplit fp32 weights) needs on the fp32 model, per output"""
    from oracle.kernel_spec import SpecBackend
    t = dr.tensors(case)
    dr.launch(SpecBackend(), case, t)
    return case.kappas_of_buffers(dr.outputs(case, t), fp32=True)


@functools.lru_cache(maxsize=None)
def _kappa_ref(i):
    case = all_cases()[i]
    return case.kappas_of_rows(case.transcription())


def kappa_ref(case):
    """output name -> kappa_ref, the kappa the transcription of the form needs; measured once per process"""
    return _kappa_ref(all_cases().index(case))

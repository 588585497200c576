"""Cases and float64 references for the decoder attention: the stand-alone kernels (sc_dec_self_attn / sc_dec_cross_attn) and
the fused layer launches (sc_dec_layer_self / _cross / _stream).  numpy float64 throughout, no GPU, and none of the arithmetic
of oracle/kernel_spec.py: tests/test_dec_attn_ref_spec.py holds these references to the torch spec on the CPU,
tests/test_gpu_decoder_attention.py holds the HIP kernels to them.

A CASE is one launch over S = 8 streams that differ in L, T, nh, ancestry and score pattern.  It is written identically into a
CPU batch (SpecBackend) and a GPU batch (HipBackend) with the same seeded weights: ctrl, yseq, anc, skv, ckv and either
dqkv / dq (stand-alone) or xin / ph1 / ffn_part (fused).  Score patterns are imposed through the CACHE CONTENTS: the cached K
rows are plain inputs, so they are solved from the case's own q (least-norm solution of q . k / sqrt(dk) = wanted score over
the hypotheses that attend to the row).  Everything the operation must not read is NaN, everything it must not write a sentinel.

ERROR MODEL.  Every reference value y comes with A(y), the sum of the absolute values of the terms a rounding error of its
computation is proportional to; a result has kappa = max |result - y| / (2^-24 A).  For a context element this is
    A = (1 + max over attended keys of sum_j |q_j k_j| / sqrt(dk)) . sum_i p_i |v_ic|
(one rounding per score term moves a score by 2^-24 sum|q k|, and a score error e moves p by the factor exp(e)).  The fused
launches carry A through residual and partial sums, LayerNorm and the projections, use the same context formula on the q, k, v
they project, and carry (A + |ctx|) through |Wo| - what tests/test_gpu_ops.py::test_ffn_fused_split_weights does for the
feed-forward.  The error of the projected q is NOT carried into the scores: as a sum of absolute values through the LayerNorm
and 256-term products it is ~50 times what any fp32 evaluation shows (kv_new, the same projection, needs kappa 0.05 - 0.4), and
amplified by max|k| it left the partial products a kappa of 1e-4 - 1e-2, where a wrong reference could hide; it is part of kappa.
The constant kappa is NOT chosen here: the CPU test measures the kappa that the fp32 torch spec needs per family and output
(kappa_ref), and the GPU test allows a kernel 4 x kappa_ref.

FP16 DECODER MODE (Case(dec_half = sc_search.act_half: 1, 2 or 3; kinds "self" and "cross"; fp16 K|V caches).  Where the
kernel (csrc/decoder_layer.hip: dec_layer_attn_kernel<.., WH>) rounds, and what E gains (r(a) = max(2^-11 |a|, 2^-25)):
  bit 1  the *_pph weights are fp16 numbers (the reference takes them as given); the LayerNorm row is rounded to fp16 on its way
         from LDS into the projection's MFMA, the context on its way into the output projection: sum |w| r(a) per product sum.
         The error dq of the projected q that comes from THIS rounding (not its fp32 part, see above) is carried into the
         scores: with Ds = max over the attended keys of sum_j (dq_j |k_j| + |q_j| dk_j) / sqrt(dk) (dk: the new token's own
         key only, cached rows are inputs) every p moves by a factor within exp(+-2 Ds), so a context element gains
         expm1(2 Ds) sum_i p_i |v_ic| + p_own dv_c.  q, the scores, the softmax and all accumulators stay fp32;
  bit 2  ph1 / ph2 / ffn_part hold fp16 elements in the first half of their buffers: what the launch reads is taken as given
         (the cases write fp16 numbers); a stored partial product is rounded once, at the store, AFTER the sum over the heads
         of a workgroup (one head, or four): r(p) per stored partial.
SpecBackend has no such mode: kappa_ref of these cases is the kappa a numpy TRANSCRIPTION of this arithmetic needs (fp32
k-ordered chains over the rounded operands, an fp32 softmax, the head partials summed per workgroup and rounded at the store).
The cases are a reduced set: families flat and dominant, cached lengths 16, 17, 128, 129, cross T 16, 17, 129."""
import dataclasses
import functools
import math

import numpy as np
import torch

EPS = 2.0 ** -24
SENTINEL = -77.25                    # in every buffer the launch must not write (exact in fp32 and fp16)
S, INACTIVE = 8, 2                   # streams per launch; the stream with ctrl active = 0
LIVE = [s for s in range(S) if s != INACTIVE]
LCAP, TCAP = 530, 920
SELF_LC = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 513)      # cached positions L - 1
CROSS_T = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 904, TCAP)
FAMILIES = ("flat", "dominant", "ascending", "descending", "offset", "multipeak")
MARGIN = 45.0                        # dominant key: >= 40 over the rest after the +-1.5 of jitter on either side
# the dominant family: where the key lies, and lengths at which that place exists (key index = position with a shared history;
# tiles of 16 keys go to the waves round-robin, a wave's second canonical batch starts at tile 8 = key 128)
DOMINANT = (("first", 65, 128), ("last", 127, 129), ("wave1", 128, 63), ("wave2", 129, 64), ("wave3", 511, 65),
            ("batch2", 512, 904), ("own", 513, TCAP))
PLACE = {"first": 0, "wave1": 16 + 5, "wave2": 32 + 5, "wave3": 48 + 5, "batch2": 128 + 3}

GEOMS = {"TINY": 16, "XL": 32, "L_LIKE": 64}     # name -> head dim


def cfg_name(geom):
    """registers the geometry's model in test_engine_spec.CFGS: the dims of config.TINY / XL / L_LIKE (d_model, heads) with
    two decoder layers and one encoder layer - the launches here address one layer and check that the other stays untouched"""
    import test_engine_spec
    from speechcatcher_amd import config
    if geom == "TINY":
        return "TINY"
    name = "DECATT_" + geom
    test_engine_spec.CFGS.setdefault(name, dataclasses.replace(getattr(config, geom), enc_layers=1, dec_layers=2))
    return name


def kv_pool_rows(W):
    """fully divergent histories of 129 positions, or three lineages over 513: the most distinct rows a case names"""
    return max(130 * W, 16 + 3 * 513 + 2 * W) + 64


def batch_kwargs(W):
    return dict(n_streams=S, max_frames=TCAP, max_tokens=LCAP, pcm_capacity=1 << 12, kv_pool_rows=kv_pool_rows(W))


def f16(a):
    """fp16 storage: rounding, not arithmetic"""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# streams of a launch
@dataclasses.dataclass
class Stream:
    s: int
    active: int
    cur: int
    T: int
    L: int
    nh: int
    anc_kind: str = ""
    fork: int = -1
    variant: str = ""
    anc: np.ndarray = None           # [L][nh] pool rows
    keys: list = None                # self: walk order - (position, tuple of hypotheses, pool row)


def stream_plan(family, W):
    """L, T, nh, ancestry and variant of the 8 streams of a family's launch.  Over the six families every length of SELF_LC and
    CROSS_T occurs three times; nh is W, 1, 3 (1 < nh < W), W - 1, 2; cur alternates."""
    f = FAMILIES.index(family)
    nhs = [W, 1, 3, W, max(W - 1, 1), 2, W]
    out = []
    for i, s in enumerate(LIVE):
        q = 7 * f + i
        if family == "dominant":
            variant, Lc, T = DOMINANT[i]
        else:
            variant, Lc, T = ("plus", "minus")[i % 2] if family == "offset" else "", SELF_LC[q % 14], CROSS_T[q % 12]
        kind = ("shared", "fork", "divergent")[(f + i) % 3]
        if kind == "divergent" and Lc > 129:
            kind = "fork"            # (the pool has no room for 513 x nh rows)
        fork = -1
        if kind == "fork":           # the 512 edge, inside a tile, on a tile edge, near the start
            fork = 512 if Lc > 512 else (max(Lc - 3, 0), (Lc // 16) * 16 if Lc >= 16 else Lc // 2, min(5, Lc))[(q // 3) % 3]
        out.append(Stream(s, 1, i % 2, T, Lc + 1, nhs[i], kind, fork, variant))
    out.insert(INACTIVE, Stream(INACTIVE, 0, 0, 100, 40, W))
    return out


HALF_LC, HALF_T = (16, 17, 128, 129), (16, 17, 129)
HALF_FAMILIES = ("flat", "dominant")
HALF_DOMINANT = ("first", "last", "wave1", "wave2", "own", "last", "wave3")      # by live stream; wave1.. only where they exist


def half_stream_plan(family, W):
    """the reduced set of the fp16 decoder mode: L - 1 over HALF_LC, T over HALF_T, the nh and ancestries of stream_plan"""
    f = FAMILIES.index(family)
    nhs = [W, 1, 3, W, max(W - 1, 1), 2, W]
    out = []
    for i, s in enumerate(LIVE):
        Lc, T = HALF_LC[(i + f) % 4], HALF_T[(i + 2 * f) % 3]
        variant = ""
        if family == "dominant":
            variant = HALF_DOMINANT[i]
            if PLACE.get(variant, 0) >= min(Lc, T):
                variant = "last"
        kind = ("shared", "fork", "divergent")[(f + i) % 3]
        fork = (max(Lc - 3, 0), (Lc // 16) * 16, min(5, Lc))[i % 3] if kind == "fork" else -1
        out.append(Stream(s, 1, i % 2, T, Lc + 1, nhs[i], kind, fork, variant))
    out.insert(INACTIVE, Stream(INACTIVE, 0, 0, 100, 40, W))
    return out


def _r16(x):
    """r(x) = max(2^-11 |x|, 2^-25), r(0) = 0: the rounding of a value to fp16"""
    x = np.abs(x)
    return np.where(x == 0, 0.0, np.maximum(2.0 ** -11 * x, 2.0 ** -25))


def build_ancestry(st, kv_rows, rng):
    """a valid ancestor table: hypotheses that share a row at a position share all earlier ones; the rows of the new token
    (position L - 1) are distinct.  Pool rows are drawn at random; streams with an even index never name row 0."""
    Lc, nh = st.L - 1, st.nh
    lin = np.zeros((st.L, nh), np.int64)                       # lineage of hypothesis h at position p
    if st.anc_kind == "divergent":
        lin[:] = np.arange(nh)
    elif st.anc_kind == "fork":
        lin[st.fork:] = np.arange(nh) % 3
        lin[max(st.fork, Lc - 2):] = np.arange(nh)
    lin[Lc] = np.arange(nh)
    pool = rng.permutation(np.arange(1 if st.s % 2 == 0 else 0, kv_rows))
    st.anc = np.zeros((st.L, nh), np.int64)
    st.keys, n = [], 0
    for p in range(st.L):
        ids = list(dict.fromkeys(lin[p].tolist()))             # first-occurrence order = the order of the kernels' row list
        for lid in ids:
            hyps = tuple(np.nonzero(lin[p] == lid)[0].tolist())
            st.anc[p, list(hyps)] = pool[n]
            if p < Lc:
                st.keys.append((p, hyps, int(pool[n])))
            n += 1
    assert n < kv_rows - 1, (n, kv_rows)
    return int(pool[n])                                        # a row nobody names (for the table's unused entries)


# ---------------------------------------------------------------------------------------------------------------------
# score patterns
def pattern(family, variant, nh, n, own=False):
    """wanted score of hypothesis h at key position p, [nh][n] (None: flat - random keys as they come).  With own = True the
    scores are relative to the score of the new token's own row."""
    if family == "flat" or n == 0:
        return None
    pos = np.arange(n, dtype=np.float64)
    t = np.zeros((nh, n))
    if family == "dominant":
        if variant == "own" and own:
            t[:] = -MARGIN
        else:
            at = {"last": n - 1, "own": max(n - 17, 0)}.get(variant, PLACE.get(variant, 0))
            t[:, min(at, n - 1)] = MARGIN
        if nh > 2:
            t[nh - 1] = 0.0          # one flat hypothesis beside the peaked ones: the maximum is per hypothesis, not per tile
    elif family == "ascending":
        t[:] = 0.25 * pos            # the running maximum moves in every batch
    elif family == "descending":
        t[:] = -0.25 * pos
    elif family == "offset":
        t[:] = 100.0 if variant == "plus" else -100.0          # exp overflows / 0/0 without the maximum subtracted
    elif family == "multipeak":      # every hypothesis its own key of ONE tile; margin 8 keeps the other keys in the sum
        p0 = 16 * ((n // 2) // 16)
        if p0 + nh > n:
            p0 = max(0, n - nh)
        for h in range(nh):
            t[h, (p0 + h) % n if p0 + h >= n else p0 + h] = 8.0
    return t


def solve_keys(q, groups, want, dk, rng):
    """K rows [n][H][dk] with q[h] . k / sqrt(dk) = want[h][head][key] for the hypotheses h of the key's group (least norm),
    plus a little noise.  q [nh][H][dk]; groups: (tuple of hypotheses, key indices)."""
    H = q.shape[1]
    K = np.zeros((want.shape[2], H, dk))
    for hyps, idx in groups:
        Q = q[list(hyps)].transpose(1, 0, 2) / math.sqrt(dk)   # [H][m][dk]
        P = np.linalg.pinv(Q)                                  # [H][dk][m]
        K[idx] = np.einsum("hdm,mhk->khd", P, want[list(hyps)][:, :, idx])
    return K + 0.02 * rng.standard_normal(K.shape)


def wanted(pat, nh, H, base, rng):
    """pattern + the score of the own row (base [nh][H] or 0) + jitter per head"""
    n = pat.shape[1]
    w = pat[:, None, :] + 0.3 * np.clip(rng.standard_normal((nh, H, n)), -5, 5)
    return w + (base[:, :, None] if base is not None else 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# float64 building blocks: value and A (see the module docstring)
def layer_norm_ref(x, Ax, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    xc = x - mu
    var = (xc * xc).mean(-1, keepdims=True) + eps
    sd = np.sqrt(var)
    xn = xc / sd * g + b
    Axc = Ax + Ax.mean(-1, keepdims=True) + np.abs(x) + np.abs(x).mean(-1, keepdims=True)
    rel = (np.abs(xc) * Axc).mean(-1, keepdims=True) / var + 2.0          # relative error of 1 / sd
    return xn, np.abs(g) * (Axc + np.abs(xc) * rel) / sd + np.abs(xn)


def linear_ref(x, Ax, W, b):
    return x @ W.T + b, (Ax + np.abs(x)) @ np.abs(W).T + np.abs(b)


def attention_ref(q, K, V, dk):
    """q [nh][H][dk]; K, V [nh][n][H][dk]: the n keys hypothesis h attends to.  Returns ctx, A [nh][H*dk]."""
    s = np.einsum("hgd,hngd->hgn", q, K) / math.sqrt(dk)
    sabs = np.einsum("hgd,hngd->hgn", np.abs(q), np.abs(K)) / math.sqrt(dk)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ctx = np.einsum("hgn,hngd->hgd", p, V)
    A = (1.0 + sabs.max(-1))[:, :, None] * np.einsum("hgn,hngd->hgd", p, np.abs(V))
    nh = q.shape[0]
    return ctx.reshape(nh, -1), A.reshape(nh, -1)


def head_partials_ref(ctx, Actx, Wo, H, hpw):
    """ph[w][g] = sum over the heads of group g of ctx[w][head] . Wo[:, head]^T"""
    nh, d = ctx.shape
    dk = d // H
    ph, A = np.zeros((nh, H // hpw, d)), np.zeros((nh, H // hpw, d))
    for h in range(H):
        c = slice(h * dk, (h + 1) * dk)
        ph[:, h // hpw] += ctx[:, c] @ Wo[:, c].T
        A[:, h // hpw] += (Actx[:, c] + np.abs(ctx[:, c])) @ np.abs(Wo[:, c]).T
    return ph, A


def kappa(got, ref, A):
    """the kappa a result needs; inf if it is not finite"""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    if got.size == 0:
        return 0.0
    return float((np.abs(got - ref) / (EPS * A)).max())


# ---------------------------------------------------------------------------------------------------------------------
def _weights(sb):
    """the model's fp32 weights as float64 arrays (cached on the batch)"""
    w = getattr(sb, "_decatt_w64", None)
    if w is None:
        n = lambda t: t.detach().cpu().double().numpy()   # noqa: E731
        names = ("ln1_g", "ln1_b", "wqkv", "bqkv", "wo", "bo", "ln2_g", "ln2_b", "wq", "bq", "wo2", "bo2", "ln3_g", "ln3_b", "b2")
        w = {"embed": n(sb.w.embed), "pe": n(sb.w.pe[:LCAP + 1]), "dec": [{k: n(lw[k]) for k in names} for lw in sb.w.dec]}
        sb._decatt_w64 = w
    return w


class Case:
    """One launch: inputs (fp32 tensors shaped like the batch's buffers), the float64 reference of every output with its A,
    and what must stay as it was.  kind: "attn" (stand-alone self + cross on one set of buffers), "self", "cross", "stream"."""

    def __init__(self, geom, W, kind, family, half=False, li=1, npart=1, hpw=1, seed=0, dec_half=0):
        sc = spec_batch(geom, W)
        cfg = sc.cfg
        self.geom, self.kind, self.family, self.half, self.li, self.npart, self.hpw = geom, kind, family, half, li, npart, hpw
        # fp16 decoder mode (sc_search.act_half): bit 1 fp16 projection weights / MFMA inputs, bit 2 fp16 partial products
        assert not dec_half or (half and kind in ("self", "cross") and dec_half in (1, 2, 3))
        self.dec_half, self.wh, self.part_half, self._t = dec_half, bool(dec_half & 1), bool(dec_half & 2), {}
        self.W, self.d, self.H = sc.W, cfg.d_model, cfg.dec_heads
        self.dk, self.nl, self.kv_rows = self.d // self.H, cfg.dec_layers, int(sc.kv_rows)
        self.eps, self.V = cfg.ln_eps, cfg.vocab_size
        self.w = _weights(sc)
        if self.wh:                      # the *_pph copies: fp16 numbers, the operands of the form
            self.w = dict(self.w, dec=[dict(lw, **{k: f16(lw[k]).astype(np.float64) for k in ("wqkv", "wq", "wo", "wo2")})
                                       for lw in self.w["dec"]])
        rng = self.rng = np.random.default_rng([seed, FAMILIES.index(family), self.W, self.dk, int(half), li, npart] +
                                               ([dec_half] if dec_half else []))
        W, d, n = self.W, self.d, S * self.W
        self.streams = half_stream_plan(family, W) if dec_half else stream_plan(family, W)
        f32 = np.float32
        nan = lambda *shape: np.full(shape, np.nan, f32)   # noqa: E731
        self.ctrl = np.array([[st.active, st.cur, 0, st.T, st.L, st.nh, 0, 0] for st in self.streams], np.int32)
        self.yseq = np.zeros((2, S, W, LCAP), np.int32)
        self.anc = np.zeros((2, S, LCAP, W), np.int32)
        self.skv = nan(S, self.nl, self.kv_rows, 2 * d)
        self.ckv = nan(S, self.nl, TCAP, 2 * d)
        self.inputs = {}                 # buffer name -> array; the caches, ctrl, yseq and anc are written besides
        self.ref, self.A = {}, {}        # output name -> {stream: array of the live rows}
        if kind == "attn":
            self.inputs["dqkv"], self.inputs["dq"] = nan(n, 3 * d), nan(n, d)
        else:
            self.inputs["dx"] = nan(n, d)
            if kind == "cross":
                self.inputs["ph1"] = nan(n, self.H, d)
            else:
                self.inputs["ffn_part"] = nan(sc.ffn_part.shape[0], n, d)
        for st in self.streams:
            if st.active:
                self._build_stream(st)
            else:                        # the inactive stream: a table that would be valid, everything else stays NaN
                self.anc[:, st.s] = 1
        self.new_rows = {st.s: st.anc[st.L - 1].copy() for st in self.streams if st.active}

    # -- inputs of one live stream and its references
    def _keep(self, st, name, val, A):
        self.ref.setdefault(name, {})[st.s] = val
        self.A.setdefault(name, {})[st.s] = A

    def _r32(self, *shape, scale=1.0):
        return (scale * self.rng.standard_normal(shape)).astype(np.float32)

    def _queries(self, nh):
        """stand-alone kernels, where q is an input: per head, rows of a random orthogonal matrix at the length of a normal
        vector (x 0.7 .. 1.3) - the keys are solved from q, and nh = dk = 16 normal rows can be nearly dependent (keys of 1e5,
        beyond fp16)"""
        H, dk = self.H, self.dk
        q = np.empty((nh, H, dk))
        for g in range(H):
            q[:, g] = np.linalg.qr(self.rng.standard_normal((dk, dk)))[0][:nh]
        return (q * math.sqrt(dk) * self.rng.uniform(0.7, 1.3, (nh, H, 1))).reshape(nh, -1).astype(np.float32)

    def _rows(self, st):
        return slice(st.s * self.W, (st.s + 1) * self.W)

    def _build_stream(self, st):
        d, nh, lw = self.d, st.nh, self.w["dec"][self.li]
        dead = build_ancestry(st, self.kv_rows, self.rng)
        self.anc[:, st.s] = dead
        self.anc[st.cur, st.s, :st.L, :nh] = st.anc
        self.yseq[st.cur, st.s, :nh, :st.L] = self.rng.integers(1, self.V - 1, (nh, st.L))
        if self.kind == "attn":          # q | k | v and q are inputs
            qkv = self._r32(nh, 3 * d)
            qkv[:, d:2 * d] *= 0.3
            qkv[:, :d] = self._queries(nh)
            ctx, _ = self._self_attention(st, qkv, None)
            self.inputs["dqkv"][self._rows(st)][:nh] = qkv
            qc = self._queries(nh)
            self.inputs["dq"][self._rows(st)][:nh] = qc
            self._cross_attention(st, qc)
            return
        x, Ax = self._prologue(st)
        if self.kind == "cross":
            self._keep(st, "xout", x, Ax)
            xn, Axn = layer_norm_ref(x, Ax, lw["ln2_g"], lw["ln2_b"], self.eps)
            qc, _, Dq = self._proj(xn[:nh], Axn[:nh], lw["wq"], lw["bq"])
            ctx2, Actx2 = self._cross_attention(st, qc, Dq)
            self._keep(st, "ph2", *self._head_partials(ctx2, Actx2, lw["wo2"]))
            return
        xn, Axn = layer_norm_ref(x, Ax, lw["ln1_g"], lw["ln1_b"], self.eps)
        qkv, Aqkv, Dqkv = self._proj(xn[:nh], Axn[:nh], lw["wqkv"], lw["bqkv"])
        ctx, Actx = self._self_attention(st, qkv, Aqkv, Dqkv)
        if self.kind == "self":
            self._keep(st, "xout", x, Ax)
            self._keep(st, "ph1", *self._head_partials(ctx, Actx, lw["wo"]))
            return
        # stream-resident form: residual of the self-attention block, norm2, q, cross-attention, residual, norm3
        x1, Ax1 = self._residual(x, Ax, ctx, Actx, lw["wo"], lw["bo"], nh)
        xn2, Axn2 = layer_norm_ref(x1, Ax1, lw["ln2_g"], lw["ln2_b"], self.eps)
        ctx2, Actx2 = self._cross_attention(st, linear_ref(xn2[:nh], Axn2[:nh], lw["wq"], lw["bq"])[0])
        x2, Ax2 = self._residual(x1, Ax1, ctx2, Actx2, lw["wo2"], lw["bo2"], nh)
        self._keep(st, "xout", x2, Ax2)
        self._keep(st, "xn_out", *layer_norm_ref(x2, Ax2, lw["ln3_g"], lw["ln3_b"], self.eps))

    def _proj(self, xn, Axn, W, b):
        """LayerNorm rows . W^T + b -> (y, A, D); fp16 decoder mode: D = sum |w| r(xn), the rounding of the rows on their way
        into the MFMA (in the units of y; also part of A), else None"""
        y, A = linear_ref(xn, Axn, W, b)
        if not self.wh:
            return y, A, None
        D = _r16(xn) @ np.abs(W).T
        return y, A + D / EPS, D

    def _head_partials(self, ctx, Actx, Wo):
        """head_partials_ref + the fp16 mode's terms: the context rounded on its way into the output projection (bit 1), the
        partial product of a workgroup's heads rounded once at the store (bit 2)"""
        ph, A = head_partials_ref(ctx, Actx, Wo, self.H, self.hpw)
        if self.wh:
            for h in range(self.H):
                c = slice(h * self.dk, (h + 1) * self.dk)
                A[:, h // self.hpw] += _r16(ctx[:, c]) @ np.abs(Wo[:, c]).T / EPS
        if self.part_half:
            A = A + _r16(ph) / EPS
        return ph, A

    def _score_terms(self, q, K, V, Dq, dk, Dk_own=None, Dv_own=None):
        """fp16 decoder mode: what a context element gains from the rounding error of the projected q (and of the new token's
        own k, v), in units of 2^-24 (see the module docstring); q [nh][H][dk], K, V [nh][n][H][dk], own row last"""
        s = np.einsum("hgd,hngd->hgn", q, K) / math.sqrt(dk)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        ds = np.einsum("hgd,hngd->hgn", Dq, np.abs(K)) / math.sqrt(dk)
        if Dk_own is not None:
            ds[..., -1] += np.einsum("hgd,hgd->hg", np.abs(q), Dk_own) / math.sqrt(dk)
        extra = np.expm1(2.0 * ds.max(-1))[:, :, None] * np.einsum("hgn,hngd->hgd", p, np.abs(V))
        if Dv_own is not None:
            extra = extra + p[..., -1][:, :, None] * Dv_own
        return extra.reshape(q.shape[0], -1) / EPS

    @staticmethod
    def _residual(x, Ax, ctx, Actx, Wo, bo, nh):
        """x + (ctx . Wo^T + bo); rows >= nh have no context: x + bo"""
        y, Ay = linear_ref(ctx, Actx, Wo, bo)
        x1, Ax1 = x + bo, Ax + np.abs(x) + np.abs(bo)
        x1[:nh] = x[:nh] + y
        Ax1[:nh] += Ay
        return x1, Ax1

    def _prologue(self, st):
        """x of all W rows: embedding + PE (layer 0 of the self / stream forms), else xin + (partial sums + bias)"""
        W, d, H, li, w = self.W, self.d, self.H, self.li, self.w
        rows = self._rows(st)
        if self.kind != "cross" and li == 0:
            tok = self.yseq[st.cur, st.s, np.minimum(np.arange(W), st.nh - 1), st.L - 1]
            e, pe = w["embed"][tok], w["pe"][st.L - 1]
            self._t[st.s] = dict(x=(e * math.sqrt(d) + pe).astype(np.float32))
            return e * math.sqrt(d) + pe, np.abs(e) * math.sqrt(d) + np.abs(pe)
        xin = self._r32(W, d, scale=2.0)
        self.inputs["dx"][rows] = xin
        if self.kind == "cross":         # per-head partial products of the self-attention's output projection
            nph = H // self.hpw
            part = self._r32(W, nph, d, scale=0.5)
            if self.part_half:
                part = f16(part)
            self.inputs["ph1"].reshape(-1)[:S * W * nph * d].reshape(S * W, nph, d)[rows] = part
            part, bias = part.transpose(1, 0, 2), w["dec"][li]["bo"]
        else:                            # split sums of the previous layer's feed-forward
            part = self._r32(self.npart, W, d, scale=0.5)
            if self.part_half:
                part = f16(part)
            self.inputs["ffn_part"][:self.npart, rows] = part
            bias = w["dec"][li - 1]["b2"]
        self._t[st.s] = dict(xin=xin, part=part.copy(), bias=bias)
        part = part.astype(np.float64)
        return xin + (part.sum(0) + bias), np.abs(xin) + np.abs(part).sum(0) + np.abs(bias)

    def _store_cache(self, K, Vshape):
        """K [n][H][dk] and random V of varying size -> fp32 (or fp16-rounded) K|V rows [n][2d]"""
        n = K.shape[0]
        V = self.rng.standard_normal(Vshape) * self.rng.uniform(0.2, 3.0, (n, 1, 1))
        kv = np.concatenate([K.reshape(n, self.d), V.reshape(n, self.d)], 1).astype(np.float32)
        if self.half:
            kv = f16(kv)
        assert np.isfinite(kv).all()
        return kv

    def _self_attention(self, st, qkv, Aqkv, Dqkv=None):
        """cached rows through the ancestor table + the new token's own row.  qkv [nh][3d] (float32 inputs or the float64
        projection, Aqkv its A); writes the cached rows into skv; keeps kv_new (and self_ctx, stand-alone)"""
        rng, d, H, dk, li = self.rng, self.d, self.H, self.dk, self.li
        nh, Lc = st.nh, st.L - 1
        q, kn, vn = (np.asarray(qkv[:, i * d:(i + 1) * d], np.float64).reshape(nh, H, dk) for i in range(3))
        pat = pattern(self.family, st.variant, nh, Lc, own=True)
        base = np.einsum("hgd,hgd->hg", q, kn) / math.sqrt(dk)
        if self.kind == "attn" and self.family == "offset":      # the own row is an input here: it takes the offset too
            off = (100.0 if st.variant == "plus" else -100.0) + 0.3 * rng.standard_normal((nh, H))
            kn = (off * math.sqrt(dk) / (q * q).sum(-1))[:, :, None] * q
            kn = kn.astype(np.float32).astype(np.float64)
            qkv[:, d:2 * d] = kn.reshape(nh, d)
            base = None
        nk = len(st.keys)
        if pat is None:
            K = 0.3 * rng.standard_normal((nk, H, dk))
        else:
            want = wanted(pat, nh, H, base, rng)[:, :, [p for p, _, _ in st.keys]]
            groups = {}
            for i, (_, hyps, _) in enumerate(st.keys):
                groups.setdefault(hyps, []).append(i)
            K = solve_keys(q, list(groups.items()), want, dk, rng)
        self.skv[st.s, li, [r for _, _, r in st.keys]] = self._store_cache(K, (nk, H, dk))
        # gather per hypothesis: positions 0 .. L-2 from the pool, L-1 = the own row (read before it is stored)
        kv = self.skv[st.s, li].astype(np.float64)[st.anc[:Lc]]      # [Lc][nh][2d]
        Kh = np.concatenate([kv[:, :, :d].transpose(1, 0, 2).reshape(nh, Lc, H, dk), kn[:, None]], 1)
        Vh = np.concatenate([kv[:, :, d:].transpose(1, 0, 2).reshape(nh, Lc, H, dk), vn[:, None]], 1)
        ctx, Actx = attention_ref(q, Kh, Vh, dk)
        if Dqkv is not None:
            Dq, Dk, Dv = (Dqkv[:, i * d:(i + 1) * d].reshape(nh, H, dk) for i in range(3))
            Actx = Actx + self._score_terms(q, Kh, Vh, Dq, dk, Dk, Dv)
        knv = np.concatenate([kn.reshape(nh, d), vn.reshape(nh, d)], 1)
        self._keep(st, "kv_new", knv, np.abs(knv) if Aqkv is None else Aqkv[:, d:])
        if self.kind == "attn":
            self._keep(st, "self_ctx", ctx, Actx)
        return ctx, Actx

    def _cross_attention(self, st, qc, Dq=None):
        """the T frames of the stream, shared by its hypotheses; qc [nh][d]; writes ckv; keeps cross_ctx (stand-alone)"""
        rng, d, H, dk, nh, T = self.rng, self.d, self.H, self.dk, st.nh, st.T
        qx = np.asarray(qc, np.float64).reshape(nh, H, dk)
        pat = pattern(self.family, st.variant, nh, T)
        if pat is None:
            K = 0.3 * rng.standard_normal((T, H, dk))
        else:
            K = solve_keys(qx, [(tuple(range(nh)), np.arange(T))], wanted(pat, nh, H, None, rng), dk, rng)
        kvx = self._store_cache(K, (T, H, dk))
        self.ckv[st.s, self.li, :T] = kvx
        kv = kvx.astype(np.float64)
        Kx = np.broadcast_to(kv[None, :, :d].reshape(1, T, H, dk), (nh, T, H, dk))
        Vx = np.broadcast_to(kv[None, :, d:].reshape(1, T, H, dk), (nh, T, H, dk))
        ctx, Actx = attention_ref(qx, Kx, Vx, dk)
        if Dq is not None:
            Actx = Actx + self._score_terms(qx, Kx, Vx, Dq.reshape(nh, H, dk), dk)
        if self.kind == "attn":
            self._keep(st, "cross_ctx", ctx, Actx)
        return ctx, Actx

    # -- writing a case into a batch
    def apply(self, sb):
        dev = sb.ctrl.device
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        sb.ctrl.copy_(t(self.ctrl))
        sb.yseq.copy_(t(self.yseq))
        sb.anc.copy_(t(self.anc))
        sb.skv.copy_(t(self.skv.reshape(-1, 2 * self.d)).to(sb.skv.dtype))
        sb.ckv.copy_(t(self.ckv.reshape(-1, 2 * self.d)).to(sb.ckv.dtype))
        for name, a in self.inputs.items():
            if self.part_half and name in ("ph1", "ffn_part"):     # fp16 elements at the same element offsets; the rest NaN
                h = np.full(2 * a.size, np.nan, np.float16)
                h[:a.size] = a.reshape(-1).astype(np.float16)
                a = h.view(np.float32).reshape(a.shape)
            getattr(sb, name).copy_(t(a))
        for name in self.outputs():
            self._elems(sb, name).fill_(SENTINEL)

    def _elems(self, sb, name):
        """a buffer as the flat array of its ELEMENTS: fp16 ones for the partial products of the fp16 decoder mode"""
        buf = getattr(sb, name).view(-1)
        return buf.view(torch.float16) if self.part_half and name in ("ph1", "ph2") else buf

    def outputs(self):
        """buffers the launch writes (besides the K|V append): all start as the sentinel"""
        return {"attn": ("datt",), "self": ("dxn", "ph1"), "cross": ("dxn", "ph2"), "stream": ("dxn", "dq")}[self.kind]

    # -- reading results: name -> {stream: rows of the live hypotheses (xout / xn_out: all W rows)}
    def collect(self, sb, name):
        W, d, H = self.W, self.d, self.H
        out = {}
        for st in self.streams:
            if not st.active:
                continue
            rows = slice(st.s * W, (st.s + 1) * W)
            if name in ("self_ctx", "cross_ctx"):
                out[st.s] = sb.datt[rows][:st.nh].cpu().double().numpy()
            elif name in ("xout", "xn_out"):
                out[st.s] = (sb.dxn if name == "xout" else sb.dq)[rows].cpu().double().numpy()
            elif name in ("ph1", "ph2"):
                nph = H // self.hpw
                buf = self._elems(sb, name)[:S * W * nph * d].view(S * W, nph, d)
                out[st.s] = buf[rows][:st.nh].cpu().double().numpy()
            elif name == "kv_new":
                pool = sb.skv.view(S, self.nl, self.kv_rows, 2 * d)[st.s, self.li]
                out[st.s] = pool[torch.from_numpy(self.new_rows[st.s]).to(pool.device)].cpu().double().numpy()
        return out

    def kappas(self, sb, names):
        """kappa of each named output over all live streams"""
        res = {}
        for name in names:
            got = self.collect(sb, name)
            res[name] = max(kappa(got[s], self.ref[name][s], self.A[name][s]) for s in got)
        return res

    def result_names(self, which=None):
        return {"attn": ("self_ctx", "cross_ctx") if which is None else (which + "_ctx",), "self": ("xout", "ph1", "kv_new"),
                "cross": ("xout", "ph2"), "stream": ("xout", "xn_out", "kv_new")}[self.kind]

    # -- what the launch must leave alone
    def untouched_problems(self, sb, skv_before, appended=True):
        """rows of the inactive stream keep the sentinel, rows >= nh are what the spec says, the K|V pool is bit for bit what
        it was except the rows of the new tokens (skv_before: a copy taken before the launch)"""
        W, d, H, bad = self.W, self.d, self.H, []
        for name in self.outputs():
            buf = getattr(sb, name)
            flat = buf.reshape(S * W, -1)
            ina = flat[INACTIVE * W:(INACTIVE + 1) * W]
            if name in ("ph1", "ph2"):
                nph = H // self.hpw
                used = self._elems(sb, name)[:S * W * nph * d].view(S * W, nph * d)
                rest = self._elems(sb, name)[S * W * nph * d:]
                ina = used[INACTIVE * W:(INACTIVE + 1) * W]
                if rest.numel() and not bool((rest == SENTINEL).all()):
                    bad.append(f"{name}: more than H / {self.hpw} partial slots per row written")
                for st in self.streams:
                    if st.active:
                        live = used[st.s * W:(st.s + 1) * W]
                        if bool((live == SENTINEL).any()):
                            bad.append(f"{name}: stream {st.s}: fewer than H / {self.hpw} partial slots per row written")
                        if not bool((live[st.nh:] == 0).all()):
                            bad.append(f"{name}: stream {st.s}: rows >= nh are not zero")
            elif name == "datt":
                for st in self.streams:
                    if st.active and not bool((flat[st.s * W + st.nh:(st.s + 1) * W] == SENTINEL).all()):
                        bad.append(f"datt: stream {st.s}: rows >= nh written")
            if not bool((ina == SENTINEL).all()):
                bad.append(f"{name}: rows of the inactive stream written")
        after = sb.skv.view(S, self.nl, self.kv_rows, 2 * d).clone()
        before = skv_before.view(S, self.nl, self.kv_rows, 2 * d)
        if appended:
            for s, r in self.new_rows.items():
                r = torch.from_numpy(r).to(after.device)
                after[s, self.li, r] = before[s, self.li, r]
        it = torch.int32 if after.dtype == torch.float32 else torch.int16
        if not torch.equal(after.view(it), before.view(it)):
            bad.append("skv: an element outside the new tokens' rows changed")
        return bad


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 transcription of a fused launch (kappa_ref of the fp16 decoder mode; it runs on an fp32 case too)
def _chain32(a, W):
    """[M][K] . [N][K]^T, one k-ordered fp32 chain per element (dense_ref.chain32)"""
    a64, W64 = a.astype(np.float64), W.astype(np.float64)
    acc = np.zeros((a.shape[0], W.shape[0]), np.float32)
    for k in range(a.shape[1]):
        acc = (acc + a64[:, k, None] * W64[None, :, k]).astype(np.float32)
    return acc


def _ln32(x, g, b, eps):
    x = x.astype(np.float32)
    n = np.float32(x.shape[-1])
    xc = x - x.sum(-1, keepdims=True, dtype=np.float32) / n
    rstd = np.float32(1.0) / np.sqrt((xc * xc).sum(-1, keepdims=True, dtype=np.float32) / n + np.float32(eps))
    return xc * rstd * g.astype(np.float32) + b.astype(np.float32)


def transcription(case):
    """name -> {stream: rows} of a "self" / "cross" case in fp32 arithmetic, rounded where the form rounds"""
    assert case.kind in ("self", "cross")
    f32 = np.float32
    d, H, dk, W, li = case.d, case.H, case.dk, case.W, case.li
    lw = case.w["dec"][li]
    rnd = f16 if case.wh else (lambda a: np.asarray(a, f32))
    out = {}
    for st in case.streams:
        if not st.active:
            continue
        nh, t = st.nh, case._t[st.s]
        if "x" in t:
            x = t["x"]
        else:
            part = t["part"].astype(f32)
            if case.kind == "cross" and part.shape[0] == H and H >= 4:       # one partial per head: aligned groups of four
                y = None
                for g in range(0, H, 4):
                    s4 = ((part[g] + part[g + 1]) + part[g + 2]) + part[g + 3]
                    y = s4 if y is None else y + s4
            elif case.kind == "cross":
                y = part[0]
                for z in range(1, part.shape[0]):
                    y = y + part[z]
            else:                                                            # split sums: trees of eight, in order
                y = None
                for z0 in range(0, part.shape[0], 8):
                    p8 = list(part[z0:z0 + 8]) + [np.zeros_like(part[0])] * (8 - len(part[z0:z0 + 8]))
                    t8 = ((p8[0] + p8[1]) + (p8[2] + p8[3])) + ((p8[4] + p8[5]) + (p8[6] + p8[7]))
                    y = t8 if y is None else y + t8
            x = t["xin"] + (y + t["bias"].astype(f32))
        ln = "ln2" if case.kind == "cross" else "ln1"
        xn = _ln32(x, lw[ln + "_g"], lw[ln + "_b"], case.eps)[:nh]
        Wp, bp = (lw["wq"], lw["bq"]) if case.kind == "cross" else (lw["wqkv"], lw["bqkv"])
        y = _chain32(rnd(xn), Wp.astype(f32)) + bp.astype(f32)
        q = (y[:, :d] / f32(math.sqrt(dk))).reshape(nh, H, dk)
        if case.kind == "cross":
            kv = case.ckv[st.s, li, :st.T].astype(f32)
            K = np.broadcast_to(kv[None, :, :d].reshape(1, st.T, H, dk), (nh, st.T, H, dk))
            V = np.broadcast_to(kv[None, :, d:].reshape(1, st.T, H, dk), (nh, st.T, H, dk))
        else:
            Lc = st.L - 1
            kv = case.skv[st.s, li].astype(f32)[st.anc[:Lc]]                  # [Lc][nh][2d]
            kn, vn = y[:, d:2 * d].reshape(nh, 1, H, dk), y[:, 2 * d:].reshape(nh, 1, H, dk)
            K = np.concatenate([kv[:, :, :d].transpose(1, 0, 2).reshape(nh, Lc, H, dk), kn], 1)
            V = np.concatenate([kv[:, :, d:].transpose(1, 0, 2).reshape(nh, Lc, H, dk), vn], 1)
        s = np.einsum("hgd,hngd->hgn", q, K).astype(f32)
        p = np.exp(s - s.max(-1, keepdims=True)).astype(f32)
        ctx = (np.einsum("hgn,hngd->hgd", p, V).astype(f32) / p.sum(-1, dtype=f32)[:, :, None]).reshape(nh, d)
        Wo = (lw["wo2"] if case.kind == "cross" else lw["wo"]).astype(f32)
        ph = np.zeros((nh, H // case.hpw, d), f32)
        for h in range(H):
            c = slice(h * dk, (h + 1) * dk)
            o = _chain32(rnd(ctx[:, c]), Wo[:, c])
            ph[:, h // case.hpw] = o if h % case.hpw == 0 else ph[:, h // case.hpw] + o
        if case.part_half:
            ph = f16(ph)
        out.setdefault("xout", {})[st.s] = x
        out.setdefault("ph2" if case.kind == "cross" else "ph1", {})[st.s] = ph
        if case.kind == "self":
            out.setdefault("kv_new", {})[st.s] = y[:, d:]
    return out


def transcription_kappas(case):
    """kappa_ref of an fp16-decoder-mode case: the kappa the transcription needs, per output"""
    t = transcription(case)
    return {name: max(kappa(rows[s], case.ref[name][s], case.A[name][s]) for s in rows) for name, rows in t.items()}


def validity_problems(case):
    """the tables of a case are valid: entries < kv_rows, the new tokens' rows distinct, rows shared only with a shared past,
    and no live hypothesis is left without a key"""
    bad = []
    if not (0 <= case.anc.min() and case.anc.max() < case.kv_rows):
        bad.append("anc entry outside the pool")
    for st in case.streams:
        if not st.active:
            continue
        if st.nh < 1 or st.T < 1 or st.L < 1:
            bad.append(f"stream {st.s}: a hypothesis without any key")
        new = st.anc[st.L - 1]
        if len(set(new.tolist())) != st.nh:
            bad.append(f"stream {st.s}: new rows not distinct")
        for p in range(1, st.L):
            same = st.anc[p][:, None] == st.anc[p][None, :]
            if (same & ~(st.anc[p - 1][:, None] == st.anc[p - 1][None, :])).any():
                bad.append(f"stream {st.s}: position {p}: a shared row with different pasts")
                break
        flat = st.anc.reshape(-1)
        by_pos = [set(r.tolist()) for r in st.anc]
        if sum(len(b) for b in by_pos) != len(set(flat.tolist())):
            bad.append(f"stream {st.s}: a pool row named at two positions")
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# the launches (the same calls on a SpecBackend and a HipBackend)
def launch(be, sb, case, which=None):
    if case.kind == "attn":
        (be.dec_self_attn if which == "self" else be.dec_cross_attn)(sb, case.li)
    elif case.kind == "self":
        be.dec_layer_self(sb, case.li, sb.dx, sb.dxn, case.npart)
    elif case.kind == "cross":
        be.dec_layer_cross(sb, case.li, sb.dx, sb.dxn)
    else:
        be.dec_layer_stream(sb, case.li, sb.dx, sb.dxn, sb.dq, case.npart)


@functools.lru_cache(maxsize=None)
def spec_batch(geom, W):
    from oracle.kernel_spec import SpecBackend
    from test_engine_spec import make_batch
    return make_batch(cfg_name(geom), 1234, "meanstd", W, False, backend=SpecBackend(), **batch_kwargs(W))


def spec_kappas(case, which=None):
    """kappa_ref: the kappa the fp32 torch spec needs on this case, per output"""
    from oracle.kernel_spec import SpecBackend
    sc = spec_batch(case.geom, case.W)
    case.apply(sc)
    be = SpecBackend()
    be.dec_hpw = case.hpw
    launch(be, sc, case, which)
    return case.kappas(sc, case.result_names(which))


def layer_variant(k):
    """(layer, npart) of the fused forms: layer 0 = embedding + PE; a later layer with one partial sum and with 11 (the reduce
    crosses a batch of eight)"""
    return ((0, 1), (1, 1), (1, 11))[k % 3]

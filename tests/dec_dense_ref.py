"""Cases, float64 references, error model and numpy transcriptions for the decoder's dense launches: sc_dec_embed,
sc_dec_layer_ffn (gemm.hip: ffn_fused_kernel<PRO>), sc_dec_layer_ffn_xn, sc_dec_layer_reduce_ln and sc_dec_output_logits in
both of its forms (reduce_ln_rows_kernel + sc_gemm; reduce_ln_proj_kernel).  numpy float64 throughout, no GPU, and none of the
arithmetic of oracle/kernel_spec.py: tests/test_dec_dense_ref_spec.py holds these references to the torch spec on the CPU,
tests/test_gpu_decoder_dense.py holds the HIP kernels to them.

A CASE is the data of ALL S*W rows of a batch, by row id (9 streams of beam 10, or 18 of beam 5: 90 rows), for one launch kind,
geometry and operand family.  A LAUNCH of it names a row count M and a row table (ROWMAP): the first M entries of the table are
the rows the launch processes.  `buffers(M, perm)` gives the launch's input buffers with NaN in every row the table does not
list (and in the other layer's slots, partial slots >= n_part, ...), so one set of per-row references serves every M and every
table - and a row's result must not depend on either, in bits.  The tables: DESCENDING (the streams in descending order, a gap
stream and the inactive stream last) and SHUFFLED (a seeded permutation of the rows).  Stream INACTIVE has ctrl active = 0 and
stream SHORT has nh < W; only sc_dec_embed reads ctrl - for the dense launches nh < W shows as what sc_dec_layer_cross leaves in
the rows >= nh: partial products of zero.

GEOMETRIES (two decoder layers, one encoder layer; the launches address layer 1 and check that layer 0's slots stay as they are):
  D8    d 256, 8 heads, F 2048, V 1024   16 chunks: the largest count that still allows one chunk per workgroup
  D4    d 256, 4 heads of 64, F 2048, V 1280
  F18   d 256, 8 heads, F 2304, V 1024   18 chunks: always aligned pairs, 9 groups, a second batch of the tree
  D128  d 128, 4 heads, F 640, V 1024    sc_dec_layer_fused_supported(128, 4, W, 640) = 1: accepted, 5 chunks (odd: never pairs)

FAMILIES: normal (N(0,1) operands); offset (xin + 100: the LayerNorm's mean dominates); zero (every third row: partials of zero
and xin = -bias, so that x is exactly zero and the LayerNorm divides by sqrt(eps = 1e-12) - for sc_dec_layer_ffn_xn the rows
themselves are zero, the pre-activation is b1, and hidden unit RELU_UNIT of layer 1, whose bias the test model sets to 0, lies
exactly on the ReLU boundary); cancel (partial sums of alternating sign, +-(50 + N(0,1)), that cancel).

ERROR MODEL (dec_attn_ref.py, dense_ref.py, dense16_ref.py).  Every reference value y comes with A(y), the sum of the absolute
values of the terms a rounding of its computation is proportional to, in units of 2^-24; kappa = max |result - y| / E(y),
E = 2^-24 A.  Reduced-precision forms add their representation terms to A (in the same units, x 2^24):
  feed-forward weights fp16 (w1_h / w2_h)   the fp16 weights are the operands; xn and the hidden row are rounded to fp16 when
                                            they are staged into LDS: sum |w| r(a), r(p) = max(2^-11 |p|, 2^-25)
  feed-forward weights split16 (w1_s)       dense16_ref.rep_term("split16")
  sc_search.act_half & 2                    ph2 / ffn_part hold fp16 elements.  What a launch READS is taken as given (the cases
                                            write fp16 numbers).  What sc_dec_layer_ffn STORES is rounded once, at the store,
                                            from the fp32 partial result of a chunk group (gemm.hip: the h16x4 store at the end
                                            of ffn_fused_kernel): r(p) for every stored partial p
  sc_search.act_half & 4                    the output layer takes out_w_qh (fp16 weights: the operands) and rounds the
                                            LayerNorm row to fp16 on its way from LDS into the MFMA (decoder_panel.hip:
                                            reduce_ln_proj_kernel<WH>): sum |w| r(xn)
Accumulators, LayerNorms, biases and residuals are fp32 in every form.  Where E = 0 the result must be the reference's bits:
sc_dec_embed at d = 256, where embed * sqrt(d) = embed * 16 is exact and the sum is rounded once however it is contracted.
At d = 128 sqrt(d) is an fp32 constant and the product rounds (or is contracted into the sum, which the kernel does not
document): there E = 2^-24 (|embed| sqrt(d) + |pe|) and kappa_ref is the spec's, as for every fp32 case.

PLANTED MISTAKES of the head partials.  FfnArgs carries a grouping argument (4: one partial per head, summed in aligned groups
of four; 1: the producer summed them).  Taking 1 where 4 is meant adds the SAME eight numbers of a row in another order: a
reordering of roundings, which no measure against float64 can see (the bit identities of the GPU test do: the split launch and
the one launch must agree).  What kappa can see is a wrong ADDRESS: "head_slots" reads slot z of a listed row at 2 z (mod the
slot count) - finite numbers of the right row, half of them twice -, "head_layout" reads H slots per row where the four-head
launch wrote H / 4 (whole rows off, and the poison behind the extent).

kappa_ref.  fp32 cases (fp32 weights, act_half = 0): the kappa the fp32 torch spec (SpecBackend) needs on the same case.
SpecBackend has no fp16 or split16 mode: for those cases kappa_ref is the kappa the numpy TRANSCRIPTION of the documented
arithmetic needs - fp32 k-ordered chains with one rounding per term, the operands rounded / split where the kernel does, the
head partials in the canonical order of common.h (aligned groups of four heads in head order, the groups in order), the chunk
results per group (one chunk or an aligned pair), stored partials rounded to fp16, the consumer's tree of eight.  The GPU test
allows a kernel 4 x kappa_ref.  "ffn@form" is the second measure, after "X@form" of dense16_ref: every STORED partial against
the float64 evaluation of the FORM - the fp16 rounding of the reference's partial, or of any value within 8 x 2^-24 A of it
(where a rounding boundary lies that close an fp32 sum may fall on the other side) - in units of the partial's fp32 scale.
The rounding happens at the store, so nothing dilutes it: the transcription's figure is 0, a kernel's must be 0 too, and only
this measure sees a kernel that keeps fp32 partials in fp16 mode (closer to the exact reference)."""
import dataclasses
import functools
import math

import numpy as np
import torch

import dense16_ref as d16
from dec_attn_ref import EPS, SENTINEL, f16, head_partials_ref, kappa as _kappa, layer_norm_ref, linear_ref   # noqa: F401
from dense_ref import chain32, layer_norm32, tree8_32

F32, F64, F16 = np.float32, np.float64, np.float16
U24 = 2.0 ** 24
LCAP, TCAP = 40, 64
INACTIVE, GAP, SHORT = 2, 5, 1       # streams: ctrl active = 0; listed last but one (a gap in the descending order); nh < W
RELU_UNIT = 7                        # hidden unit of layer 1 whose bias the test model sets to 0
LI = 1                               # the layer the launches address
OTHER_TOKEN = 5                      # sc_dec_embed: the id at every position of yseq that the launch must not read
M_EDGES = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 79, 80, 81, 90)     # the 16-row tile edges up to rtt = 5
FAMILIES = ("normal", "offset", "zero", "cancel")
NPARTS = (1, 2, 8, 9, 16)
GEOMS = {"D8": dict(d_model=256, dec_heads=8, ffn_dim=2048, vocab_size=1024),
         "D4": dict(d_model=256, dec_heads=4, ffn_dim=2048, vocab_size=1280),
         "F18": dict(d_model=256, dec_heads=8, ffn_dim=2304, vocab_size=1024),
         "D128": dict(d_model=128, dec_heads=4, ffn_dim=640, vocab_size=1024)}
# (geometry, beam, heads per workgroup, feed-forward weight form, act_half) of the feed-forward launches
FFN_CONFIGS = [("D8", 10, 1, "float32", 0), ("D8", 10, 4, "float32", 0), ("D8", 5, 1, "float32", 0), ("D4", 10, 1, "float32", 0),
               ("F18", 10, 1, "float32", 0), ("D128", 10, 1, "float32", 0), ("D8", 10, 1, "float16", 0), ("D8", 10, 1, "split16", 0),
               ("D8", 10, 1, "float32", 1), ("D8", 10, 1, "float32", 2), ("D8", 10, 4, "float32", 3), ("D8", 10, 1, "float16", 3)]
# (geometry, beam, act_half) of the output layer: V 1024 and 1280 in the rows-then-GEMM form, fp16 partial sums, the row panels
LOGITS_CONFIGS = [("D8", 10, 0), ("D4", 10, 0), ("D128", 10, 0), ("D8", 5, 0), ("D8", 10, 2), ("D8", 10, 3), ("D8", 10, 7)]
FFN_MISTAKES = ("bias_twice", "ln_before_residual", "head_layout", "head_slots", "parts_fp32_in_half")
LOGITS_MISTAKES = ("drop_last_partial", "bias_twice", "ln_before_residual", "by_position", "half_as_fp32")


def nparts_of(geom):
    """the partial counts of the output layer's cases: NPARTS as far as the batch's ffn_part holds them, and its slot count"""
    mp = GEOMS[geom]["ffn_dim"] // 128
    return [p for p in NPARTS if p <= mp] + ([mp] if mp not in NPARTS and mp < 16 else [])


def fp32_case(wform, act_half):
    return wform == "float32" and not act_half


def config_of(geom):
    from speechcatcher_amd.config import ModelConfig
    return ModelConfig(enc_heads=4, enc_layers=1, dec_layers=2, **GEOMS[geom])


def cfg_name(geom):
    """registers the geometry in test_engine_spec.CFGS, as dec_attn_ref.cfg_name does"""
    import test_engine_spec
    name = "DECDENSE_" + geom
    test_engine_spec.CFGS.setdefault(name, config_of(geom))
    return name


def state_dict(geom):
    """the seeded weights of test_engine_spec.make_batch with ONE change: the bias of hidden unit RELU_UNIT of layer 1 is 0"""
    from speechcatcher_amd import synth
    sd = synth.make_state_dict(config_of(geom), 1234)
    sd[f"decoder.decoders.{LI}.feed_forward.w_1.bias"][RELU_UNIT] = 0.0
    return sd


def make_batch(geom, W, S, backend=None, device="cpu", ffn_dtype="float32", dec_dtype="float32", kv_dtype="float32"):
    from oracle.kernel_spec import SpecBackend
    from speechcatcher_amd import synth
    from speechcatcher_amd.config import SearchConfig
    from speechcatcher_amd.engine import StreamBatch
    from speechcatcher_amd.weights import PackedWeights
    cfg = config_of(geom)
    cfg_name(geom)
    mean, std = synth.stats_to_mean_std(synth.make_stats(cfg, kind="meanstd"))
    w = PackedWeights(state_dict(geom), cfg, device, mean, std, ffn_dtype=ffn_dtype, dec_dtype=dec_dtype)
    return StreamBatch(w, backend or SpecBackend(), S, SearchConfig(beam_size=W), max_frames=TCAP, max_tokens=LCAP,
                       pcm_capacity=1 << 12, max_chunk_samples=2048, kv_dtype=kv_dtype, kv_pool_rows=4 * W)


@functools.lru_cache(maxsize=None)
def spec_batch(geom, W, S):
    return make_batch(geom, W, S)


@functools.lru_cache(maxsize=None)
def weights64(geom):
    """the model's fp32 weights as float64 arrays"""
    cfg, sd = config_of(geom), state_dict(geom)
    n = lambda k: sd[k].detach().double().numpy()   # noqa: E731
    p = f"decoder.decoders.{LI}."
    from speechcatcher_amd.weights import positional_encoding_table
    return dict(bo2=n(p + "src_attn.linear_out.bias"), ln3_g=n(p + "norm3.weight"), ln3_b=n(p + "norm3.bias"),
                w1=n(p + "feed_forward.w_1.weight"), b1=n(p + "feed_forward.w_1.bias"), w2=n(p + "feed_forward.w_2.weight"),
                b2=n(p + "feed_forward.w_2.bias"), norm_g=n("decoder.after_norm.weight"), norm_b=n("decoder.after_norm.bias"),
                out_w=n("decoder.output_layer.weight"), out_b=n("decoder.output_layer.bias"), embed=n("decoder.embed.0.weight"),
                pe=positional_encoding_table(cfg.pe_max_len, cfg.d_model)[:LCAP + 1].double().numpy(), eps=cfg.ln_eps)


# ---------------------------------------------------------------------------------------------------------------------
# rows of a launch
def rowmaps(S, W):
    """name -> permutation of the S*W row ids.  descending: the rows of the streams in descending stream order, the gap stream and
    the inactive stream last; shuffled: a seeded permutation of the rows"""
    order = [s for s in reversed(range(S)) if s not in (GAP, INACTIVE)] + [GAP, INACTIVE]
    desc = np.concatenate([np.arange(s * W, (s + 1) * W) for s in order]).astype(np.int32)
    return {"descending": desc, "shuffled": np.random.default_rng(7).permutation(S * W).astype(np.int32)}


def short_nh(W):
    return max(W - 3, 1)


def n_part_rule(F, max_part, part_half=False):
    """the values the documented rule (scasr.h: sc_dec_layer_ffn) allows n_part: F/128 (one chunk per workgroup) or F/256
    (aligned pairs), never more than max_part, and pairs only - and then always - when F > 2048 (with F/128 even).  With fp16
    partial sums, which are rounded at the store, the count is a function of F alone: pairs whenever F/128 is even"""
    nch = F // 128
    pairs_only = nch % 2 == 0 and (nch > 16 or part_half)
    return [nch // c for c in (1, 2) if nch % c == 0 and nch // c <= max_part and not (pairs_only and c != 2)]


def kappa(got, ref, A):
    """dense_ref.kappa: where A = 0 the result must be the reference itself"""
    got, ref, A = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(A, F64)
    live = A > 0
    if not np.array_equal(got[~live], ref[~live]):
        return float("inf")
    return _kappa(got[live], ref[live], A[live])


def _r(x):
    return d16._r(x)


def _nan(*shape):
    return np.full(shape, np.nan, F32)


def _half_interval(p, Ap):
    """the fp16 numbers a partial may be stored as: the roundings of the values within 8 x 2^-24 A of the reference (an fp32
    sum is that close, and rounding is monotone) - one number unless a rounding boundary lies that close"""
    tol = 8.0 * EPS * Ap
    with np.errstate(over="ignore"):
        return (p - tol).astype(F16).astype(F64), (p + tol).astype(F16).astype(F64)


# ---------------------------------------------------------------------------------------------------------------------
class _Rows:
    """what the cases share: geometry, rows, tables, the masks of a launch"""

    def _init_rows(self, geom, W, family, tag, S=None):
        cfg = config_of(geom)
        self.geom, self.W, self.family = geom, W, family
        self.S = S or 90 // W                                    # (S given: the one large batch)
        self.n, self.d, self.H, self.F, self.V = self.S * W, cfg.d_model, cfg.dec_heads, cfg.ffn_dim, cfg.vocab_size
        self.w = weights64(geom)
        self.rng = np.random.default_rng([tag, list(GEOMS).index(geom), W, FAMILIES.index(family)])
        self.maps = rowmaps(self.S, W)
        self.zero_rows = np.zeros(self.n, bool)
        if family == "zero":
            self.zero_rows[::3] = True

    def listed(self, M, perm):
        m = np.zeros(self.n, bool)
        m[self.maps[perm][:M]] = True
        return m

    def _x(self):
        x = 2.0 * self.rng.standard_normal((self.n, self.d))
        return x + 100.0 if self.family == "offset" else x

    def _partials(self, k):
        """[n][k][d] by family"""
        p = 0.5 * self.rng.standard_normal((self.n, k, self.d))
        if self.family == "cancel":
            p = (50.0 + self.rng.standard_normal((self.n, k, self.d))) * np.where(np.arange(k) % 2 == 0, 1.0, -1.0)[None, :, None]
        p[self.zero_rows] = 0.0
        return p


class FfnCase(_Rows):
    """sc_dec_layer_ffn, sc_dec_layer_reduce_ln and sc_dec_layer_ffn_xn on layer LI: inputs xin (dx) and the cross-attention's
    head partials ph2 ([n][nph][d], fp16 numbers with act_half & 2); for the prologue-less form xn_in (dq).  References by row
    id: xout, xn, the chunk partials c[k] = relu(xn W1^T + b1)[chunk k] W2[:, chunk k]^T with their A, the same from xn_in."""

    def __init__(self, geom, W, family, hpw=1, wform="float32", act_half=0, S=None):
        self._init_rows(geom, W, family, 1, S)
        self.hpw, self.wform, self.act_half = hpw, wform, act_half
        self.part_half, self._t32 = bool(act_half & 2), {}
        self.nph = self.H // hpw
        self.nch = self.F // 128
        self.name = f"ffn:{geom},W={W},hpw={hpw},{wform},act_half={act_half},{family}"
        w, n, d = self.w, self.n, self.d
        xin, ph = self._x(), self._partials(self.nph)
        nh = short_nh(W)
        ph[SHORT * W + nh:(SHORT + 1) * W] = 0.0                 # rows >= nh: what sc_dec_layer_cross leaves there
        self.xin = xin.astype(F32)
        self.xin[self.zero_rows] = -w["bo2"].astype(F32)         # x = -bo2 + (0 + bo2) = 0 exactly
        self.ph = f16(ph) if self.part_half else ph.astype(F32)
        xn_in = self.rng.standard_normal((n, d))
        xn_in[self.zero_rows] = 0.0
        self.xn_in = xn_in.astype(F32)
        # the weights as the form takes them
        self.W1 = f16(w["w1"]).astype(F64) if wform == "float16" else w["w1"]
        self.W2 = f16(w["w2"]).astype(F64) if wform == "float16" else w["w2"]
        # references
        x64, p64 = self.xin.astype(F64), self.ph.astype(F64)
        self.ref, self.A = {}, {}
        x = x64 + (p64.sum(1) + w["bo2"])
        Ax = np.abs(x64) + np.abs(p64).sum(1) + np.abs(w["bo2"])
        if family == "zero":
            assert (x[self.zero_rows] == 0).all()
        xn, Axn = layer_norm_ref(x, Ax, w["ln3_g"], w["ln3_b"], w["eps"])
        self.ref["xout"], self.A["xout"], self.ref["xn"], self.A["xn"] = x, Ax, xn, Axn
        self.ref["c"], self.A["c"], self.hidden = self._ffn_ref(xn, Axn)
        self.ref["c_xn"], self.A["c_xn"], hid = self._ffn_ref(self.xn_in.astype(F64), np.zeros((n, d)))
        if family == "zero":                                     # the family is what it is called
            assert (hid[self.zero_rows][:, RELU_UNIT] == 0).all() and (hid[self.zero_rows] >= 0).all()

    def _ffn_ref(self, xn, Axn):
        """-> chunk partials [nch][n][d], their A, the hidden rows"""
        w, W1, W2 = self.w, self.W1, self.W2
        h, Ah = linear_ref(xn, Axn, W1, w["b1"])
        if self.wform != "float32":
            Ah = Ah + U24 * d16.rep_term(self.wform, xn, W1)[0]
        h = np.maximum(h, 0.0)
        c, Ac = [], []
        for k in range(self.nch):
            s = slice(128 * k, 128 * (k + 1))
            ck, Ak = linear_ref(h[:, s], Ah[:, s], W2[:, s], 0.0)
            if self.wform != "float32":
                Ak = Ak + U24 * d16.rep_term(self.wform, h[:, s], W2[:, s])[0]
            c.append(ck), Ac.append(Ak)
        return np.stack(c), np.stack(Ac), h

    # -- the reduced feed-forward of a launch that left n_part groups
    def reduced(self, n_part, which="c"):
        """(y, A) of sum over the groups; with fp16 partials A gains r(p) of every stored partial"""
        c, Ac = self.ref[which], self.A[which]
        y, A = c.sum(0), Ac.sum(0)
        if self.part_half and which == "c":
            cpw = self.nch // n_part
            A = A + U24 * sum(_r(c[g * cpw:(g + 1) * cpw].sum(0)) for g in range(n_part))
        return y, A

    def form_kappa(self, rows, parts):
        """"ffn@form": every STORED partial against the form - it is the fp16 rounding of a value within 8 x 2^-24 A of the
        reference's partial of its chunk group - in units of the partial's own 2^-24 A.  0 unless a partial was not rounded to
        fp16 where the form says, or is further off than fp32 sums can be."""
        c, Ac = self.ref["c"], self.A["c"]
        n_part = parts.shape[0]
        cpw, worst = self.nch // n_part, 0.0
        for g in range(n_part):
            p, Ap = c[g * cpw:(g + 1) * cpw].sum(0)[rows], Ac[g * cpw:(g + 1) * cpw].sum(0)[rows]
            lo, hi = _half_interval(p, Ap)
            got = parts[g].astype(F64)
            if not np.isfinite(got).all():
                return float("inf")
            worst = max(worst, float((np.maximum(np.maximum(lo - got, got - hi), 0.0) / (EPS * Ap)).max()))
        return worst

    # -- buffers of a launch (numpy, as the batch holds them)
    def buffers(self, M, perm):
        """dx, ph2 ([n][H][d] floats; the first nph slots of a row - in fp16 mode the first n*nph*d fp16 ELEMENTS of the buffer -
        are the partials), dq (xn_in); NaN wherever the launch must not read"""
        n, d, H, nph = self.n, self.d, self.H, self.nph
        on = self.listed(M, perm)
        dx, dq = _nan(n, d), _nan(n, d)
        dx[on], dq[on] = self.xin[on], self.xn_in[on]
        if self.part_half:
            ph2 = np.full(2 * n * H * d, np.nan, F16)
            v = ph2[:n * nph * d].reshape(n, nph, d)
            v[on] = self.ph[on].astype(F16)
            ph2 = ph2.view(F32).reshape(n, H, d)
        else:
            ph2 = _nan(n * H * d)
            v = ph2[:n * nph * d].reshape(n, nph, d)
            v[on] = self.ph[on]
            ph2 = ph2.reshape(n, H, d)
        return dict(dx=dx, ph2=ph2, dq=dq)

    def read_partials(self, ph2, layout_nph=None):
        """the head partials [n][nph][d] as a consumer with `layout_nph` partials per row reads them out of the buffer"""
        nph = layout_nph or self.nph
        flat = ph2.reshape(-1).view(F16).astype(F32) if self.part_half else ph2.reshape(-1)
        return flat[:self.n * nph * self.d].reshape(self.n, nph, self.d)

    # -- the fp32 transcription of one launch
    def _chunks32(self, M, perm, mistake, xn_form):
        """rows, xout, xn and the chunk results [nch][M][d] of a launch in fp32 arithmetic (kept: the group count varies)"""
        key = (M, perm, mistake if mistake != "parts_fp32_in_half" else None, xn_form)
        hit = self._t32.get(key)
        if hit is not None:
            return hit
        w = self.w
        rows = self.maps[perm][:M]
        b = self.buffers(M, perm)
        f = lambda a: np.asarray(a, F32)   # noqa: E731
        if xn_form:
            x, xn = None, b["dq"][rows]
        else:
            wrong = mistake == "head_layout" and self.nph != self.H
            ph = self.read_partials(b["ph2"], self.H if wrong else None)[rows]
            k = ph.shape[1]
            if mistake == "head_slots":                          # slot z read at 2 z (mod k): half of a row's partials twice
                ph = ph[:, (2 * np.arange(k)) % k]
            with np.errstate(invalid="ignore"):
                if k == self.H and k >= 4:                       # one partial per head: aligned groups of four, the groups in order
                    y = None
                    for g in range(0, k, 4):
                        t = ((ph[:, g] + ph[:, g + 1]) + ph[:, g + 2]) + ph[:, g + 3]
                        y = t if y is None else y + t
                else:                                            # the producer summed the groups: in order
                    y = ph[:, 0]
                    for z in range(1, k):
                        y = y + ph[:, z]
                bo2 = f(w["bo2"])
                x = b["dx"][rows] + (y + bo2)
                if mistake == "bias_twice":
                    x = x + bo2
                xn = layer_norm32(b["dx"][rows] if mistake == "ln_before_residual" else x, w["ln3_g"], w["ln3_b"], w["eps"])
        with np.errstate(invalid="ignore", over="ignore"):
            if self.wform == "split16":
                hh, c = d16.split_sum(xn, f(w["w1"]))
                h = hh + c
            else:
                h = chain32(f16(xn) if self.wform == "float16" else xn, f(self.W1))
            h = np.maximum(h + f(w["b1"]), F32(0))
            chunks = []
            for k in range(self.nch):
                s = slice(128 * k, 128 * (k + 1))
                if self.wform == "split16":
                    hh, c = d16.split_sum(h[:, s], f(w["w2"])[:, s])
                    chunks.append(hh + c)
                else:
                    chunks.append(chain32(f16(h[:, s]) if self.wform == "float16" else h[:, s], f(self.W2)[:, s]))
        self._t32[key] = (rows, x, xn, chunks)
        return self._t32[key]

    def transcription(self, M, perm, n_part, mistake=None, xn_form=False):
        """-> rows (the listed row ids in launch order), xout, xn [M][d] and parts [n_part][M][d] (fp16 numbers in fp16 mode)"""
        rows, x, xn, chunks = self._chunks32(M, perm, mistake, xn_form)
        cpw = self.nch // n_part
        parts = [chunks[g * cpw] if cpw == 1 else chunks[g * cpw] + chunks[g * cpw + 1] for g in range(n_part)]
        if self.part_half and not xn_form and mistake != "parts_fp32_in_half":
            parts = [f16(p) for p in parts]
        return rows, x, xn, np.stack(parts)

    def kappas_of(self, rows, x, xn, parts, xn_form=False):
        """kappa per output of a launch's results (rows in launch order; x / xn may be None)"""
        which = "c_xn" if xn_form else "c"
        y, A = self.reduced(parts.shape[0], which)
        res = {"ffn": kappa(parts.astype(F64).sum(0), y[rows], A[rows])}
        if x is not None:
            res["xout"] = kappa(x, self.ref["xout"][rows], self.A["xout"][rows])
        if xn is not None and not xn_form:
            res["xn"] = kappa(xn, self.ref["xn"][rows], self.A["xn"][rows])
        if self.part_half and not xn_form:
            res["ffn@form"] = self.form_kappa(rows, parts)
        return res


class LogitsCase(_Rows):
    """sc_dec_output_logits: inputs xin (dx) and npart partial sums by row id (fp16 numbers with act_half & 2); outputs xout
    (dxn), logits and - rows-then-GEMM form - the after_norm rows xn (dq)."""

    def __init__(self, geom, W, family, npart, act_half=0, S=None):
        self._init_rows(geom, W, family, 2 + npart, S)
        self.npart, self.act_half = npart, act_half
        self.part_half, self.out_half = bool(act_half & 2), bool(act_half & 4)
        self.name = f"logits:{geom},W={W},S={self.S},npart={npart},act_half={act_half},{family}"
        w = self.w
        xin, parts = self._x(), self._partials(npart).transpose(1, 0, 2)
        self.xin = xin.astype(F32)
        self.xin[self.zero_rows] = -w["b2"].astype(F32)
        self.parts = f16(parts) if self.part_half else parts.astype(F32)           # [npart][n][d]
        self.Wout = f16(w["out_w"]).astype(F64) if self.out_half else w["out_w"]
        x64, p64 = self.xin.astype(F64), self.parts.astype(F64)
        x = x64 + (p64.sum(0) + w["b2"])
        Ax = np.abs(x64) + np.abs(p64).sum(0) + np.abs(w["b2"])
        xn, Axn = layer_norm_ref(x, Ax, w["norm_g"], w["norm_b"], w["eps"])
        lg, Alg = linear_ref(xn, Axn, self.Wout, w["out_b"])
        if self.out_half:
            Alg = Alg + U24 * (_r(xn) @ np.abs(self.Wout).T)
        self.ref = {"xout": x, "xn": xn, "logits": lg}
        self.A = {"xout": Ax, "xn": Axn, "logits": Alg}

    def buffers(self, M, perm, max_part=None):
        """dx and ffn_part [max_part][n][d] floats (fp16 mode: the first max_part*n*d fp16 elements); NaN in unlisted rows and in
        the slots >= npart"""
        n, d = self.n, self.d
        mp = max_part or self.F // 128
        on = self.listed(M, perm)
        dx = _nan(n, d)
        dx[on] = self.xin[on]
        if self.part_half:
            fp = np.full(2 * mp * n * d, np.nan, F16)
            v = fp[:mp * n * d].reshape(mp, n, d)
            v[:self.npart, on] = self.parts[:, on].astype(F16)
            fp = fp.view(F32).reshape(mp, n, d)
        else:
            fp = _nan(mp, n, d)
            fp[:self.npart, on] = self.parts[:, on]
        return dict(dx=dx, ffn_part=fp)

    def transcription(self, M, perm, mistake=None):
        """-> rows, xout, xn [M][d], logits [M][V]"""
        w = self.w
        rows = self.maps[perm][:M]
        b = self.buffers(M, perm)
        f = lambda a: np.asarray(a, F32)   # noqa: E731
        flat = b["ffn_part"].reshape(-1)
        mp = b["ffn_part"].shape[0]
        if self.part_half and mistake != "half_as_fp32":
            flat = flat.view(F16).astype(F32)
        buf = flat[:mp * self.n * self.d].reshape(mp, self.n, self.d)
        at = np.arange(M) if mistake == "by_position" else rows
        npart = self.npart - 1 if mistake == "drop_last_partial" and self.npart == 9 else self.npart
        with np.errstate(invalid="ignore", over="ignore"):
            y = tree8_32([buf[z, at] for z in range(npart)])
            b2 = f(w["b2"])
            x = b["dx"][rows] + (y + b2)
            if mistake == "bias_twice":
                x = x + b2
            xn = layer_norm32(b["dx"][rows] if mistake == "ln_before_residual" else x, w["norm_g"], w["norm_b"], w["eps"])
            lg = chain32(f16(xn) if self.out_half else xn, f(self.Wout)) + f(w["out_b"])
        return rows, x, xn, lg

    def kappas_of(self, rows, x, xn, lg):
        res = {"xout": kappa(x, self.ref["xout"][rows], self.A["xout"][rows]),
               "logits": kappa(lg, self.ref["logits"][rows], self.A["logits"][rows])}
        if xn is not None:
            res["xn"] = kappa(xn, self.ref["xn"][rows], self.A["xn"][rows])
        return res


class EmbedCase(_Rows):
    """sc_dec_embed: L - 1 in 0, 1 and LCAP - 2; the tokens 0, V - 1 and a repeated id; nh < W; an inactive stream.
    The launch reads ctrl and yseq only: every position other than L - 1 holds OTHER_TOKEN, which no row of the case embeds."""

    def __init__(self, geom, W):
        self._init_rows(geom, W, "normal", 0)
        self.exact = self.d == 256       # sqrt(d) = 16: the product is exact and the sum rounds once, E = 0
        S, V, w = self.S, self.V, self.w
        self.name = f"embed:{geom},W={W}"
        self.ctrl = np.zeros((S, 8), np.int32)
        self.yseq = np.full((2, S, W, LCAP), OTHER_TOKEN, np.int32)
        self.L, self.nh, self.tok = {}, {}, {}
        for s in range(S):
            L = (1, 2, LCAP - 1)[s % 3]
            nh = 0 if s == INACTIVE else short_nh(W) if s == SHORT else W
            cur = s % 2
            tok = self.rng.integers(OTHER_TOKEN + 1, V - 1, W)
            tok[0], tok[-1] = 0, V - 1
            if W > 3:
                tok[2] = tok[1]                                  # a repeated id
            if s == INACTIVE:
                self.ctrl[s] = (0, cur, 0, 10, L, W, 0, 0)       # (a row that would be valid: only `active` says no)
                self.yseq[cur, s, :, L - 1] = tok
                continue
            self.ctrl[s] = (1, cur, 0, 10, L, nh, 0, 0)
            self.yseq[cur, s, :nh, L - 1] = tok[:nh]
            self.L[s], self.nh[s], self.tok[s] = L, nh, tok[:nh]
        self.ref = {s: w["embed"][self.tok[s]] * math.sqrt(self.d) + w["pe"][self.L[s] - 1] for s in self.L}
        # d = 128: sqrt(d) is an fp32 constant, the product rounds (or is contracted into the sum): one unit per term
        self.A = {s: np.abs(w["embed"][self.tok[s]]) * math.sqrt(self.d) + np.abs(w["pe"][self.L[s] - 1]) for s in self.L}
        self.ref_wrong_row = {s: w["embed"][self.tok[s]] * math.sqrt(self.d) + w["pe"][self.L[s]] for s in self.L}

    def written(self):
        m = np.zeros(self.n, bool)
        for s, nh in self.nh.items():
            m[s * self.W:s * self.W + nh] = True
        return m

    def kappa_of(self, dx):
        """d = 128: the kappa the rows need"""
        return max(kappa(dx[s * self.W:s * self.W + self.nh[s]], self.ref[s], self.A[s]) for s in self.ref)

    def problems(self, dx, kref=None):
        """dx [n][d] after the launch (it started as the sentinel); d = 128: kref = the kappa the spec needs"""
        bad = []
        keep = ~self.written()
        if not (dx[keep].view(np.int32) == np.float32(SENTINEL).view(np.int32)).all():
            bad.append("a row >= nh or of the inactive stream was written")
        for s, ref in self.ref.items():
            got = dx[s * self.W:s * self.W + self.nh[s]]
            if not self.exact:
                k = kappa(got, ref, self.A[s])
                if not k <= 4 * kref:
                    bad.append(f"stream {s} (L {self.L[s]}, nh {self.nh[s]}): kappa {k:.3g} > 4 x kappa_ref {kref:.3g}")
            elif not np.array_equal(got.view(np.int32), ref.astype(F32).view(np.int32)):
                bad.append(f"stream {s} (L {self.L[s]}, nh {self.nh[s]}): not the bits of embed[token] * sqrt(d) + pe[L - 1]")
        return bad


# ---------------------------------------------------------------------------------------------------------------------
# writing a launch into a batch, reading it back (the same on a SpecBackend batch and a HipBackend batch)
def _t(sb, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(sb.ctrl.device)


def set_rows(sb, case, M, perm):
    sb.rowmap.copy_(_t(sb, case.maps[perm]))
    sb.n_rows_step = int(M)


def fill(buf, value, half=False):
    """the whole buffer as the sentinel / NaN - in fp16 mode every fp16 element of it"""
    (buf.view(-1).view(torch.float16) if half else buf).fill_(value)


def apply_ffn(sb, case, M, perm):
    b = case.buffers(M, perm)
    set_rows(sb, case, M, perm)
    sb.dx.copy_(_t(sb, b["dx"]))
    sb.dq.copy_(_t(sb, b["dq"]))
    sb.ph2.copy_(_t(sb, b["ph2"]))
    sb.ph1.fill_(float("nan"))
    sb.dxn.fill_(SENTINEL)
    fill(sb.ffn_part, SENTINEL, case.part_half)


def apply_logits(sb, case, M, perm):
    b = case.buffers(M, perm, sb.ffn_part.shape[0])
    set_rows(sb, case, M, perm)
    sb.dx.copy_(_t(sb, b["dx"]))
    sb.ffn_part.copy_(_t(sb, b["ffn_part"]))
    for name in ("ph1", "ph2"):
        getattr(sb, name).fill_(float("nan"))
    for name in ("dxn", "dq", "logits"):
        getattr(sb, name).fill_(SENTINEL)


def apply_embed(sb, case):
    sb.ctrl.copy_(_t(sb, case.ctrl))
    sb.yseq.copy_(_t(sb, case.yseq))
    sb.dx.fill_(SENTINEL)


def read_parts(sb, half):
    """ffn_part as float32 numbers [max_part][n][d] (fp16 mode: the first half of the buffer's fp16 elements) and the mask of
    what still is the sentinel, over EVERY element of the buffer"""
    fp = sb.ffn_part
    if half:
        h = fp.view(-1).view(torch.float16)
        vals = h[:fp.numel()].view(fp.shape).float().cpu().numpy()
        rest_ok = bool((h[fp.numel():] == SENTINEL).all())
    else:
        vals, rest_ok = fp.cpu().numpy(), True
    return vals, rest_ok


def ffn_sentinel_problems(case, sb, M, perm, n_part, xout=True):
    """rows the table does not list keep the sentinel in xout and ffn_part, and so do the slots >= n_part (bit for bit)"""
    bad = []
    off = ~case.listed(M, perm)
    if xout and not bool((sb.dxn.cpu().numpy()[off] == F32(SENTINEL)).all()):
        bad.append("xout: a row the table does not list was written")
    vals, rest_ok = read_parts(sb, case.part_half)
    if not rest_ok:
        bad.append("ffn_part: fp16 elements beyond the fp16 extent of the buffer were written")
    if not (vals[n_part:] == F32(SENTINEL)).all():
        bad.append(f"ffn_part: a slot >= n_part = {n_part} was written")
    if not (vals[:n_part, off] == F32(SENTINEL)).all():
        bad.append("ffn_part: a row the table does not list was written")
    if (vals[:n_part][:, ~off] == F32(SENTINEL)).all(-1).any():
        bad.append("ffn_part: a listed row of a slot < n_part was not written")
    return bad


def logits_sentinel_problems(case, sb, M, perm, rows_form):
    bad = []
    off = ~case.listed(M, perm)
    for name in ("dxn", "logits") + (("dq",) if rows_form else ()):
        if not bool((getattr(sb, name).cpu().numpy()[off] == F32(SENTINEL)).all()):
            bad.append(f"{name}: a row the table does not list was written")
    if not rows_form and not bool((sb.dq == SENTINEL).all()):
        bad.append("dq: written by the row-panel form")
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# kappa_ref
def spec_ffn(case, M=None, perm="descending"):
    """SpecBackend on the case (fp32): kappas of xout and of the ONE partial sum it writes; the prologue-less form besides"""
    from oracle.kernel_spec import SpecBackend
    be, sb = SpecBackend(), spec_batch(case.geom, case.W, case.S)
    be.dec_hpw = case.hpw
    M = case.n if M is None else M
    rows = case.maps[perm][:M]
    apply_ffn(sb, case, M, perm)
    assert be.dec_layer_ffn(sb, LI, sb.dx, sb.dxn) == 1
    res = case.kappas_of(rows, sb.dxn.numpy()[rows], None, sb.ffn_part.numpy()[:1, rows])
    _, _, xn, _ = case.transcription(M, perm, n_part_rule(case.F, case.F // 128)[0])
    res["xn"] = kappa(xn, case.ref["xn"][rows], case.A["xn"][rows])   # (the spec keeps no norm3 rows: the transcription's)
    bad = ffn_sentinel_problems(case, sb, M, perm, 1)
    apply_ffn(sb, case, M, perm)
    assert be.dec_layer_ffn_xn(sb, LI, sb.dq) == 1
    res["ffn_xn"] = case.kappas_of(rows, None, None, sb.ffn_part.numpy()[:1, rows], xn_form=True)["ffn"]
    return res, bad + ffn_sentinel_problems(case, sb, M, perm, 1, xout=False)


def spec_logits(case, M=None, perm="descending"):
    from oracle.kernel_spec import SpecBackend
    sb = spec_batch(case.geom, case.W, case.S)
    M = case.n if M is None else M
    rows = case.maps[perm][:M]
    apply_logits(sb, case, M, perm)
    SpecBackend().dec_output_logits(sb, sb.dx, sb.dxn, case.npart)
    res = case.kappas_of(rows, sb.dxn.numpy()[rows], None, sb.logits.numpy()[rows])
    _, _, xn, _ = case.transcription(M, perm)      # (the spec keeps no after_norm rows: kappa_ref of xn is the transcription's)
    res["xn"] = kappa(xn, case.ref["xn"][rows], case.A["xn"][rows])
    return res, logits_sentinel_problems(case, sb, M, perm, False)


@functools.lru_cache(maxsize=None)
def embed_kappa_ref(geom, W):
    """the kappa SpecBackend needs on the embed case (0 at d = 256: the reference's bits)"""
    from oracle.kernel_spec import SpecBackend
    case = EmbedCase(geom, W)
    sb = spec_batch(geom, W, case.S)
    apply_embed(sb, case)
    SpecBackend().dec_embed(sb)
    return case.kappa_of(sb.dx.numpy())


@functools.lru_cache(maxsize=None)
def ffn_case(geom, W, family, hpw, wform, act_half, S=None):
    return FfnCase(geom, W, family, hpw, wform, act_half, S)


@functools.lru_cache(maxsize=None)
def logits_case(geom, W, family, npart, act_half, S=None):
    return LogitsCase(geom, W, family, npart, act_half, S)


@functools.lru_cache(maxsize=None)
def ffn_kappa_ref(geom, W, family, hpw, wform, act_half):
    """output -> kappa_ref of the case: SpecBackend's on an fp32 case, else the transcription's (all rows, at both group counts
    the rule allows: the larger)"""
    case = ffn_case(geom, W, family, hpw, wform, act_half)
    if fp32_case(wform, act_half):
        res, bad = spec_ffn(case)
        assert not bad, bad
        return res
    res = {}
    for n_part in n_part_rule(case.F, case.F // 128, case.part_half):
        k = case.kappas_of(*case.transcription(case.n, "descending", n_part))
        k["ffn_xn"] = case.kappas_of(*case.transcription(case.n, "descending", n_part, xn_form=True), xn_form=True)["ffn"]
        res = {name: max(v, res.get(name, 0.0)) for name, v in k.items()}
    return res


@functools.lru_cache(maxsize=None)
def logits_kappa_ref(geom, W, family, npart, act_half, S=None):
    case = logits_case(geom, W, family, npart, act_half, S)
    if not act_half:
        res, bad = spec_logits(case)
        assert not bad, bad
        return res
    return case.kappas_of(*case.transcription(case.n, "descending"))


@dataclasses.dataclass
class Worst:
    """the worst kappa / kappa_ref of a kernel's output over a test, for the report"""
    kappa: float = 0.0
    kappa_ref: float = 0.0
    case: str = ""

    def see(self, k, kref, name):
        if kref > 0 and (self.case == "" or k / kref > self.kappa / max(self.kappa_ref, 1e-300)):
            self.kappa, self.kappa_ref, self.case = float(k), float(kref), name

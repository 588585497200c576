"""Contract of attention rescoring of n-best lists (csrc/dec_rescore.hip: sc_seq_attention, sc_dec_rescore),
numpy float64.

A job is one list: the T encoder rows E [T][d] it was decoded from, n_hyp <= 16 rows of labels (no <sos>, no <eos>) with
m_h = lens[h] labels each (or L for all rows), the rows' first-pass totals score[h], and w_att, w_ctc, beta.  Row h is
scored as the attention decoder scores it WITHOUT a cache (oracle/ref_port.py: decoder_layer(..., cache=None),
decoder_batch_score): the inputs [sos, y_0 .. y_{m-1}] at positions 0 .. m, the targets [y_0 .. y_{m-1}, eos];
    x = embed[tok] * sqrt(d) + pe[pos]
    per layer, pre-LN: causal self-attention, cross-attention over all T rows of E, feed-forward, each with its residual
    after_norm, the output layer, log-softmax over V
    tok_att[h][t]  log-probability of target t, t in [0, m_h]; the last is the <eos> term
    att[h]         ((0.0 + tok_att[0]) + tok_att[1]) + ...                          ascending t, float64
    fused[h]       (w_ctc * score[h] + w_att * att[h]) + beta * m_h                  every product and sum rounded on its
                                                                                      own; a NaN is THE quiet NaN
    order[r]       the row at rank r: fused descending, ties to the lower row
status[h] is a set of bits.  BAD_TOKEN: lens[h] outside [0, L] (nothing else of the row is examined) or a label outside
[0, V); TOO_LONG: m_h + 1 exceeds the position table (pe_rows) or LCAP; NO_FRAMES: T == 0, for every row of the job.  A row
with one of these has att = 0.0, fused = NaN and its whole tok_att row (L + 1 entries) 0.0.  NONFINITE: score[h] is not
finite, or the fused total of a row without those bits is not.  Rows with any status rank behind all others, in row order
among themselves.  A label equal to the sos / eos id is an ordinary label.

The weights are a dict of float64 arrays (``weights64``), so the same functions serve the oracle's state dict and the
packed weights of the engine."""
import math

import numpy as np

NONFINITE, BAD_TOKEN, TOO_LONG, NO_FRAMES = 1, 2, 4, 8      # SC_ATT_* status bits
MAX_HYPS = 16
EPS = 2.0 ** -24
QNAN = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), np.float64)[0]


def weights64(sd, cfg):
    """the decoder's weights of a reference state dict (name -> tensor) as float64 arrays"""
    g = lambda k: sd[k].detach().cpu().double().numpy()   # noqa: E731
    layers = []
    for i in range(cfg.dec_layers):
        p = f"decoder.decoders.{i}"
        lw = {}
        for n in ("norm1", "norm2", "norm3"):
            lw[n] = (g(f"{p}.{n}.weight"), g(f"{p}.{n}.bias"))
        for a in ("self_attn", "src_attn"):
            for n in ("linear_q", "linear_k", "linear_v", "linear_out"):
                lw[f"{a}.{n}"] = (g(f"{p}.{a}.{n}.weight"), g(f"{p}.{a}.{n}.bias"))
        for n in ("w_1", "w_2"):
            lw[n] = (g(f"{p}.feed_forward.{n}.weight"), g(f"{p}.feed_forward.{n}.bias"))
        layers.append(lw)
    return {"embed": g("decoder.embed.0.weight"), "layers": layers,
            "after_norm": (g("decoder.after_norm.weight"), g("decoder.after_norm.bias")),
            "out": (g("decoder.output_layer.weight"), g("decoder.output_layer.bias"))}


def weights64_packed(pw):
    """the same from the engine's PackedWeights (speechcatcher_amd/weights.py), with its position table"""
    n = lambda t: t.detach().cpu().double().numpy()   # noqa: E731
    d = pw.cfg.d_model
    layers = []
    for lw in pw.dec:
        wqkv, bqkv, wkv, bkv = n(lw["wqkv"]), n(lw["bqkv"]), n(lw["wkv"]), n(lw["bkv"])
        layers.append({"norm1": (n(lw["ln1_g"]), n(lw["ln1_b"])), "norm2": (n(lw["ln2_g"]), n(lw["ln2_b"])),
                       "norm3": (n(lw["ln3_g"]), n(lw["ln3_b"])),
                       "self_attn.linear_q": (wqkv[:d], bqkv[:d]), "self_attn.linear_k": (wqkv[d:2 * d], bqkv[d:2 * d]),
                       "self_attn.linear_v": (wqkv[2 * d:], bqkv[2 * d:]), "self_attn.linear_out": (n(lw["wo"]), n(lw["bo"])),
                       "src_attn.linear_q": (n(lw["wq"]), n(lw["bq"])), "src_attn.linear_k": (wkv[:d], bkv[:d]),
                       "src_attn.linear_v": (wkv[d:], bkv[d:]), "src_attn.linear_out": (n(lw["wo2"]), n(lw["bo2"])),
                       "w_1": (n(lw["w1"]), n(lw["b1"])), "w_2": (n(lw["w2"]), n(lw["b2"]))})
    return {"embed": n(pw.embed), "layers": layers, "after_norm": (n(pw.dec_norm_g), n(pw.dec_norm_b)),
            "out": (n(pw.out_w), n(pw.out_b)), "pe": n(pw.pe)}


def layer_norm(x, gb, eps):
    mu = x.mean(-1, keepdims=True)
    xc = x - mu
    return xc / np.sqrt((xc * xc).mean(-1, keepdims=True) + eps) * gb[0] + gb[1]


def linear(x, wb):
    return x @ wb[0].T + wb[1]


def seq_attention(q, k, v, H, causal, dtype=np.float64):
    """Attention of one sequence: q [Lq][H * dk], k, v [Lk][H * dk]; key j is masked for query i when causal and j > i.
    Returns (o [Lq][H * dk], A): A is the amplitude of a context element as tests/dec_attn_ref.py defines it,
    (1 + max_j |q_i| . |k_j| / sqrt(dk)) * sum_j p_ij |v_j|, over the keys that are not masked.  ``dtype=np.float32``: the
    plain evaluation in fp32 numpy that kappa_ref is measured on (every intermediate an fp32 array)."""
    q, k, v = (np.asarray(a, dtype) for a in (q, k, v))
    Lq, Lk, dk = q.shape[0], k.shape[0], q.shape[1] // H
    o, A = np.zeros((Lq, H * dk), dtype), np.zeros((Lq, H * dk), np.float64)
    keep = np.ones((Lq, Lk), bool) if not causal else np.arange(Lk)[None, :] <= np.arange(Lq)[:, None]
    for h in range(H):
        c = slice(h * dk, (h + 1) * dk)
        s = _mm(q[:, c], k[:, c], dtype) / dtype(math.sqrt(dk))
        sabs = (np.abs(q[:, c]).astype(np.float64) @ np.abs(k[:, c]).astype(np.float64).T) / math.sqrt(dk)
        s = np.where(keep, s, dtype(-np.inf))
        p = np.where(keep, np.exp(s - s.max(-1, keepdims=True)), dtype(0))
        p = p / p.sum(-1, keepdims=True)
        o[:, c] = _mm(p, v[:, c].T, dtype)
        A[:, c] = (1.0 + np.where(keep, sabs, 0.0).max(-1))[:, None] * (p.astype(np.float64) @ np.abs(v[:, c]).astype(np.float64))
    return o, A


def _mm(a, bt, dtype):
    """a @ bt.T; in fp32 as one chain per element, k ascending (no library's blocking decides the bits)"""
    if dtype is np.float64:
        return a @ bt.T
    acc = np.zeros((a.shape[0], bt.shape[0]), dtype)
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * bt[None, :, k]
    return acc


def kappa(got, ref, A):
    """the kappa a result needs (tests/dec_attn_ref.py); inf if it is not finite"""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / (EPS * A)).max()) if got.size else 0.0


def attention_family(family, Lq, Lk, H, dk, rng):
    """q, k, v of the two families of the parity tests: "flat" - scores within a few units of each other; "dominant" - per
    query and head one key whose score is ahead of every other by 80 (40 sqrt(dk) in the product: k = a multiple of q)"""
    q = rng.standard_normal((Lq, H * dk))
    k = rng.standard_normal((Lk, H * dk))
    v = rng.standard_normal((Lk, H * dk))
    if family == "dominant":
        # every query of a head points the same way up to a positive factor, key `top` of the head points there too
        for h in range(H):
            c = slice(h * dk, (h + 1) * dk)
            u = rng.standard_normal(dk)
            u /= np.linalg.norm(u)
            q[:, c] = u * rng.uniform(4.0, 5.0, (Lq, 1)) + 0.01 * q[:, c]
            k[:, c] *= 0.5
            k[:, c] -= np.outer(k[:, c] @ u, u)                   # the other keys: orthogonal to u
            k[0, c] += u * (80.0 * math.sqrt(dk) / 4.0 + 8.0)     # key 0 is visible to every query, causal or not
    else:
        assert family == "flat"
    return q, k, v


# the shapes sc_seq_attention is held to (tests/test_gpu_dec_rescore.py) and kappa_ref is measured on
ATTN_DK, ATTN_H = (16, 32, 64), (1, 2, 8)
ATTN_LQ, ATTN_LK = (1, 2, 15, 16, 17, 33, 65), (1, 31, 32, 33, 63, 64, 65, 130)
FAMILIES = ("flat", "dominant")


def attention_cases(family, dk, causal):
    """(H, Lq, Lk, q, k, v) over the grid: causal - Lk = Lq over ATTN_LQ; full - every ATTN_LK with the ATTN_LQ in turn.
    The operands are fp32 numbers (in float64 arrays)."""
    for H in ATTN_H:
        shapes = [(a, a) for a in ATTN_LQ] if causal else [(ATTN_LQ[i % len(ATTN_LQ)], Lk) for i, Lk in enumerate(ATTN_LK)]
        for n, (Lq, Lk) in enumerate(shapes):
            rng = np.random.default_rng([ATTN_DK.index(dk), H, int(causal), n, FAMILIES.index(family)])
            q, k, v = (a.astype(np.float32).astype(np.float64) for a in attention_family(family, Lq, Lk, H, dk, rng))
            yield H, Lq, Lk, q, k, v


def tok_att(w, cfg, E, y):
    """the m + 1 log-probabilities of the targets [y_0 .. y_{m-1}, eos] of one row"""
    d, H = cfg.d_model, cfg.dec_heads
    toks = [cfg.sos_id] + [int(c) for c in y]
    m = len(y)
    x = w["embed"][toks] * math.sqrt(d) + w["pe"][:m + 1]
    E = np.asarray(E, np.float64)
    for lw in w["layers"]:
        xn = layer_norm(x, lw["norm1"], cfg.ln_eps)
        ctx, _ = seq_attention(linear(xn, lw["self_attn.linear_q"]), linear(xn, lw["self_attn.linear_k"]),
                               linear(xn, lw["self_attn.linear_v"]), H, True)
        x = x + linear(ctx, lw["self_attn.linear_out"])
        xn = layer_norm(x, lw["norm2"], cfg.ln_eps)
        ctx, _ = seq_attention(linear(xn, lw["src_attn.linear_q"]), linear(E, lw["src_attn.linear_k"]),
                               linear(E, lw["src_attn.linear_v"]), H, False)
        x = x + linear(ctx, lw["src_attn.linear_out"])
        xn = layer_norm(x, lw["norm3"], cfg.ln_eps)
        x = x + linear(np.maximum(linear(xn, lw["w_1"]), 0.0), lw["w_2"])
    logits = linear(layer_norm(x, w["after_norm"], cfg.ln_eps), w["out"])
    M = logits.max(-1, keepdims=True)
    logp = logits - (M + np.log(np.exp(logits - M).sum(-1, keepdims=True)))
    targets = [int(c) for c in y] + [cfg.eos_id]
    return logp[np.arange(m + 1), targets]


def fuse(score, att, m, w_att, w_ctc, beta):
    """(w_ctc * score + w_att * att) + beta * m, every operation rounded on its own; a NaN is THE quiet NaN"""
    with np.errstate(all="ignore"):
        f = np.float64(np.float64(np.float64(w_ctc) * np.float64(score)) + np.float64(np.float64(w_att) * np.float64(att))) \
            + np.float64(np.float64(beta) * np.float64(m))
    return QNAN if f != f else float(f)


def rank(fused, status):
    """order[r]: rows without a status by fused descending, ties to the lower row; then the rows with one, in row order"""
    n = len(fused)
    good = sorted((h for h in range(n) if not status[h]), key=lambda h: (-fused[h], h))
    return np.asarray(good + [h for h in range(n) if status[h]], np.int32)


def rescore(w, cfg, E, rows, lens, scores, w_att=1.0, w_ctc=0.5, beta=0.0, L=None, pe_rows=None, LCAP=None):
    """One job.  rows: n sequences of ints (at least lens[h] each); lens None: L labels each.  w carries "pe" [pe_rows][d].
    Returns tok_att (a list of float64 arrays: m_h + 1 values, or L + 1 zeros for a row with a status), att, fused
    (float64 [n]), order, status (int32 [n])."""
    n = len(rows)
    assert 1 <= n <= MAX_HYPS
    L = max((len(r) for r in rows), default=0) if L is None else L
    pe_rows = w["pe"].shape[0] if pe_rows is None else pe_rows
    LCAP = pe_rows if LCAP is None else LCAP
    T = 0 if E is None else int(np.asarray(E).shape[0])
    toks, att, fused, status = [], np.zeros(n), np.full(n, QNAN), np.zeros(n, np.int32)
    for h in range(n):
        ln = L if lens is None else int(lens[h])
        st = NO_FRAMES if T == 0 else 0
        y = []
        if ln < 0 or ln > L:
            st |= BAD_TOKEN
        else:
            y = [int(c) for c in rows[h][:ln]]
            if ln + 1 > pe_rows or ln + 1 > LCAP:
                st |= TOO_LONG
            if any(c < 0 or c >= cfg.vocab_size for c in y):
                st |= BAD_TOKEN
        sc = float(scores[h])
        if st:
            toks.append(np.zeros(L + 1))
        else:
            t = tok_att(w, cfg, E, y)
            a = 0.0
            for v in t:
                a = float(a + v)
            toks.append(t)
            att[h] = a
            fused[h] = fuse(sc, a, len(y), w_att, w_ctc, beta)
            if not math.isfinite(fused[h]):
                st |= NONFINITE
        if not math.isfinite(sc):
            st |= NONFINITE
        status[h] = st
    return {"tok_att": toks, "att": att, "fused": fused, "order": rank(fused, status), "status": status}

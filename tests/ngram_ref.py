"""The textbook backoff recursion of an n-gram model, evaluated on the plain dict {n-gram: (logp, backoff)} - what
speechcatcher_amd/ngram.py's packed automaton must give bit for bit.  float64.

    p(c | h) = logp[h + c]                         when the model holds h + c
             = backoff[h] + p(c | h without its oldest token)     else (backoff 0 for a context the model does not hold)
             = FLOOR                               for a token without a unigram
The backoffs are added oldest context first and the logp last, ((0 + b_1) + b_2 ...) + logp: the order the automaton's
score() fixes.  A context longer than order - 1 is cut to its last order - 1 tokens first.
"""
import math

FLOOR = -99.0 * math.log(10.0)


def logp(model, order: int, ctx, c: int) -> float:
    ctx = tuple(ctx)[max(0, len(ctx) - (order - 1)):] if order > 1 else ()
    acc = 0.0
    while True:
        if ctx + (c,) in model:
            return float(acc + model[ctx + (c,)][0])
        if not ctx:
            return float(acc + FLOOR)
        if ctx in model:
            acc = float(acc + model[ctx][1])
        ctx = ctx[1:]


def sequence(model, order: int, ids, start=()) -> float:
    """the raw sum of the scores along ``ids``, left to right, after the context ``start``"""
    lm, ctx = 0.0, tuple(start)
    for c in ids:
        lm = float(lm + logp(model, order, ctx, c))
        ctx = ctx + (c,)
    return lm


def estimate(sentences, V: int, order: int, discount: float = 0.4, bos=None):
    """an absolute-discounting backoff model from token sequences: p(w | h) = (n(h, w) - D) / n(h) for a seen h + w, the
    left-over mass of h spread by the lower order; unigrams (n(w) + 1) / (N + V), so every token has one.  Properly
    normalised: sum_w p(w | h) = 1 for every h."""
    counts = [dict() for _ in range(order + 1)]
    for s in sentences:
        s = ([bos] if bos is not None else []) + list(s)
        for n in range(1, order + 1):
            for k in range(len(s) - n + 1):
                g = tuple(s[k:k + n])
                if bos is not None and bos in g[1:]:
                    continue
                counts[n][g] = counts[n].get(g, 0) + 1
    N = sum(counts[1].values())
    model = {(w,): (math.log((counts[1].get((w,), 0) + 1) / (N + V)), 0.0) for w in range(V)}
    for n in range(2, order + 1):
        ctx_total = {}
        for g, k in counts[n].items():
            ctx_total[g[:-1]] = ctx_total.get(g[:-1], 0) + k
        for g, k in counts[n].items():
            if g[:-1] in model:
                model[g] = (math.log((k - discount) / ctx_total[g[:-1]]), 0.0)
    # backoff weights, shortest contexts first: (1 - seen mass at h) / (1 - the lower order's mass of the same tokens)
    children = {}
    for g in model:
        if len(g) > 1:
            children.setdefault(g[:-1], []).append(g[-1])
    for h in sorted(children, key=len):
        seen = children[h]
        hi = math.fsum(math.exp(model[h + (w,)][0]) for w in seen)
        lo = math.fsum(math.exp(logp(model, order, h[1:], w)) for w in seen)
        model[h] = (model[h][0], math.log((1.0 - hi) / (1.0 - lo)))
    return model

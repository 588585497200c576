"""Stable partials: which part of a partial transcript can still change.

Every live hypothesis of a stream descends from the hypotheses that were live at the previous reply, a decode step only
appends a token, and a block boundary rewinds at most the step taken last - so the prefix ALL live hypotheses share, the
committed prefix, is final: no later chunk changes it, and it only grows.  Behind it, ``stability[i]`` is the share of
the beam's probability mass that agrees with the best hypothesis up to and including token i.

The host-side form of the contract (tests/hyp_commit_ref.py; the C++ engine computes it on the GPU: sc_hyp_commit,
sc_get_hyps_delta) and ``StablePrefix``, the tracker a client keeps per stream."""
from typing import List, Optional, Sequence

import numpy as np

NONFINITE = 1            # status bit: a score of the beam is a NaN or an infinity
MAX_HYPS = 16
FIELDS = ("L", "commit", "tokens", "xpos", "stability", "score", "score_dec", "score_ctc")


def agree_lengths(yseq) -> np.ndarray:
    """[n] int32: the length of the common prefix of row h and row 0 of yseq [n, L]"""
    y = np.asarray(yseq, np.int32)
    n, L = y.shape
    if L == 0:
        return np.zeros(n, np.int32)
    diff = y != y[0]
    return np.where(diff.any(1), diff.argmax(1), L).astype(np.int32)


def beam_weights(score):
    """(w [n] float64, status): exp(score - the largest finite score); a non-finite score weighs 0 and sets NONFINITE;
    with no finite score every weight is 1 (as alternates.nbest_posterior shares the mass evenly)"""
    s = np.asarray(score, np.float64).reshape(-1)
    fin = np.isfinite(s)
    status = 0 if fin.all() else NONFINITE
    if not fin.any():
        return np.ones(s.shape[0], np.float64), status
    m = s[fin].max()
    w = np.zeros(s.shape[0], np.float64)
    for h in np.nonzero(fin)[0]:
        w[h] = np.exp(s[h] - m)
    return w, status


def stability_of(agree, w, frm: int, L: int, final: bool = False) -> np.ndarray:
    """[L - frm] float64: (the sum, in ascending h, of the w[h] with agree[h] > i) / (the sum of all w, ascending h)"""
    t = max(L - frm, 0)
    if final or t == 0:
        return np.ones(t, np.float64)
    pos = np.arange(frm, L)
    num, z = np.zeros(t, np.float64), np.float64(0.0)
    for h in range(len(w)):   # ascending h: the order the kernel adds in
        num = np.where(agree[h] > pos, num + w[h], num)
        z = z + w[h]
    return num / z


def empty_delta() -> dict:
    """the delta of a stream that has not started"""
    return {"L": 0, "commit": 0, "n_hyp": 0, "status": 0, "tokens": np.zeros(0, np.int32), "xpos": np.zeros(0, np.int32),
            "stability": np.zeros(0, np.float64), "score": 0.0, "score_dec": 0.0, "score_ctc": 0.0}


def hyp_commit(yseq, xpos, score, frm: int = 0, final: bool = False, score_dec=None, score_ctc=None) -> dict:
    """The contract over one beam: yseq / xpos [n, L], score [n], best first -> {"L", "commit", "n_hyp", "status",
    "agree" [n], "tokens" / "xpos" [L - frm] int32, "stability" [L - frm] float64, "score", "score_dec", "score_ctc"}."""
    y, x = np.asarray(yseq, np.int32), np.asarray(xpos, np.int32)
    n, L = y.shape
    if not (1 <= n <= MAX_HYPS and x.shape == y.shape):
        raise ValueError(f"a beam is 1 to {MAX_HYPS} hypotheses of one length")
    if not 0 <= frm <= L:
        raise ValueError(f"from = {frm} is outside [0, {L}]")
    s = np.asarray(score, np.float64).reshape(n)
    agree = agree_lengths(y)
    w, status = beam_weights(s)
    return {"L": L, "commit": L if final else int(agree.min()), "n_hyp": n, "status": status, "agree": agree,
            "tokens": y[0, frm:].copy(), "xpos": x[0, frm:].copy(), "stability": stability_of(agree, w, frm, L, final),
            "score": float(s[0]), "score_dec": float(s[0] if score_dec is None else np.asarray(score_dec, np.float64)[0]),
            "score_ctc": float(s[0] if score_ctc is None else np.asarray(score_ctc, np.float64)[0])}


def of_hypotheses(hyps: Sequence[dict], frm: int = 0, final: bool = False) -> dict:
    """``hyp_commit`` over hypothesis dicts (yseq, xpos, score, score_dec, score_ctc), best first; [] gives empty_delta()"""
    if not hyps:
        if frm:
            raise ValueError(f"from = {frm} is outside [0, 0]")
        return empty_delta()
    return hyp_commit([h["yseq"] for h in hyps], [h["xpos"] for h in hyps], [h["score"] for h in hyps], frm, final,
                      [h["score_dec"] for h in hyps], [h["score_ctc"] for h in hyps])


class StablePrefix:
    """The committed tokens of one stream's utterance, grown from the replies' deltas.

        sp = StablePrefix()
        d = batch.hyps_delta([s], [sp.next_from])[s]      # only what is not held yet travels
        sp.update(d)                                      # raises if the reply contradicts what is held
        sp.tokens, sp.tail, sp.stability                  # committed | still open, with the open tokens' stability

    ``update(d, final=True)`` (or ``reset()``) starts over for the next utterance after handing out the last state."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.tokens: List[int] = []      # committed token ids (the <sos> first), final
        self.xpos: List[int] = []
        self.tail: List[int] = []        # the best hypothesis behind them, open
        self.tail_xpos: List[int] = []
        self.stability: List[float] = []  # one value per open token
        self.L = 0
        self.fresh = True                # nothing held: the next reply starts an utterance

    @property
    def next_from(self) -> int:
        return len(self.tokens)

    @property
    def committed(self) -> int:
        return len(self.tokens)

    def update(self, d: dict, final: bool = False, frm: Optional[int] = None) -> "StablePrefix":
        """take the delta asked for with ``from = next_from`` (``frm``: what was asked, when not that)"""
        frm = self.next_from if frm is None else int(frm)
        L, commit = int(d["L"]), int(d["commit"])
        tok, xp = [int(t) for t in d["tokens"]], [int(t) for t in d["xpos"]]
        stab = [float(v) for v in d["stability"]]
        if frm > len(self.tokens):
            raise ValueError(f"the delta starts at {frm}, behind the {len(self.tokens)} tokens held")
        if L == 0 and frm == 0 and not tok:   # the stream has not started
            if self.tokens:
                raise ValueError("the reply has no hypotheses but tokens are held")
            self.tail, self.tail_xpos, self.stability, self.L = [], [], [], 0
            return self
        if len(tok) != L - frm or len(xp) != len(tok) or len(stab) != len(tok):
            raise ValueError(f"a delta from {frm} of {L} tokens has {len(tok)}")
        if commit < len(self.tokens) or commit > L:
            raise ValueError(f"the committed length went from {len(self.tokens)} to {commit} (L = {L})")
        over = len(self.tokens) - frm    # tokens of the delta that are held already: they must be the same
        if tok[:over] != self.tokens[frm:] or xp[:over] != self.xpos[frm:]:
            raise ValueError("the reply contradicts the committed tokens")
        new = commit - len(self.tokens)
        if any(v != 1.0 for v in stab[over:over + new]):
            raise ValueError("a committed token has a stability below 1")
        self.tokens += tok[over:over + new]
        self.xpos += xp[over:over + new]
        self.tail, self.tail_xpos, self.stability = tok[over + new:], xp[over + new:], stab[over + new:]
        self.L = L
        self.fresh = False
        if final:
            done = StablePrefix()
            done.__dict__.update(self.__dict__)
            self.reset()
            return done
        return self

    def state(self) -> dict:
        return {"committed": len(self.tokens), "tokens": list(self.tokens) + list(self.tail),
                "stability": list(self.stability)}

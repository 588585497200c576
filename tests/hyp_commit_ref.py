"""The numpy contract of the stable-partial read-back (sc_hyp_commit, csrc/commit.hip), float64 / int32.

A stream's live beam is n hypotheses of one length L, best first.  Every hypothesis of a later reply descends from one
of them, so the prefix all of them share - the committed prefix - cannot change any more.

  agree[h]      length of the common prefix of yseq[h] and yseq[0] (agree[0] = L)
  commit        min_h agree[h]; L with `final` set (the first hypothesis is the result and the utterance is over)
  w[h]          exp(score[h] - the largest finite score); a non-finite score: weight 0 and status bit NONFINITE; no finite
                score at all: every weight 1
  Z             ((w[0] + w[1]) + ...) in ascending h
  stability[i]  for i in [frm, L): the sum, in ascending h, of the w[h] with agree[h] > i, divided by Z - the share of the
                beam's mass that agrees with the best hypothesis up to and including token i; 1.0 with `final` set
  tail          yseq[0, frm:L], xpos[0, frm:L]; totals: the three scores of hypothesis 0

stability[i] == 1.0 bit for bit for i < commit (the numerator is the sum that gives Z), and stability never rises with
i (the sets are nested, the terms are not negative, rounding is monotone)."""
import numpy as np

NONFINITE = 1            # status bit: a score of the beam is a NaN or an infinity
MAX_HYPS = 16


def agree_lengths(yseq):
    y = np.asarray(yseq, np.int32)
    n, L = y.shape
    out = np.full(n, L, np.int32)
    for h in range(n):
        bad = np.nonzero(y[h] != y[0])[0]
        if bad.size:
            out[h] = bad[0]
    return out


def weights(score):
    """(w [n] float64, status)"""
    s = np.asarray(score, np.float64)
    fin = np.isfinite(s)
    status = 0 if fin.all() else NONFINITE
    if not fin.any():
        return np.ones(s.shape[0], np.float64), status
    m = s[fin].max()
    w = np.zeros(s.shape[0], np.float64)
    for h in range(s.shape[0]):
        if fin[h]:
            w[h] = np.exp(s[h] - m)
    return w, status


def stability_of(agree, w, frm, L, final=False):
    out = np.ones(max(L - frm, 0), np.float64)
    if final:
        return out
    z = np.float64(0.0)
    for h in range(len(w)):
        z = z + w[h]
    for i in range(frm, L):
        a = np.float64(0.0)
        for h in range(len(w)):
            if agree[h] > i:
                a = a + w[h]
        out[i - frm] = a / z
    return out


def hyp_commit(yseq, xpos, score, frm=0, final=False, score_dec=None, score_ctc=None):
    """yseq / xpos [n, L] int32, score [n] (score_dec / score_ctc [n]: only hypothesis 0's are passed on) ->
    {"L", "commit", "n_hyp", "status", "agree" [n], "tokens" / "xpos" [L - frm] int32, "stability" [L - frm] float64,
    "score", "score_dec", "score_ctc"}"""
    y = np.asarray(yseq, np.int32)
    x = np.asarray(xpos, np.int32)
    n, L = y.shape
    assert 1 <= n <= MAX_HYPS and x.shape == y.shape and 0 <= frm <= L
    s = np.asarray(score, np.float64).reshape(n)
    agree = agree_lengths(y)
    commit = L if final else int(agree.min())
    w, status = weights(s)
    return {"L": L, "commit": commit, "n_hyp": n, "status": status, "agree": agree,
            "tokens": y[0, frm:].copy(), "xpos": x[0, frm:].copy(),
            "stability": stability_of(agree, w, frm, L, final),
            "score": float(s[0]), "score_dec": float(s[0] if score_dec is None else np.asarray(score_dec, np.float64)[0]),
            "score_ctc": float(s[0] if score_ctc is None else np.asarray(score_ctc, np.float64)[0])}


def of_hypotheses(hyps, frm=0, final=False):
    """the contract over a list of hypothesis dicts (yseq, xpos, score, score_dec, score_ctc), best first; an empty list
    (a stream that has not started): L = commit = n_hyp = 0"""
    if not hyps:
        assert frm == 0
        return {"L": 0, "commit": 0, "n_hyp": 0, "status": 0, "agree": np.zeros(0, np.int32),
                "tokens": np.zeros(0, np.int32), "xpos": np.zeros(0, np.int32), "stability": np.zeros(0),
                "score": 0.0, "score_dec": 0.0, "score_ctc": 0.0}
    return hyp_commit([h["yseq"] for h in hyps], [h["xpos"] for h in hyps], [h["score"] for h in hyps], frm, final,
                      [h["score_dec"] for h in hyps], [h["score_ctc"] for h in hyps])

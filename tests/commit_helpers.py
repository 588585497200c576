"""Shared by the stable-partial tests: the engines they run (synthetic models of draft_helpers, a chosen beam, block-boundary
detection on or off), constructed beams, and the checks every reply of a run has to pass."""
import numpy as np

import draft_helpers
import hyp_commit_ref as R
from speechcatcher_amd import commit, synth
from speechcatcher_amd.config import SearchConfig

CHUNK, N_CHUNKS = 10240, 8
SEEDS = (5, 6)                        # audio of stream 0 / stream 1
# (model, beam, block-boundary detection)
RUNS = [(m, w, bbd) for m in ("plain", "mixed") for w in (3, 10) for bbd in (False, True)]
STAB_TOL = 1e-12                      # device stability against the contract: two exponentials of <= 1 ulp each, at most
                                      # 16 ascending adds, one correctly rounded divide - a few 1e-14; the bar is ~50 x that


def make_batch(model, cfg_name, backend, n_streams, beam, use_bbd, device="cpu", weights=None, **kw):
    """backend: "native" = the C++ engine, else a backend object for the Python engine"""
    w = weights if weights is not None else draft_helpers.packed_weights(model, cfg_name, device)
    sc = SearchConfig(beam_size=beam, use_bbd=use_bbd)
    if isinstance(backend, str) and backend == "native":
        from speechcatcher_amd.native import NativeStreamBatch
        return NativeStreamBatch(w, n_streams, sc, **kw)
    from speechcatcher_amd.engine import StreamBatch
    return StreamBatch(w, backend, n_streams, sc, **kw)


def audio(seed, n_chunks=N_CHUNKS):
    return synth.synth_audio(seed, CHUNK * n_chunks)


def beam(rng, n, L, mismatch, vocab=50):
    """yseq / xpos [n, L]: row 0 random; row h > 0 differs from it first at mismatch[h - 1] (None: nowhere), and wherever
    else it likes behind that"""
    y = np.tile(rng.integers(2, vocab, size=L, dtype=np.int32), (n, 1))
    x = np.tile(np.cumsum(rng.integers(0, 3, size=L)).astype(np.int32), (n, 1))
    for h in range(1, n):
        m = mismatch[(h - 1) % len(mismatch)]
        if m is None or m >= L:
            continue
        y[h, m] = y[0, m] + 1 + h
        if m + 1 < L:
            tail = rng.integers(2, vocab, size=L - m - 1, dtype=np.int32)
            y[h, m + 1:] = np.where(rng.random(L - m - 1) < 0.5, tail, y[h, m + 1:])
            x[h, m + 1:] += 1
    return y, x


def same_ints(got, want):
    """every int32 of a delta equals the contract's"""
    for k in ("L", "commit"):
        assert int(got[k]) == int(want[k]), (k, got[k], want[k])
    for k in ("n_hyp", "status"):
        if k in got:
            assert int(got[k]) == int(want[k]), (k, got[k], want[k])
    for k in ("tokens", "xpos"):
        assert np.asarray(got[k], np.int32).tolist() == np.asarray(want[k], np.int32).tolist(), k
    if "agree" in got:
        assert np.asarray(got["agree"]).tolist() == np.asarray(want["agree"]).tolist()


def same_delta(got, want, tol=0.0):
    """ints equal, the three totals bit-identical, stability within tol (0: equal)"""
    same_ints(got, want)
    for k in ("score", "score_dec", "score_ctc"):
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])
    a, b = np.asarray(got["stability"], np.float64), np.asarray(want["stability"], np.float64)
    assert a.shape == b.shape
    err = float(np.abs(a - b).max(initial=0.0))
    assert err <= tol, err
    return err


def exact_properties(d, frm):
    """the two properties the summation order gives, asserted exactly: 1.0 bit for bit below commit, never rising"""
    st = np.asarray(d["stability"], np.float64)
    k = max(0, int(d["commit"]) - frm)
    assert (st[:k] == 1.0).all()
    assert (np.diff(st) <= 0.0).all()
    assert ((st >= 0.0) & (st <= 1.0)).all()


class Follower:
    """what a client of one stream does with the replies of an utterance, and the invariants of the committed prefix"""

    def __init__(self):
        self.sp = commit.StablePrefix()
        self.prev = None              # (commit, best yseq, best xpos) of the previous reply
        self.trace = []               # (L, commit) per reply of the utterance

    @property
    def frm(self):
        return self.sp.next_from

    def reply(self, delta, hyps, final=False):
        """delta: what hyps_delta gave for from = self.frm; hyps: the hypotheses of the same reply"""
        frm = self.frm
        held = list(self.sp.tokens), list(self.sp.xpos)
        if hyps:
            assert held[0] + [int(t) for t in delta["tokens"]] == hyps[0]["yseq"]          # held + tail = the best hypothesis
            assert held[1] + [int(t) for t in delta["xpos"]] == hyps[0]["xpos"]
        if self.prev is not None:
            c, y, x = self.prev
            assert delta["commit"] >= c                                                    # never shrinks
            for h in hyps:                                                                 # every hypothesis keeps it
                assert h["yseq"][:c] == y[:c] and h["xpos"][:c] == x[:c]
        exact_properties(delta, frm)
        done = self.sp.update(delta, final=final)                                          # raises on a contradiction
        self.trace.append((int(delta["L"]), int(delta["commit"])))
        if final:
            assert done.committed == delta["L"] == delta["commit"] and done.tail == []
            self.prev = None
        elif hyps:
            self.prev = (int(delta["commit"]), hyps[0]["yseq"], hyps[0]["xpos"])
        return done


def non_vacuous(trace):
    """at least three replies with 1 < commit < L, and commit grows between them"""
    mid = [c for (L, c) in trace if 1 < c < L]
    return len(mid) >= 3 and len(set(mid)) >= 3 and mid == sorted(mid)

"""Stable partials on the CPU: the numpy contract (tests/hyp_commit_ref.py) and its exact properties on constructed beams,
the host-side form (speechcatcher_amd.commit) and StablePrefix against it, and the Python lock-step engine on the spec
backend - the committed prefix never shrinks and every later hypothesis keeps it."""
import ctypes
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import hyp_commit_ref as R
from commit_helpers import CHUNK, N_CHUNKS, RUNS, SEEDS, Follower, audio, beam, exact_properties, make_batch, non_vacuous, \
    same_delta
from speechcatcher_amd import _abi, commit

ROOT = pathlib.Path(__file__).resolve().parents[1]


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_are_at_abi_12_with_both_entry_points():
    hdr = (ROOT / "include" / "scasr.h").read_text()
    assert int(re.search(r"#define SC_ABI_VERSION (\d+)", hdr).group(1)) == _abi.ABI_VERSION == 12
    for name, val in (("SC_COMMIT_MAX_HYPS", _abi.COMMIT_MAX_HYPS), ("SC_COMMIT_FINAL", _abi.COMMIT_FINAL),
                      ("SC_COMMIT_NONFINITE", _abi.COMMIT_NONFINITE), ("SC_COMMIT_MAX_JOBS", _abi.COMMIT_MAX_JOBS)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == val
    assert (R.MAX_HYPS, R.NONFINITE) == (commit.MAX_HYPS, commit.NONFINITE) == (_abi.COMMIT_MAX_HYPS, _abi.COMMIT_NONFINITE)
    assert "sc_hyp_commit" in _abi.EXPORTED_SYMBOLS and "sc_get_hyps_delta" in _abi.EXPORTED_SYMBOLS
    assert re.search(r"int sc_hyp_commit\(const sc_hyp_commit_job \*jobs, int n_jobs, void \*stream\);", hdr)
    assert "int sc_get_hyps_delta(sc_streams *streams, const int *stream_ids, int n, const int *from, const int *final," in hdr


def test_job_struct_layout_matches_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    cls = _abi.CommitJob
    c_name = {"frm": "from"}                                          # (a Python keyword)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "scasr.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(sc_hyp_commit_job));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(sc_hyp_commit_job, {c_name.get(fname, fname)}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls) == 120
    assert len(out) == len(cls._fields_) + 1 == 18
    for fname, _ in cls._fields_:
        assert int(out[fname]) == getattr(cls, fname).offset, fname


# ---- the contract on constructed beams ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 10, 16])
@pytest.mark.parametrize("where", ["first", "last", "nowhere", "spread"])
def test_contract_on_constructed_beams(n, where):
    rng = np.random.default_rng(100 * n + len(where))
    L = 37
    mism = {"first": [0], "last": [L - 1], "nowhere": [None], "spread": [20, 9, None, 30, 9]}[where]
    y, x = beam(rng, n, L, mism)
    score = -np.sort(rng.random(n) * 6.0)
    want_commit = min([L] + [m for m in (mism * 16)[:n - 1] if m is not None])
    base = R.hyp_commit(y, x, score)
    assert base["commit"] == want_commit and base["agree"][0] == L and base["status"] == 0
    for final in (False, True):
        for frm in sorted({0, want_commit, L}):
            d = R.hyp_commit(y, x, score, frm, final, score - 1.0, score + 1.0)
            assert d["L"] == L and d["n_hyp"] == n and d["commit"] == (L if final else want_commit)
            assert d["agree"].tolist() == base["agree"].tolist()
            assert d["tokens"].tolist() == y[0, frm:].tolist() and d["xpos"].tolist() == x[0, frm:].tolist()
            assert (d["score"], d["score_dec"], d["score_ctc"]) == (score[0], score[0] - 1.0, score[0] + 1.0)
            assert d["stability"].shape == (L - frm,)
            exact_properties(d, frm)
            if final:
                assert (d["stability"] == 1.0).all()
            else:
                assert d["stability"].tobytes() == base["stability"][frm:].tobytes()
            same_delta(commit.hyp_commit(y, x, score, frm, final, score - 1.0, score + 1.0), d)   # the host-side form
    # stability by hand: the mass of the hypotheses that still agree
    w = np.exp(score - score.max())
    for i in (0, L // 2, L - 1):
        assert abs(base["stability"][i] - w[base["agree"] > i].sum() / w.sum()) < 1e-15
    if where == "first" and n > 1:
        assert base["stability"][0] < 1.0 and base["stability"][0] == base["stability"][-1]    # only the best agrees with itself


def test_identical_rows_agree_over_the_whole_length():
    y = np.tile(np.arange(9, dtype=np.int32), (4, 1))
    d = R.hyp_commit(y, y, [-1.0, -2.0, -3.0, -4.0])
    assert d["agree"].tolist() == [9] * 4 and d["commit"] == 9 and (d["stability"] == 1.0).all()
    d = R.hyp_commit(y[:, :0], y[:, :0], [0.0] * 4)                # L = 0: nothing to agree on, nothing written
    assert d["L"] == d["commit"] == 0 and d["stability"].shape == (0,)


@pytest.mark.parametrize("bad", ["+inf", "-inf", "nan", "all -inf", "all nan"])
def test_non_finite_scores_weigh_nothing_and_set_the_status_bit(bad):
    rng = np.random.default_rng(7)
    y, x = beam(rng, 4, 12, [3, 8, None])
    s = np.asarray([-1.0, -1.5, -2.0, -2.5])
    if bad.startswith("all"):
        s[:] = -np.inf if bad == "all -inf" else np.nan
    else:
        s[1] = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}[bad]
    d = R.hyp_commit(y, x, s)
    assert d["status"] == R.NONFINITE == commit.NONFINITE == _abi.COMMIT_NONFINITE
    assert d["agree"].tolist() == [12, 3, 8, 12] and d["commit"] == 3
    w, _ = R.weights(s)
    if bad.startswith("all"):
        assert w.tolist() == [1.0] * 4                              # the mass is shared evenly
        assert d["stability"][3] == 0.75 and d["stability"][8] == 0.5
    else:
        assert w[1] == 0.0 and w[0] == 1.0 and np.isfinite(w).all()
        assert (d["stability"][:8] == 1.0).all()                    # hypothesis 1 weighs nothing: leaving costs nothing
        assert d["stability"][8] < 1.0
    exact_properties(d, 0)
    same_delta(commit.hyp_commit(y, x, s), d)
    assert np.isfinite(d["stability"]).all()


def test_random_beams_keep_the_exact_properties():
    rng = np.random.default_rng(3)
    for _ in range(200):
        n, L = int(rng.integers(1, 17)), int(rng.integers(1, 80))
        y, x = beam(rng, n, L, [int(rng.integers(0, L + 5)) for _ in range(5)])
        s = -np.sort(rng.random(n) * float(rng.choice([0.1, 5.0, 60.0, 800.0])))
        frm = int(rng.integers(0, L + 1))
        d = R.hyp_commit(y, x, s, frm)
        exact_properties(d, frm)
        same_delta(commit.hyp_commit(y, x, s, frm), d)
        for h in range(n):
            a = int(d["agree"][h])
            assert (y[h, :a] == y[0, :a]).all() and (a == L or y[h, a] != y[0, a])


def test_arguments_outside_the_contract_are_refused():
    y = np.zeros((2, 5), np.int32)
    for fn in (commit.hyp_commit,):
        with pytest.raises(ValueError):
            fn(y, y, [0.0, 0.0], 6)
        with pytest.raises(ValueError):
            fn(np.zeros((17, 5), np.int32), np.zeros((17, 5), np.int32), np.zeros(17))
    assert commit.of_hypotheses([])["L"] == 0 and R.of_hypotheses([])["n_hyp"] == 0
    with pytest.raises(ValueError):
        commit.of_hypotheses([], 1)


# ---- StablePrefix ------------------------------------------------------------------------------------------------------
def _delta(y, x, frm, commit_len, stab=None):
    L = len(y)
    st = np.ones(L - frm) if stab is None else np.asarray(stab, np.float64)
    if stab is None:
        st[max(0, commit_len - frm):] = 0.5
    return {"L": L, "commit": commit_len, "tokens": np.asarray(y[frm:], np.int32), "xpos": np.asarray(x[frm:], np.int32),
            "stability": st}


def test_stable_prefix_grows_and_refuses_contradictions():
    sp = commit.StablePrefix()
    assert sp.next_from == 0 and sp.fresh
    sp.update(commit.empty_delta())                                  # a stream that has not started
    assert sp.fresh and sp.state() == {"committed": 0, "tokens": [], "stability": []}
    y, x = [60, 5, 6, 7, 8], [0, 2, 4, 6, 8]
    sp.update(_delta(y[:3], x[:3], 0, 1))
    assert sp.tokens == [60] and sp.tail == [5, 6] and sp.stability == [0.5, 0.5] and sp.next_from == 1
    sp.update(_delta(y, x, 1, 3))
    assert sp.tokens == [60, 5, 6] and sp.xpos == [0, 2, 4] and sp.tail == [7, 8] and sp.L == 5
    assert sp.state() == {"committed": 3, "tokens": y, "stability": [0.5, 0.5]}
    sp.update(_delta(y, x, 0, 3), frm=0)                             # a delta that overlaps what is held: the same tokens
    assert sp.tokens == [60, 5, 6] and sp.tail == [7, 8]
    for bad in (_delta(y, x, 3, 2),                                  # the committed length shrank
                _delta([60, 5, 9, 7], x[:4], 0, 3),                  # a held token changed
                _delta(y, [0, 2, 5, 6, 8], 0, 3),                    # a held position changed
                _delta(y, x, 3, 4, [0.9, 0.5]),                      # committed with a stability below 1
                dict(_delta(y, x, 3, 4), tokens=np.asarray([7], np.int32)),   # a tail of the wrong length
                _delta(y, x, 3, 6)):                                 # committed beyond L
        with pytest.raises(ValueError):
            sp.update(bad, frm=0 if len(bad["tokens"]) == len(bad["xpos"]) == bad["L"] else None)
        assert sp.tokens == [60, 5, 6] and sp.tail == [7, 8]         # a refused reply changes nothing
    with pytest.raises(ValueError):
        sp.update(_delta(y, x, 4, 4), frm=4)                         # a gap behind what is held
    with pytest.raises(ValueError):
        sp.update(commit.empty_delta())                              # no hypotheses, but tokens are held
    done = sp.update(_delta(y, x, 3, 5), final=True)
    assert done.tokens == y and done.tail == [] and done.committed == 5
    assert sp.fresh and sp.next_from == 0 and sp.tokens == []        # the next utterance starts over
    sp.update(_delta(y[:2], x[:2], 0, 2))
    sp.reset()
    assert sp.fresh and sp.state()["committed"] == 0


# ---- the Python engine on the spec backend -----------------------------------------------------------------------------
def _spec_batch(model, beam_size, bbd, n_streams=2):
    from oracle.kernel_spec import SpecBackend
    return make_batch(model, "TINY", SpecBackend(), n_streams, beam_size, bbd, max_frames=400, max_tokens=300,
                      pcm_capacity=1 << 18)


@pytest.fixture(scope="module", params=RUNS, ids=lambda r: f"{r[0]}-beam{r[1]}-{'bbd' if r[2] else 'nobbd'}")
def spec_run(request):
    """two streams over 8 chunks (the last one final); stream 1 is reset after chunk 3 and fed its audio again from the
    start (its utterance then ends unfinished).  Every reply goes through a Follower; returns the traces."""
    model, w, bbd = request.param
    sb = _spec_batch(model, w, bbd)
    assert not hasattr(sb.be, "hyp_commit")                          # the spec backend: the numpy route
    pcm = [audio(s) for s in SEEDS]
    fol = [Follower(), Follower()]
    traces = {0: [], 1: [], "1 before reset": None}
    pos = [0, 0]
    for k in range(N_CHUNKS):
        if k == 4:
            traces["1 before reset"] = list(fol[1].trace)
            sb.reset(1)
            fol[1] = Follower()
            pos[1] = 0
        fin = k == N_CHUNKS - 1
        sb.push([(s, pcm[s][pos[s] * CHUNK:(pos[s] + 1) * CHUNK], fin and s == 0) for s in (0, 1)])
        pos = [p + 1 for p in pos]
        before = [sb.hypotheses(s) for s in (0, 1)]
        frm = [f.frm for f in fol]
        got = sb.hyps_delta([0, 1], frm, final=[0] if fin else [])
        assert [sb.hypotheses(s) for s in (0, 1)] == before          # the call changes nothing
        for s in (0, 1):
            want = R.of_hypotheses(before[s], frm[s], fin and s == 0)
            same_delta(got[s], want)                                 # the same numpy arithmetic: equal
            assert sorted(got[s]) == sorted(commit.FIELDS + ("n_hyp", "status"))
            whole = sb.hyps_delta([s], [0], final=[s] if fin and s == 0 else [])[s]      # ... and from 0: the whole best one
            same_delta(whole, R.of_hypotheses(before[s], 0, fin and s == 0))
            fol[s].reply(got[s], before[s], fin and s == 0)
    traces[0], traces[1] = fol[0].trace, fol[1].trace
    return {"param": request.param, "traces": traces}


def test_spec_engine_deltas_follow_the_contract_and_the_prefix_is_final(spec_run):
    (model, w, bbd), tr = spec_run["param"], spec_run["traces"]
    assert len(tr[0]) == N_CHUNKS and len(tr[1]) == N_CHUNKS - 4 and len(tr["1 before reset"]) == 4
    assert tr[0][-1][0] == tr[0][-1][1] > 1                           # the final commits everything
    assert tr[1][:4] == tr["1 before reset"]                          # the same audio after the reset: the same replies
    for t in (tr[0][:-1], tr[1]):
        assert all(c <= L for L, c in t) and [c for _, c in t] == sorted(c for _, c in t)
    if not bbd:
        assert non_vacuous(tr[0][:-1]), tr[0]                          # at least three replies with 1 < commit < L, growing
    if bbd and w == 10:
        stuck = [c for L, c in tr[0][:-1] if L > 2]
        assert stuck.count(1) >= 3, tr[0]                              # the stuck case: the beam keeps a rival from token 1 on


def test_engine_refuses_what_the_native_call_refuses():
    from speechcatcher_amd.engine import EngineError
    sb = _spec_batch("plain", 3, False)
    assert sb.hyps_delta([0, 1], [0, 0])[1]["L"] == 0                  # streams that have not started
    sb.push([(0, audio(5)[:CHUNK], False)])
    L = sb.hyps_delta([0], [0])[0]["L"]
    assert L >= 1
    for streams, frm in (([0], [L + 1]), ([0, 0], [0, 0]), ([1], [1]), ([0], [0, 0]), ([0], [-1])):
        with pytest.raises(EngineError):
            sb.hyps_delta(streams, frm)
    assert sb.hyps_delta([0], [L])[0]["tokens"].shape == (0,)

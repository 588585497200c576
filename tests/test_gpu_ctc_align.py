"""CTC forced alignment on the GPU (csrc/align.hip, sc_align_hyps / sc_align_tokens) against the float32 spec of
tests/ctc_align_ref.py: the kernel in lock-step, the stream level on the exact CTC rows the kernel saw, alignment
interleaved with continuous batching (no effect on decoding), and the public surfaces."""
import numpy as np
import pytest
import torch

import ctc_align_ref as ref
from speechcatcher_amd import synth

pytestmark = pytest.mark.gpu


def _check_job(got, k, e, y, blank):
    start, end, lp, ps, st = got
    want = ref.align(e, y, blank)
    assert st[k] == want["status"], (k, st[k], want["status"])
    if want["status"] != ref.OK:
        assert np.isneginf(ps[k])
        return
    L = len(y)
    np.testing.assert_array_equal(start[k, :L], want["start"])
    np.testing.assert_array_equal(end[k, :L], want["end"])
    assert ps[k].tobytes() == np.float32(want["path_score"]).tobytes(), (k, ps[k], want["path_score"])
    np.testing.assert_allclose(lp[k, :L], want["logp_mean"], atol=1e-5, rtol=0)


def test_kernel_lockstep_ragged_and_adversarial():
    from speechcatcher_amd.hip_backend import HipBackend
    be = HipBackend("cuda:0", use_graphs=False)
    rng = np.random.default_rng(7)
    jobs = []   # (table [T, V] fp32, labels, blank)

    def rand_labels(L, V, blank, rep_every=0):
        y = rng.integers(0, V - 1, L)
        y[y >= blank] += 1
        if rep_every:
            for i in range(rep_every, L, rep_every):
                y[i] = y[i - 1]
        return y.astype(np.int32)

    for T, L, V in [(1, 0, 64), (1, 1, 64), (7, 2, 64), (7, 1, 1024), (430, 50, 1024), (430, 400, 5000),
                    (1500, 400, 1024), (4800, 1023, 1024), (1500, 0, 5000), (7, 0, 1024), (4800, 50, 64)]:
        if 2 * L + 1 > 2 * 1023 + 1 or T < L:
            continue
        blank = int(rng.integers(0, V)) if V == 64 else 0
        e = (rng.standard_normal((T, V)) * 4).astype(np.float32)
        if T > 100:
            e[:T // 2] -= np.log(np.exp(e[:T // 2].astype(np.float64)).sum(1, keepdims=True)).astype(np.float32)
        jobs.append((e, rand_labels(L, V, blank), blank))
    # adversarial: long runs of repeats at the minimum feasible T, one frame short of it, a constant table (all ties)
    y = np.array([5] * 40 + [6, 6, 7] * 20, np.int32)
    reps = int(np.sum(y[1:] == y[:-1]))
    for T in (len(y) + reps, len(y) + reps - 1, len(y) + reps + 3):
        jobs.append(((rng.standard_normal((T, 64)) * 2).astype(np.float32), y, 0))
    jobs.append((np.full((300, 128), -3.0, np.float32), rand_labels(100, 128, 0), 0))
    jobs.append((np.zeros((64, 64), np.float32), np.array([1, 1, 1, 2], np.int32), 0))
    # integer-valued table: exact sums, many ties between distinct paths
    jobs.append((rng.integers(-3, 1, (200, 32)).astype(np.float32), rand_labels(60, 32, 0, rep_every=4), 0))
    bad = (rng.standard_normal((50, 64))).astype(np.float32)
    bad[17, 9] = np.nan
    jobs.append((bad, rand_labels(10, 64, 0), 0))
    jobs.append((rng.standard_normal((50, 64)).astype(np.float32), np.array([3, 0, 4], np.int32), 0))   # blank label
    # a strided view: rows of a wider table
    wide = (rng.standard_normal((300, 200)) * 3).astype(np.float32)
    dev = []
    for e, y, blank in jobs:
        dev.append((torch.from_numpy(e).cuda(), torch.from_numpy(np.ascontiguousarray(y, np.int32)).cuda(), blank))
    wide_d = torch.from_numpy(wide).cuda()
    dev.append((wide_d[:, 20:148], torch.from_numpy(rand_labels(90, 128, 0)).cuda(), 0))
    jobs.append((wide[:, 20:148].copy(), dev[-1][1].cpu().numpy(), 0))
    before = [t[0].clone() for t in dev]
    got = be.ctc_align(dev)
    for k, (e, y, blank) in enumerate(jobs):
        _check_job(got, k, e, y, blank)
    for a, b in zip(before, dev):            # the table is only read (bytes: one table holds a NaN on purpose)
        assert a.cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()
    assert got[4][-3] == ref.NONFINITE and got[4][-2] == ref.BAD_INPUT


def test_kernel_lockstep_every_states_per_lane_form():
    """one launch per label-length bucket, so that every form of the kernel (NPL = 2, 4, 8, 16, 32 states per lane: the
    launch's longest label sequence picks it) is held to the spec - the backtrace tile is widest at NPL 2"""
    from speechcatcher_amd.hip_backend import HipBackend
    be = HipBackend("cuda:0", use_graphs=False)
    rng = np.random.default_rng(11)
    for Ls in ((1, 20, 63), (64, 100, 127), (128, 200, 255), (256, 400, 511), (512, 1023)):
        jobs = []
        for L in Ls:
            V = 1024
            y = rng.integers(1, V, L).astype(np.int32)
            y[1::7] = y[0::7][:len(y[1::7])]          # some repeats
            reps = int(np.sum(y[1:] == y[:-1]))
            for T in (L + reps, L + reps + 37, 2 * L + 200):
                e = (rng.standard_normal((T, V)) * 4).astype(np.float32)
                jobs.append((e, y, 0))
        dev = [(torch.from_numpy(e).cuda(), torch.from_numpy(y).cuda(), b) for e, y, b in jobs]
        got = be.ctc_align(dev)
        for k, (e, y, blank) in enumerate(jobs):
            _check_job(got, k, e, y, blank)


def _xl_or_tiny_case(name):
    from test_engine_spec import run_case
    sb, js, _ = run_case(name, backend="native", score_tol=1e-3)
    return sb


def _check_stream(sb, s, nbest=None):
    a = sb.align([s], nbest)
    hy = sb.hypotheses(s)
    tab = sb.read_ctc(s)
    T = tab.shape[0]
    eos = sb.cfg.eos_id
    assert a["n_hyps"][0] == len(hy[:a["start"].shape[1]])
    for h in range(int(a["n_hyps"][0])):
        y = hy[h]["yseq"][1:]
        if y and y[-1] == eos:
            y = y[:-1]
        want = ref.align(tab, y, sb.cfg.blank_id)
        assert a["status"][0, h] == want["status"]
        if want["status"] != ref.OK:
            continue
        L = len(y)
        st, en = a["start"][0, h, :L], a["end"][0, h, :L]
        np.testing.assert_array_equal(st, want["start"])
        np.testing.assert_array_equal(en, want["end"])
        assert np.float32(a["path_score"][0, h]).tobytes() == want["path_score"].tobytes()
        np.testing.assert_allclose(a["logp_mean"][0, h, :L], want["logp_mean"], atol=1e-5, rtol=1e-5)
        assert np.all(st < en) and np.all(en[:-1] <= st[1:]) and (L == 0 or (st[0] >= 0 and en[-1] <= T))
    return tab


@pytest.mark.parametrize("name", ["tiny_c10240_b10_bbd0", "xl_c10240_b10_bbd1"])
def test_stream_alignment_equals_the_spec(name):
    sb = _xl_or_tiny_case(name)
    tab = _check_stream(sb, 0)
    assert tab.shape[0] > 0
    # a hand-written transcript against the same frames
    V = sb.cfg.vocab_size
    y = [int(v) for v in (np.arange(12) * 37 % (V - 3)) + 2 if v != sb.cfg.blank_id]
    got = sb.align_tokens(0, y)
    want = ref.align(tab, y, sb.cfg.blank_id)
    assert got["status"] == want["status"] == ref.OK
    np.testing.assert_array_equal(got["start"], want["start"])
    np.testing.assert_array_equal(got["end"], want["end"])
    assert np.float32(got["path_score"]).tobytes() == want["path_score"].tobytes()
    np.testing.assert_allclose(got["logp_mean"], want["logp_mean"], atol=1e-5, rtol=1e-5)


def test_alignment_has_no_effect_on_serving():
    """XL streams under continuous batching (sc_submit / sc_poll, queue depth 2) with alignment calls on the answered
    streams between the polls: every reply is bit-identical to the same run without them, and every alignment equals
    the spec on the frames of its snapshot."""
    from test_engine_spec import make_batch
    S, chunk = 128, 10240
    lens = [chunk * (2 + (i * 5) % 3) + (i * 977) % 3000 for i in range(S)]
    audio = [synth.synth_audio(300 + i, n) for i, n in enumerate(lens)]

    def run(with_align):
        sb = make_batch("XL", 1234, "meanstd", 5, True, n_streams=S, backend="native", max_frames=160, max_tokens=200,
                        pcm_capacity=1 << 17)
        sb.set_queue_depth(2)
        pos = [0] * S
        replies, n_checked = {}, 0

        def nxt(s):
            a, e = pos[s], min(pos[s] + chunk, lens[s])
            pos[s] = e
            return (s, audio[s][a:e], e >= lens[s])

        sb.submit([nxt(s) for s in range(S)])
        sb.submit([nxt(s) for s in range(S) if pos[s] < lens[s]])
        while sb.outstanding:
            done = sb.poll(1)
            ids = sorted(done)
            a = sb.hypotheses_arrays(ids)
            for i, s in enumerate(ids):          # per stream: which streams a poll reports together may vary
                replies.setdefault(s, []).append((a["ids"][i].tobytes(), a["lens"][i].tobytes(), a["score"][i].tobytes()))
            if with_align:
                al = sb.align(ids, 1)
                for i, s in enumerate(ids[:6]):
                    if al["n_hyps"][i] == 0:
                        continue
                    tab = sb.read_ctc(s)
                    L = int(a["lens"][i, 0]) - 1
                    y = a["ids"][i, 0, 1:L + 1].tolist()
                    if y and y[-1] == sb.cfg.eos_id:
                        y = y[:-1]
                    want = ref.align(tab, y, sb.cfg.blank_id)
                    assert al["status"][i, 0] == want["status"]
                    if want["status"] == ref.OK:
                        n = len(y)
                        np.testing.assert_array_equal(al["start"][i, 0, :n], want["start"])
                        assert np.float32(al["path_score"][i, 0]).tobytes() == want["path_score"].tobytes()
                        n_checked += 1
            again = [nxt(s) for s in ids if pos[s] < lens[s]]
            if again:
                sb.submit(again)
        return replies, n_checked

    plain, _ = run(False)
    aligned, n_checked = run(True)
    assert n_checked > 0
    assert plain == aligned



def test_speech2text_token_alignment(tmp_path):
    """Speech2TextStreaming.token_alignment(): one entry per result of the last call, same order and token filtering,
    spans in seconds from the model geometry, conf in (0, 1]; the results themselves are unchanged."""
    from conftest import load_case
    from speechcatcher_amd.config import TINY
    from speechcatcher_amd.speech2text_streaming import Speech2TextStreaming
    js, _ = load_case("tiny_c10240_b10_bbd0")
    meta = js["meta"]
    mdir = synth.write_model_dir(tmp_path / "tiny", TINY, seed=meta["seed"], stats_kind=meta["stats"])
    s2t = Speech2TextStreaming(mdir, beam_size=meta["beam"], ctc_weight=0.3, device="cuda", use_bbd=meta["bbd"],
                               max_frames=256, max_tokens=200)
    audio = synth.synth_audio(0, meta["n_samples"])
    pos, res = 0, []
    for call in js["calls"]:
        end = min(pos + 10240, len(audio))
        fin = end >= len(audio)
        res = s2t(audio[pos:end], is_final=fin, finalize_all=fin)
        pos = end
        assert [r[2] for r in res] == [r[2] for r in call["results"]]
    ta = s2t.token_alignment()
    assert len(ta) == len(res) > 0
    dur = len(audio) / TINY.sample_rate
    for r, a in zip(res, ta):
        assert a["token_ids"] == [int(t) for t in r[2]]
        n = len(a["token_ids"])
        assert len(a["start_s"]) == len(a["end_s"]) == len(a["conf"]) == n
        for k in range(n):
            assert 0 <= a["start_s"][k] < a["end_s"][k] <= dur + 0.25
            assert 0 < a["conf"][k] <= 1.0
        assert all(a["end_s"][k] <= a["start_s"][k + 1] + 1e-9 for k in range(n - 1))


def _write_wav(path, samples):
    import wave
    pcm = np.clip(samples * 32767, -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(pcm.tobytes())


def _tiny_s2t(tmp_path):
    from conftest import load_case
    from speechcatcher_amd.config import TINY
    from speechcatcher_amd.speech2text_streaming import Speech2TextStreaming
    meta = load_case("tiny_c10240_b10_bbd0")[0]["meta"]
    mdir = synth.write_model_dir(tmp_path / "tiny", TINY, seed=meta["seed"], stats_kind=meta["stats"])
    s2t = Speech2TextStreaming(mdir, beam_size=5, ctc_weight=0.3, device="cuda", use_bbd=False,
                               max_frames=256, max_tokens=200)
    V = TINY.vocab_size
    s2t.token_list = [("▁" if v % 3 == 0 else "") + f"t{v}" for v in range(V)]
    return s2t


def test_cli_token_alignment(tmp_path):
    """recognize_file with --token-alignment: token_start / token_end / token_conf of the length of tokens next to
    token_timestamps; without the flag the .json is exactly what it was (no new keys, same bytes otherwise)."""
    import json
    from speechcatcher_amd.__main__ import make_parser, recognize_file
    s2t = _tiny_s2t(tmp_path)
    wav = tmp_path / "a.wav"
    _write_wav(wav, synth.synth_audio(21, 16000 * 5 + 1234))
    args = make_parser().parse_args(["--token-alignment", str(wav)])
    recognize_file(s2t, str(wav), output_file=str(tmp_path / "with"), token_alignment=args.token_alignment)
    recognize_file(s2t, str(wav), output_file=str(tmp_path / "without"))
    plain = (tmp_path / "without.json").read_text()
    withal = json.loads((tmp_path / "with.json").read_text())
    n_tok = 0
    for par in withal["paragraphs"]:
        n = len(par["tokens"])
        n_tok += n
        assert len(par["token_start"]) == len(par["token_end"]) == len(par["token_conf"]) == n
        for a, b, c in zip(par["token_start"], par["token_end"], par["token_conf"]):
            assert a is not None and 0 <= a < b <= 5.5 and 0 < c <= 1
        assert par["token_start"] == sorted(par["token_start"])
        for key in ("token_start", "token_end", "token_conf"):
            del par[key]
    assert n_tok > 0
    assert json.loads(plain) == withal
    assert "token_start" not in plain and "token_conf" not in plain


def test_server_vosk_alignment():
    """ServerLoop(vosk_alignment=True): a final Vosk result carries words (tokens merged at the word mark) with aligned
    start < end and conf in (0, 1] - or, where its hypothesis cannot be aligned, the default per-token entries; the
    default run keeps per-token entries with conf 1.0, and the replies are otherwise the same."""
    from test_engine_spec import make_batch
    from speechcatcher_amd.config import TINY
    from speechcatcher_amd.scheduler import StreamScheduler
    from speechcatcher_amd.server_session import ServerLoop
    tokens = [("▁" if v % 3 == 0 else "") + f"t{v}" for v in range(TINY.vocab_size)]
    chunks = [(synth.synth_audio(40 + k, 10240) * 32767).astype(np.int16) for k in range(9)]

    def serve(**kw):
        sb = make_batch("TINY", 1234, "meanstd", 3, True, n_streams=1, backend="native", max_frames=400,
                        max_tokens=300, pcm_capacity=1 << 18)
        loop = ServerLoop(StreamScheduler(sb, tokens, result_format="espnet"), vosk_output_format=True,
                          finalize_update_iters=2, max_partial_iters=5, **kw)
        sid = loop.connect()
        for c in chunks:
            loop.submit(sid, c)
        loop.submit(sid, '{"eof" : 1}')
        reps = []
        while loop.pending():
            for _sid, r in loop.step().items():
                reps.extend(r)
        return reps

    plain, aligned = serve(), serve(vosk_alignment=True)
    assert len(plain) == len(aligned)
    n_final = 0
    for p, a in zip(plain, aligned):
        if not (isinstance(p, dict) and "result" in p):
            assert p == a
            continue
        assert all(w["conf"] == 1.0 for w in p["result"])
        assert a["text"] == p["text"]
        if a == p:         # no alignment (e.g. the eof reply: hypotheses longer than the frames of its block): default entries
            continue
        n_final += 1
        words = a["result"]
        assert words and len(words) <= len(p["result"])
        for w in words:
            assert 0 <= w["start"] < w["end"] and 0 < w["conf"] <= 1 and w["word"]
        assert "".join(w["word"] for w in words) == "".join(w["word"] for w in p["result"]).replace(" ", "")
    assert n_final > 0

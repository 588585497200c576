"""The C++ engine behind the stream-level C ABI (csrc/streams.hip: sc_engine_* / sc_streams_* / sc_push /
sc_get_hyps / sc_reset) against the fixtures of the real reference, the oracle sessions, and a plain C host
program that links libscasr.so - no Python in the decode loop."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_case
from speechcatcher_amd import synth

pytestmark = pytest.mark.gpu

TINY_CASES = [f"tiny_c{c}_b{b}_bbd{d}" for c in (8192, 10240) for b in (1, 10) for d in (0, 1)] + ["tiny_c25600_b10_bbd0"]
XL_CASES = ["xl_c10240_b10_bbd0", "xl_c10240_b10_bbd1", "xl_c25600_b10_bbd0", "xl_c8192_b10_bbd1", "xl_c8192_b5_bbd1",
            "xl_c10240_b1_bbd0"]


@pytest.mark.parametrize("name", TINY_CASES + ["tiny_stats64_b5"])
def test_native_engine_matches_reference_tiny(name):
    from test_engine_spec import run_case
    sb, js, npz = run_case(name, backend="native")
    if npz is not None:
        enc = sb.encoder_buffer(0)
        np.testing.assert_allclose(enc, npz["enc"][:enc.shape[0]], atol=1e-3, rtol=0)


@pytest.mark.parametrize("name", XL_CASES)
def test_native_engine_matches_reference_xl(name):
    from test_engine_spec import run_case
    run_case(name, backend="native", score_tol=1e-3)


@pytest.mark.parametrize("engine", ["native", "python"])
@pytest.mark.parametrize("name", [f"tiny_c10240_b10_bbd{d}_cw{w}" for d in (0, 1) for w in ("00", "05")] +
                         ["xl_c10240_b10_bbd0_cw00", "xl_c10240_b10_bbd0_cw05"])
def test_ctc_weight_fixtures_on_the_gpu(name, engine):
    """Speech2TextStreaming(ctc_weight=...) is part of the surface (speech2text_streaming.py:143-150): fixtures of the
    real reference at 0.5 and at 0.0 - where it builds NO CTC scorer (beam_search.py:925: decoder-only search, no scan,
    score_ctc stays 0; the tiny cases then run into max_length = 500, beam_search.py:701) - on both engines."""
    from test_engine_spec import run_case
    kw = dict(max_tokens=520) if name.startswith("tiny") else {}
    if engine == "native":
        run_case(name, backend="native", score_tol=1e-3, **kw)
    else:
        from speechcatcher_amd.hip_backend import HipBackend
        run_case(name, backend=HipBackend("cuda:0"), device="cuda:0", score_tol=1e-3, **kw)


@pytest.mark.parametrize("engine", ["native", "python"])
@pytest.mark.parametrize("name", [f"tiny_v1182_c10240_b10_bbd{d}" for d in (0, 1)])
def test_vocabulary_1182_fixtures_on_the_gpu(name, engine):
    """The real reference's trajectories of the tiny model at V = 1182 (tools/gen_golden.py --vocab) on both engines:
    V % d != 0 takes the six-launch decoder layers with the generic output GEMM, V > 1024 the LDS sort of the pre-beam."""
    from test_engine_spec import run_case
    if engine == "native":
        sb, _, _ = run_case(name, backend="native", score_tol=1e-3)
        c = sb.take_attn_counters()
        assert c["self_positions"][0] > 0 and c["self_positions"][1] == c["self_positions"][2] == 0, c
    else:
        from speechcatcher_amd.hip_backend import HipBackend
        sb, _, _ = run_case(name, backend=HipBackend("cuda:0"), device="cuda:0", score_tol=1e-3)
        assert sb.ph1 is None
    assert sb.cfg.vocab_size == 1182


def test_native_engine_at_vocabulary_1182_against_the_oracle():
    """The C++ engine at V = 1182 (tiny dims): 3 streams of different audio in one batch, whole utterances, against the
    oracle run on the same box - token ids exact, scores within 1e-3 - and the forced alignment of the reported
    hypotheses (sc_align_hyps) against the float32 spec of tests/ctc_align_ref.py on the CTC rows it aligned against."""
    import helpers
    from oracle.ref_port import RefPortStreaming
    from test_engine_spec import check_against_blocks, make_batch
    from test_gpu_ctc_align import _check_stream
    S, chunk = 3, 10240
    lens = [16000 * 5 + 1234, 16000 * 4 + 77, 16000 * 6 + 3217]
    audio = [synth.synth_audio(40 + i, n) for i, n in enumerate(lens)]
    sb = make_batch("TINY_V1182", 1234, "meanstd", 10, False, n_streams=S, backend="native", max_frames=256,
                    max_tokens=300, pcm_capacity=1 << 18)
    model = helpers.oracle_model("TINY_V1182", 1234, "meanstd")
    oras = [RefPortStreaming(model, beam_size=10, use_bbd=False) for _ in range(S)]
    pos = 0
    while pos < max(lens):
        items = []
        for i in range(S):
            if pos < lens[i]:
                end = min(pos + chunk, lens[i])
                fin = end >= lens[i]
                items.append((i, audio[i][pos:end], fin))
                oras[i](audio[i][pos:end], is_final=fin, finalize_all=fin)
        sb.push(items)
        pos += chunk
    c = sb.take_attn_counters()
    assert c["self_positions"][0] > 0 and c["self_positions"][1] == c["self_positions"][2] == 0, c
    for i, ora in enumerate(oras):
        ref = ora.running_hyps
        blk = {"yseq": [list(h.yseq) for h in ref], "xpos": [list(h.xpos) for h in ref],
               "score": [h.score for h in ref], "score_dec": [h.scores.get("decoder", 0.0) for h in ref],
               "score_ctc": [h.scores.get("ctc", 0.0) for h in ref], "process_idx": ora.process_idx}
        check_against_blocks(sb, i, blk, 1e-3)
        assert len(sb.hypotheses(i)[0]["yseq"]) > 5
    assert any(max(h["yseq"]) > 1023 for i in range(S) for h in sb.hypotheses(i))   # ids past the old vocabulary
    _check_stream(sb, 1)


def test_native_streams_refuse_a_vocabulary_above_the_limit():
    """sc_streams_create refuses V > SC_MAX_VOCAB (the full-vocabulary LDS of sc_fuse_topw) with an error before it
    allocates or launches anything; V = SC_MAX_VOCAB itself is accepted (the kernels run there: tests/test_gpu_ops.py)."""
    import dataclasses

    import test_engine_spec
    from speechcatcher_amd._abi import MAX_VOCAB
    from speechcatcher_amd.config import TINY
    from speechcatcher_amd.engine import EngineError
    from test_engine_spec import make_batch
    for V in (MAX_VOCAB, MAX_VOCAB + 1):
        test_engine_spec.CFGS.setdefault(f"TINY_V{V}", dataclasses.replace(TINY, vocab_size=V))
    kw = dict(backend="native", max_frames=64, max_tokens=32, pcm_capacity=1 << 14)
    with pytest.raises(EngineError, match="SC_MAX_VOCAB"):
        make_batch(f"TINY_V{MAX_VOCAB + 1}", 1234, "meanstd", 5, False, **kw)
    sb = make_batch(f"TINY_V{MAX_VOCAB}", 1234, "meanstd", 5, False, **kw)
    sb.push([(0, synth.synth_audio(5, 12000), True)])
    assert len(sb.hypotheses(0)) > 0


@pytest.mark.parametrize("name", ["tiny_c10240_b10_bbd0", "tiny_c8192_b10_bbd1", "xl_c10240_b10_bbd0"])
def test_native_engine_with_the_t_parallel_ctc_scan(name, monkeypatch):
    """the same fixtures with the CTC prefix scan split over T from 32 frames on (default: 256): every block after
    the first one takes the 16-segment kernel"""
    from test_engine_spec import run_case
    monkeypatch.setenv("SC_SCAN_SPLIT_MIN", "32")
    run_case(name, backend="native", score_tol=1e-3)


def test_native_short_utterances_and_the_reference_exception():
    from test_engine_spec import make_batch, check_against_blocks
    js = json.loads((GOLDEN / "tiny_short.json").read_text())
    for n in (3000, 9000, 20000):
        sb = make_batch("TINY", 1234, "meanstd", 5, False, backend="native", max_frames=128, max_tokens=600,
                        pcm_capacity=1 << 16)
        sb.push([(0, synth.synth_audio(3, n), True)])
        check_against_blocks(sb, 0, js[str(n)]["blocks"][-1])
    sb = make_batch("TINY", 1234, "meanstd", 5, False, backend="native", max_frames=128, max_tokens=64,
                    pcm_capacity=1 << 16)
    with pytest.raises(RuntimeError):           # final chunk with < 7 feature frames: the reference dies in Conv2d (A3)
        sb.push([(0, synth.synth_audio(3, 700), True)])
    assert sb.st[0].T_enc == 0                  # ... and the stream is usable again
    sb.push([(0, synth.synth_audio(3, 9000), True)])
    check_against_blocks(sb, 0, js["9000"]["blocks"][-1])


@pytest.mark.parametrize("chunk", [400, 640, 1000])
def test_native_sub_window_chunks_call_by_call(chunk):
    """the reference's own degenerate inputs on the C++ engine.  BASELINE's metric says "640-sample chunks":
    such a call yields 2 feature frames, the reference skips the encoder and drops the frames (beam_search.py:551-559), every
    non-final call returns one empty hypothesis and the final call dies in Conv2d (speech2text_streaming.py:328-338, 362-383;
    fixture tests/golden/tiny_short.json["640"], tests/golden/frontend.json sizes 400 / 640 / 1000).  Here: a 64 000-sample
    utterance through sc_push in calls of 400 / 640 / 1000 samples - the carried-over waveform length of every call against
    the reference's frontend fixture, and, against the oracle run call by call on the same audio, the number of results of every
    call, the hypotheses (ids exact, scores 1e-3), the encoder calls, and the exception of the final call."""
    import torch
    from helpers import oracle_model
    from oracle.ref_port import RefPortStreaming
    from speechcatcher_amd.speech2text_streaming import hyps_to_results
    from test_engine_spec import make_batch
    ref = json.loads((GOLDEN / "frontend.json").read_text())[str(chunk)]
    short = json.loads((GOLDEN / "tiny_short.json").read_text())
    audio = synth.synth_audio(7, 64000)
    ora = RefPortStreaming(oracle_model("TINY", 1234, "meanstd"), beam_size=5)
    sb = make_batch("TINY", 1234, "meanstd", 5, False, backend="native", max_frames=256, max_tokens=200, pcm_capacity=1 << 17)
    n_calls = (len(audio) + chunk - 1) // chunk
    assert n_calls == len(ref["counts"])
    for k in range(n_calls):
        a = audio[k * chunk:(k + 1) * chunk]
        fin = k == n_calls - 1
        try:
            want = ora(torch.from_numpy(a), is_final=fin, finalize_all=fin)
            want_exc = None
        except RuntimeError as e:
            want, want_exc = None, e
        if want_exc is not None:
            assert fin and chunk in (400, 640)               # (the reference's Conv2d on < 7 frames: quirk A3)
            with pytest.raises(RuntimeError):
                sb.push([(0, a, fin)])
            assert sb.st[0].T_enc == 0                       # ... and the stream has been reset
            break
        out = sb.push([(0, a, fin)])
        got = hyps_to_results(sb.hypotheses(0), fin, fin, None, "native") if out[0] else []
        assert len(got) == len(want), (chunk, k)
        for g, w in zip(got, want):     # oracle: (filtered token ids, yseq, score, xpos); engine: (text, tokens, ids)
            assert g[2] == list(w[0]), (chunk, k)
        if not fin:
            assert sb.st[0].pcm_buffered == ref["buffers"][k], (chunk, k)
            hy, oh = sb.hypotheses(0), ora.running_hyps
            if oh is not None:     # (None until the oracle's first decode block)
                assert [h["yseq"] for h in hy] == [list(h.yseq) for h in oh], (chunk, k)
                np.testing.assert_allclose([h["score"] for h in hy], [float(h.score) for h in oh], atol=1e-3, rtol=0)
    if chunk == 640:     # the literal fixture: the encoder never ran, every call answered one empty hypothesis
        assert sb.stats["enc_calls"] == short["640"]["enc_calls"] == 0
    if chunk == 400:
        assert sb.stats["enc_calls"] == 0


def test_native_reset_quirk_and_calls_after_final():
    from test_engine_spec import run_after_final, run_reset_quirk
    run_reset_quirk(backend="native", score_tol=1e-3)
    for bbd in (0, 1):
        run_after_final(bbd, backend="native", score_tol=1e-3)


def test_native_capacity_faults_are_isolated():
    from speechcatcher_amd.engine import EngineError
    from test_engine_spec import make_batch
    sb = make_batch("TINY", 1234, "meanstd", 5, False, n_streams=2, backend="native", max_frames=40, max_tokens=160,
                    pcm_capacity=1 << 18)
    a, b = synth.synth_audio(0, 80000), synth.synth_audio(1, 80000)
    ref = make_batch("TINY", 1234, "meanstd", 5, False, n_streams=1, backend="native", max_frames=400, max_tokens=160,
                     pcm_capacity=1 << 18)
    failed = False
    for pos in range(0, 30720, 10240):
        out = sb.push([(0, a[pos:pos + 10240], False), (1, b[pos:pos + 10240], False)], isolate_faults=True)
        ref.push([(0, b[pos:pos + 10240], False)])
        assert not isinstance(out[1], Exception)
    # stream 0 gets a chunk that is too long for the batch: it alone fails, stream 1 is decoded normally
    out = sb.push([(0, a[:40000], False), (1, b[30720:40960], False)], isolate_faults=True)
    ref.push([(0, b[30720:40960], False)])
    assert isinstance(out[0], EngineError) and out[1] is True
    assert [h["yseq"] for h in sb.hypotheses(1)] == [h["yseq"] for h in ref.hypotheses(0)]
    with pytest.raises(EngineError):
        sb.push([(0, a[:40000], False)])


def test_native_final_chunk_that_faults_on_a_running_stream():
    """the LAST remaining chunk of a call faults inside the encoder planning on a stream that already has
    encoder frames (T_enc > 0) - a final chunk beyond max_frames, and a final chunk of < 7 feature frames without a reset
    after the previous final (strict server mode).  The call must report SC_ERR_CAPACITY / SC_ERR_INPUT for that stream
    (not an out_of_range from the block schedule), reset it, and accept the next push (sc_push-only hosts such as
    Speech2TextStreaming were wedged: 'still has a chunk outstanding')."""
    from speechcatcher_amd.engine import EngineError
    from test_engine_spec import make_batch
    a = synth.synth_audio(0, 120000)
    sb = make_batch("TINY", 1234, "meanstd", 5, False, n_streams=1, backend="native", max_frames=48, max_tokens=160,
                    pcm_capacity=1 << 18)
    for pos in range(0, 30720, 10240):
        sb.push([(0, a[pos:pos + 10240], False)])
    assert sb.st[0].T_enc > 0
    with pytest.raises(EngineError, match="capacity"):       # 26 s more: beyond 48 encoder frames
        sb.push([(0, a[30720:30720 + 32768], True)])
    assert sb.st[0].T_enc == 0                                # the stream has been reset ...
    ref = make_batch("TINY", 1234, "meanstd", 5, False, n_streams=1, backend="native", max_frames=48, max_tokens=160,
                     pcm_capacity=1 << 18)
    for b in (sb, ref):                                       # ... and serves the next utterance like a fresh one
        b.push([(0, a[:10240], False)])
        b.push([(0, a[10240:20480], True)])
    assert [h["yseq"] for h in sb.hypotheses(0)] == [h["yseq"] for h in ref.hypotheses(0)]
    # the same call through the isolating interface: the exception object is the stream's result
    out = sb.push([(0, a[:10240], False)], isolate_faults=True)
    out = sb.push([(0, a[10240:10240 + 10240], False)], isolate_faults=True)
    out = sb.push([(0, a[20480:20480 + 32768], True)], isolate_faults=True)
    assert isinstance(out[0], EngineError)
    assert sb.push([(0, a[:10240], False)], isolate_faults=True)[0] is True
    # a too-short final chunk right after a final chunk, no reset in between (the reference server never resets)
    sb2 = make_batch("TINY", 1234, "meanstd", 5, False, n_streams=1, backend="native", max_frames=128, max_tokens=160,
                     pcm_capacity=1 << 18)
    sb2.push([(0, a[:10240], False)])
    sb2.push([(0, a[10240:20480], True)])
    assert sb2.st[0].T_enc > 0
    with pytest.raises(RuntimeError):
        sb2.push([(0, a[:700], True)])
    sb2.push([(0, a[:10240], False)])                         # not wedged


@pytest.mark.parametrize("engine", ["native", "python"])
def test_kv_pool_exhaustion_on_the_gpu(engine):
    """self-attention K|V pool (sc_search.skv / anc) on both engines: default pool = full pool = fixture; too small a pool is a
    per-stream capacity fault"""
    from test_engine_spec import run_kv_pool_exhaustion
    if engine == "native":
        run_kv_pool_exhaustion(backend="native")
    else:
        from speechcatcher_amd.hip_backend import HipBackend
        run_kv_pool_exhaustion(backend=HipBackend("cuda:0"), device="cuda:0")


def test_poll_reports_the_oldest_completions_first():
    """sc_poll with a small max_done: streams are reported in the order their chunks completed, not
    by stream index.  Six streams get one chunk each in one admission; the engine decodes until ALL are complete
    (min_done = 6) but may only report one per call: the sequence must be ordered by the decode steps each stream needed
    for its chunk (a stream that needs fewer steps completes in an earlier tick), ties by index; every stream exactly once."""
    from test_engine_spec import make_batch
    S = 6
    sb = make_batch("TINY", 1234, "meanstd", 5, False, n_streams=S, backend="native", max_frames=200, max_tokens=300,
                    pcm_capacity=1 << 17)
    audio = [synth.synth_audio(40 + s, 10240 * 4) for s in range(S)]
    for k in range(3):                       # bring every stream to its first decode blocks, in lock-step
        sb.push([(s, audio[s][k * 10240:(k + 1) * 10240], False) for s in range(S)])
    before = [sb.st[s].n_steps_total for s in range(S)]
    # reversed submission order: the reporting order must not depend on it either
    sb.submit([(s, audio[s][3 * 10240:4 * 10240], False) for s in reversed(range(S))])
    order = []
    ids, st = sb.poll_ids(S, max_done=1)     # decodes until all six are complete, reports one
    while len(ids):
        assert len(ids) == 1 and st[0] >= 0
        order.append(int(ids[0]))
        ids, st = sb.poll_ids(0, max_done=1)
    assert sorted(order) == list(range(S))
    steps = [sb.st[s].n_steps_total - before[s] for s in range(S)]
    assert len(set(steps)) > 1, steps        # (the streams do need different numbers of steps)
    assert order == sorted(range(S), key=lambda s: (steps[s], s)), (order, steps)


def test_native_batch_of_distinct_streams_equals_one_by_one():
    """32 different utterances of different lengths in one batch (ragged-batch compaction, per-bucket graphs,
    head-parallel and six-launch layer forms by bucket size) = every stream alone = the same streams served by
    CONTINUOUS BATCHING (sc_submit / sc_poll: every stream gets its next chunk as soon as its previous one is
    reported, so the streams desynchronise and blocks of different chunk steps share decode iterations)."""
    from test_engine_spec import make_batch
    S, chunk, beam = 32, 10240, 5
    lens = [chunk * (2 + (i * 7) % 5) + (i * 1234) % 4000 for i in range(S)]
    audio = [synth.synth_audio(100 + i, n) for i, n in enumerate(lens)]

    def mk(n):
        return make_batch("TINY", 1234, "meanstd", beam, False, n_streams=n, backend="native",
                          max_frames=400, max_tokens=500, pcm_capacity=1 << 17)

    def run(streams):
        sb = mk(len(streams))
        pos = 0
        while True:
            items = []
            for slot, i in enumerate(streams):
                if pos < lens[i]:
                    end = min(pos + chunk, lens[i])
                    items.append((slot, audio[i][pos:end], end >= lens[i]))
            if not items:
                break
            sb.push(items)
            pos += chunk
        return [sb.hypotheses(slot) for slot in range(len(streams))], sb.stats

    def run_continuous(streams, min_done):
        sb = mk(len(streams))
        pos = [0] * len(streams)

        def nxt(slot):
            i = streams[slot]
            a, e = pos[slot], min(pos[slot] + chunk, lens[i])
            pos[slot] = e
            return (slot, audio[i][a:e], e >= lens[i])

        sb.submit([nxt(slot) for slot in range(len(streams))])
        n_reports, max_group = 0, 0
        while sb.outstanding:
            done = sb.poll(min_done)
            assert done and not any(isinstance(v, Exception) for v in done.values())
            n_reports += len(done)
            max_group = max(max_group, len(done))
            again = [nxt(slot) for slot in done if pos[slot] < lens[streams[slot]]]
            if again:
                sb.submit(again)
        assert n_reports == sum((lens[i] + chunk - 1) // chunk for i in streams)
        return sb.hypotheses_batch(list(range(len(streams)))), sb.stats, max_group

    batch, st = run(list(range(S)))
    for min_done in (1, 5):
        cont, stc, max_group = run_continuous(list(range(S)), min_done)
        assert stc["dec_blocks"] == st["dec_blocks"], (stc, st, max_group)
        assert stc["dec_steps"] < st["dec_steps"], (stc, st)     # fewer, fuller decode iterations
        for i in range(S):
            assert [(h["yseq"], h["xpos"]) for h in cont[i]] == [(h["yseq"], h["xpos"]) for h in batch[i]], i
            for x, y in zip(cont[i], batch[i]):
                assert abs(x["score"] - y["score"]) < 1e-3
    for i in range(0, S, 3):
        solo, sts = run([i])
        assert len(solo[0]) == len(batch[i]) > 0
        for x, y in zip(solo[0], batch[i]):
            assert x["yseq"] == y["yseq"] and x["xpos"] == y["xpos"], i
            assert abs(x["score"] - y["score"]) < 2e-3 * max(1.0, abs(x["score"])), i


def test_native_batched_readback_and_argument_checks():
    """sc_get_hyps_batch (one pack launch + one copy for all streams) = sc_get_hyps stream by stream; push_block =
    push; the C ABI refuses a stream listed twice, a second chunk for a stream that has one outstanding, and a
    reset of such a stream; per-stream failure messages do not clobber each other."""
    import ctypes as C
    from speechcatcher_amd import _abi
    from speechcatcher_amd.engine import EngineError
    from test_engine_spec import make_batch
    S, chunk = 6, 10240
    kw = dict(n_streams=S, backend="native", max_frames=400, max_tokens=300, pcm_capacity=1 << 18)
    sb, sb2 = make_batch("TINY", 1234, "meanstd", 5, False, **kw), make_batch("TINY", 1234, "meanstd", 5, False, **kw)
    audio = np.stack([synth.synth_audio(40 + s, chunk * 4) for s in range(S)])
    for k in range(4):
        sb.push([(s, audio[s, k * chunk:(k + 1) * chunk], False) for s in range(S)])
        st = sb2.push_block(np.arange(S), np.ascontiguousarray(audio[:, k * chunk:(k + 1) * chunk]))
        assert (st >= 0).all()
    one = [sb.hypotheses(s) for s in range(S)]
    allb = sb2.hypotheses_batch(list(range(S)))
    assert all(len(one[s]) > 0 and one[s] == allb[s] for s in range(S))
    arr = sb.hypotheses_arrays([3, 1], nbest=2)
    assert arr["n_hyps"].tolist() == [2, 2] and arr["ids"][0, 0, :arr["lens"][0, 0]].tolist() == one[3][0]["yseq"]
    assert arr["xpos"][1, 1, :arr["lens"][1, 1]].tolist() == one[1][1]["xpos"] and arr["score"][1, 0] == one[1][0]["score"]
    with pytest.raises(EngineError, match="listed twice"):
        sb.push([(2, audio[2, :chunk], False), (2, audio[2, :chunk], False)])
    sb.submit([(0, audio[0, :chunk], False)])
    with pytest.raises(EngineError, match="outstanding"):
        sb.submit([(0, audio[0, :chunk], False)])
    with pytest.raises(_abi.ScasrError, match="outstanding"):
        sb.reset(0)
    with pytest.raises(_abi.ScasrError, match="decode block|reported"):
        sb.hypotheses(0)
    assert sb.poll(1) == {0: True} and sb.outstanding == 0
    # two streams fail in one call, each keeps its own message
    sb.reset(1)
    out = sb.push([(1, synth.synth_audio(1, 700), True), (4, np.zeros(50000, np.float32), False),
                   (5, audio[5, :chunk], False)], isolate_faults=True)
    assert isinstance(out[1], RuntimeError) and "3x3" in str(out[1]) and "stream 1" in str(out[1])
    assert isinstance(out[4], EngineError) and "max_chunk_samples" in str(out[4]) and out[5] is True
    assert sb.lib.sc_stream_last_error(sb.handle, 5) == b""


@pytest.mark.parametrize("seed,bbd,continuous,split", [(0, False, False, None), (1, True, False, None), (2, False, True, None),
                                                       (3, True, True, "32"), (4, False, False, "32")])
def test_native_random_sessions_equal_the_python_engine(seed, bbd, continuous, split, monkeypatch):
    """Randomised sessions on 16 stream slots (tiny dims): every push feeds a random subset of the streams with chunks
    of random length (a few hundred samples to 1.5 s), utterances end at random and their slots are reset and reused -
    block schedules, ragged buckets, final calls, resets and the early `return []` calls interleave in ways no fixture
    covers.  The C++ engine (sc_push, or continuous: the chunks of a step submitted as two groups and polled one
    completion at a time) and the Python engine over the same kernels must end every step with the same hypotheses
    for every stream.  split: the CTC scan of the C++ engine split over T
    from 32 frames on (the Python engine always walks sequentially)."""
    from speechcatcher_amd.hip_backend import HipBackend
    from test_engine_spec import make_batch
    if split:
        monkeypatch.setenv("SC_SCAN_SPLIT_MIN", split)
    S, beam = 16, 5
    kw = dict(n_streams=S, max_frames=400, max_tokens=400, pcm_capacity=1 << 17, strict_reference=False)
    nat = make_batch("TINY", 1234, "meanstd", beam, bbd, backend="native", **kw)
    pye = make_batch("TINY", 1234, "meanstd", beam, bbd, backend=HipBackend("cuda:0"), device="cuda:0", **kw)
    rng = np.random.default_rng(seed)
    fed = [0] * S            # samples fed to the current utterance of a slot
    utt = list(range(S))     # audio stream id of the current utterance
    next_utt = S
    longest, resets = 0, 0
    for step in range(40):
        items = []
        for s in range(S):
            if rng.random() < 0.35:
                continue
            n = int(rng.choice([300, 700, 1600, 4000, 8192, 10240, 16000, 24000]))
            audio = synth.synth_audio(utt[s], fed[s] + n)[fed[s]:]
            fin = bool(rng.random() < 0.12 and fed[s] + n > 12000)
            items.append((s, audio, fin))
            fed[s] += n
        if not items:
            continue
        if continuous:
            cut = int(rng.integers(0, len(items) + 1))
            a = {}
            for part in (items[:cut], items[cut:]):
                if part:
                    nat.submit(part)
                    if rng.random() < 0.5:
                        a.update(nat.poll(1))
            while nat.outstanding:
                a.update(nat.poll(1))
        else:
            a = nat.push(items, isolate_faults=True)
        b = pye.push(items, isolate_faults=True)
        for s, _, fin in items:
            fa, fb = isinstance(a[s], Exception), isinstance(b[s], Exception)
            assert fa == fb, (step, s, a[s], b[s])
            if not fa:
                assert bool(a[s]) == bool(b[s]), (step, s)
                ha, hb = nat.hypotheses(s), pye.hypotheses(s)
                assert [(h["yseq"], h["xpos"]) for h in ha] == [(h["yseq"], h["xpos"]) for h in hb], (step, s)
                for x, y in zip(ha, hb):
                    assert abs(x["score"] - y["score"]) < 2e-3 * max(1.0, abs(y["score"])), (step, s)
                longest = max([longest] + [len(h["yseq"]) for h in ha])
            if fin or fa or fed[s] > 90000:
                nat.reset(s)
                pye.reset(s)
                fed[s], utt[s] = 0, next_utt
                next_utt += 1
                resets += 1
    assert longest > 30 and resets >= 5, (longest, resets)   # the sessions did decode and did end


@pytest.mark.parametrize("seed,bbd,depth", [(0, False, 2), (1, True, 3), (2, False, 4), (3, True, 2)])
def test_native_queued_chunks_equal_one_at_a_time(seed, bbd, depth):
    """sc_streams_set_queue_depth > 1: a host that has the audio already hands a stream's next chunk(s) to the engine
    while an earlier one is still being decoded.  12 streams of random utterances (random chunk lengths, final chunks,
    resets, new utterances on the same slot), submitted ahead up to the depth in random subsets and polled in random
    portions: EVERY reply - has-output flag and all hypotheses, read between the polls while the stream's next chunk is
    already decoding - equals the reply of the one-call-at-a-time protocol (sc_push) for that chunk."""
    from speechcatcher_amd.engine import EngineError
    from test_engine_spec import make_batch
    S, beam = 12, 5
    kw = dict(n_streams=S, max_frames=400, max_tokens=400, pcm_capacity=1 << 17, strict_reference=False)
    ref = make_batch("TINY", 1234, "meanstd", beam, bbd, backend="native", **kw)
    que = make_batch("TINY", 1234, "meanstd", beam, bbd, backend="native", **kw)
    que.set_queue_depth(depth)
    rng = np.random.default_rng(100 + seed)
    # per stream: utterances = lists of (samples, is_final)
    plan, expect = [], []
    for s in range(S):
        chunks = []
        for u in range(int(rng.integers(1, 4))):
            n_chunks = int(rng.integers(2, 9))
            lens = [int(rng.choice([700, 1600, 4000, 8192, 10240, 16000])) for _ in range(n_chunks)]
            audio = synth.synth_audio(1000 * seed + 10 * s + u, sum(lens))
            pos = 0
            for k, n in enumerate(lens):
                chunks.append((audio[pos:pos + n], k == n_chunks - 1))
                pos += n
        plan.append(chunks)
        rec = []
        for pcm, fin in chunks:                       # the one-at-a-time protocol on this stream
            out = ref.push([(s, pcm, fin)])
            rec.append((bool(out[s]), ref.hypotheses(s)))
            if fin:
                ref.reset(s)
        expect.append(rec)
    sub = [0] * S      # chunks submitted
    rep = [0] * S      # chunks reported
    wait_reset = [False] * S
    n_ahead, longest = 0, 0
    while any(rep[s] < len(plan[s]) for s in range(S)):
        for _ in range(depth):                         # one chunk per stream and call: up to `depth` calls
            items = []
            for s in range(S):
                if sub[s] - rep[s] < depth and sub[s] < len(plan[s]) and not wait_reset[s] and rng.random() < 0.8:
                    pcm, fin = plan[s][sub[s]]
                    items.append((s, pcm, fin))
                    n_ahead += sub[s] > rep[s]
                    sub[s] += 1
                    wait_reset[s] = fin                # nothing behind a final chunk: wait for its reply, then reset
            if items:
                que.submit(items)
        if not que.outstanding:
            continue
        got = que.poll(int(rng.integers(1, 4)))
        assert got
        for s, has in got.items():
            exp_has, exp_hyps = expect[s][rep[s]]
            assert not isinstance(has, Exception), (s, has)
            assert bool(has) == exp_has, (s, rep[s])
            hy = que.hypotheses(s)
            assert [(h["yseq"], h["xpos"]) for h in hy] == [(h["yseq"], h["xpos"]) for h in exp_hyps], (s, rep[s])
            for x, y in zip(hy, exp_hyps):
                assert abs(x["score"] - y["score"]) < 2e-3 * max(1.0, abs(y["score"])), (s, rep[s])
            longest = max([longest] + [len(h["yseq"]) for h in hy])
            fin = plan[s][rep[s]][1]
            rep[s] += 1
            if fin:
                assert sub[s] == rep[s]
                que.reset(s)
                wait_reset[s] = False
    assert n_ahead > 20 and longest > 20, (n_ahead, longest)      # chunks WERE queued behind outstanding ones
    # the rules: no more than `depth` outstanding, nothing behind a final chunk
    que.submit([(0, synth.synth_audio(7, 8192), False)])
    for _ in range(depth - 1):
        que.submit([(0, synth.synth_audio(7, 8192), True if _ == depth - 2 else False)])
    with pytest.raises(EngineError, match="outstanding"):
        que.submit([(0, synth.synth_audio(7, 8192), False)])
    while que.outstanding:
        que.poll(1)
    que.reset(0)
    que.submit([(0, synth.synth_audio(7, 8192), True)])
    with pytest.raises(EngineError, match="final chunk"):
        que.submit([(0, synth.synth_audio(7, 8192), False)])
    while que.outstanding:
        que.poll(1)


def test_native_queue_depth_with_lock_step_calls_and_late_reads():
    """queue depth 2 on a batch that is ALSO driven with sc_push, and hypotheses read late: a push supersedes the copy
    of the stream's last polled reply (its hypotheses are the live ones again), and a polled reply stays readable while
    the stream's next chunk - already queued - is decoding."""
    from test_engine_spec import make_batch
    kw = dict(n_streams=2, max_frames=400, max_tokens=400, pcm_capacity=1 << 17, strict_reference=False)
    one = make_batch("TINY", 1234, "meanstd", 5, False, backend="native", **kw)
    two = make_batch("TINY", 1234, "meanstd", 5, False, backend="native", **kw)
    two.set_queue_depth(2)
    a = synth.synth_audio(31, 10240 * 8)
    ck = [a[k * 10240:(k + 1) * 10240] for k in range(8)]
    exp = []
    for k in range(8):
        one.push([(0, ck[k], False)])
        exp.append([(h["yseq"], h["xpos"]) for h in one.hypotheses(0)])
    ids = lambda sb: [(h["yseq"], h["xpos"]) for h in sb.hypotheses(0)]   # noqa: E731
    two.push([(0, ck[0], False)])
    assert ids(two) == exp[0]
    two.submit([(0, ck[1], False)])
    two.submit([(0, ck[2], False)])                   # queued behind chunk 1
    assert list(two.poll(1)) == [0] and ids(two) == exp[1]      # chunk 2 may be decoding by now
    assert list(two.poll(1)) == [0] and ids(two) == exp[2]
    two.push([(0, ck[3], False)])                     # lock-step again: live hypotheses, not the copy of chunk 2's reply
    assert ids(two) == exp[3]
    two.push([(0, ck[4], False)])
    assert ids(two) == exp[4]
    two.submit([(0, ck[5], False)])
    two.submit([(0, ck[6], False)])
    two.submit([(1, ck[0], False)])
    got = {}
    while two.outstanding:
        for s in two.poll(1):
            got.setdefault(s, []).append([(h["yseq"], h["xpos"]) for h in two.hypotheses(s)])
    assert got[0] == [exp[5], exp[6]] and got[1] == [exp[0]]


def test_native_queued_chunks_and_failures():
    """queue depth 3 and failures: (a) a chunk that cannot be admitted (longer than max_chunk_samples) is reported as
    failed in its turn, after the good chunk before it, and so is the chunk queued behind it; (b) a chunk that fails
    while decoding (max_tokens exceeded) takes the chunks queued behind it with it.  Other streams are not affected and
    the failed streams work again after their reset."""
    from speechcatcher_amd.engine import EngineError
    from test_engine_spec import make_batch
    sb = make_batch("TINY", 1234, "meanstd", 5, False, backend="native", n_streams=3, max_frames=400, max_tokens=48,
                    pcm_capacity=1 << 18, strict_reference=False, max_chunk_samples=20000)
    one = make_batch("TINY", 1234, "meanstd", 5, False, backend="native", n_streams=1, max_frames=400, max_tokens=48,
                     pcm_capacity=1 << 18, strict_reference=False, max_chunk_samples=20000)
    sb.set_queue_depth(3)
    a = synth.synth_audio(11, 10240 * 12)
    # (a) stream 0: good, too long, good (fails with the one before it)
    sb.submit([(0, a[:10240], False)])
    sb.submit([(0, a[10240:10240 + 30000], False)])
    sb.submit([(0, a[:8192], False)])
    # (b) stream 1: chunks until its hypotheses outgrow max_tokens, three in the queue at a time; stream 2: healthy
    sb.submit([(2, a[:10240], False)])
    got, k1, failed_at = {0: [], 1: [], 2: []}, 0, None
    while failed_at is None or sb.outstanding:
        while failed_at is None and k1 < 12 and (k1 - len(got[1])) < 3:
            sb.submit([(1, a[k1 * 10240:(k1 + 1) * 10240], False)])
            k1 += 1
        for s, r in sb.poll(1).items():
            got[s].append(r)
            if s == 1 and isinstance(r, Exception) and failed_at is None:
                failed_at = len(got[1]) - 1
    assert got[0][0] is True and isinstance(got[0][1], EngineError) and "max_chunk_samples" in str(got[0][1])
    assert len(got[0]) == 3 and isinstance(got[0][2], EngineError)
    assert got[2] == [True]
    assert failed_at is not None and failed_at >= 2 and "max_tokens" in str(got[1][failed_at])
    assert all(r is True or r is False for r in got[1][:failed_at])
    assert all(isinstance(r, Exception) for r in got[1][failed_at:]) and len(got[1]) == k1   # the queued ones went with it
    # the one-at-a-time protocol fails at the same chunk
    for k in range(failed_at + 1):
        r = one.push([(0, a[k * 10240:(k + 1) * 10240], False)], isolate_faults=True)[0]
        assert isinstance(r, Exception) == (k == failed_at), k
    # all three streams go on (0 and 1 were reset by their failures)
    for s in range(3):
        sb.submit([(s, a[:10240], False)])
    while sb.outstanding:
        for s, r in sb.poll(3).items():
            assert r is True, (s, r)
    one.reset(0)
    one.push([(0, a[:10240], False)])
    assert [h["yseq"] for h in sb.hypotheses(0)] == [h["yseq"] for h in one.hypotheses(0)]
    assert [h["yseq"] for h in sb.hypotheses(1)] == [h["yseq"] for h in one.hypotheses(0)]


def test_native_xl_batch_equals_python_engine():
    """XL dims, 12 streams: the C++ engine and the Python engine (same kernels) end with identical hypotheses."""
    from speechcatcher_amd.hip_backend import HipBackend
    from test_engine_spec import make_batch
    S, chunk, beam, n = 12, 10240, 10, 6
    audio = [synth.synth_audio(300 + i, chunk * n) for i in range(S)]

    def run(backend, device):
        sb = make_batch("XL", 1234, "meanstd", beam, False, n_streams=S, backend=backend, device=device, max_frames=200,
                        max_tokens=600, pcm_capacity=1 << 17)
        for k in range(n):
            last = k == n - 1
            sb.push([(s, audio[s][k * chunk:(k + 1) * chunk], last) for s in range(S) if not last or s % 2 == 0])
        return [sb.hypotheses(s) for s in range(S)]

    nat = run("native", "cuda:0")
    py = run(HipBackend("cuda:0"), "cuda:0")
    for s in range(S):
        assert [h["yseq"] for h in nat[s]] == [h["yseq"] for h in py[s]], s
        # (not bit-equal: the C++ engine projects the CTC / cross-attention K|V rows inside the encoder stage, in other
        # GEMM batches - another split-K summation order - than the Python engine does at block start)
        assert all(abs(x["score"] - y["score"]) < 5e-4 for x, y in zip(nat[s], py[s])), s


@pytest.mark.parametrize("dims,steps,streams,seed", [("TINY", 80, 24, 3), ("TINY", 80, 24, 4), ("XL", 50, 12, 5)])
def test_random_sessions_are_bit_reproducible(dims, steps, streams, seed):
    """tools/soak_continuous.py, short: randomised sessions (chunk lengths 300..24000 samples, finals, resets, oversized
    chunks that fail alone, random poll sizes and encoder-batch thresholds, lock-step calls mixed in) served with
    continuous batching against the SAME calls one stream at a time - every reply carries the same hypotheses with
    BIT-IDENTICAL scores, whatever shared the GPU with it (the script asserts both).  The long runs of the round:
    profiles/r05_soak_continuous.txt."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SC_TEST_HOOKS="1")
    env.pop("SOAK_ALLOW_INEXACT", None)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "soak_continuous.py"), str(steps), str(streams), str(seed), dims],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("soak ok") and "scores bit-identical in" in last, last
    a, b = last.split("scores bit-identical in ")[1].split(" compared")[0].split(" of ")
    assert a == b and int(a) > 50, last


@pytest.mark.parametrize("dims,kv", [("XL", "float32"), ("XL", "float16"), ("TINY", "float32")])
def test_kv_rows_of_all_layers_in_one_launch(dims, kv, monkeypatch):
    """project_rows (csrc/streams.hip) computes the cross-attention K|V rows of ALL decoder layers with one product over the
    layers' weights, one behind the other (sc_gemm_colblocks), instead of one sc_gemm per layer.  Same k chain per element:
    the hypotheses AND their scores are the same bits as with the per-layer launches (SC_KV_PER_LAYER)."""
    from test_engine_spec import make_batch
    S, chunk, beam, n = 6, 10240, 10 if dims == "XL" else 5, 5
    audio = [synth.synth_audio(500 + i, chunk * n) for i in range(S)]

    def run():
        sb = make_batch(dims, 1234, "meanstd", beam, False, n_streams=S, backend="native", device="cuda:0", max_frames=200,
                        max_tokens=600, pcm_capacity=1 << 17, kv_dtype=kv)
        for k in range(n):
            sb.push([(s, audio[s][k * chunk:(k + 1) * chunk], k == n - 1) for s in range(S)])
        return [sb.hypotheses(s) for s in range(S)]

    one = run()
    monkeypatch.setenv("SC_KV_PER_LAYER", "1")
    per = run()
    assert any(len(h[0]["yseq"]) > 3 for h in one)
    for s in range(S):
        assert [h["yseq"] for h in one[s]] == [h["yseq"] for h in per[s]], s
        assert [h["score"] for h in one[s]] == [h["score"] for h in per[s]], s


@pytest.mark.parametrize("vosk,continuous", [(False, False), (True, False), (False, True), (True, True)])
def test_native_server_sessions_equal_private_oracle_sessions(vosk, continuous):
    """continuous: the server loop over sc_submit / sc_poll - every client is answered as soon as ITS chunk is decoded"""
    from test_server_session import run_sessions_vs_oracle
    run_sessions_vs_oracle(vosk, backend="native", continuous=continuous)


def test_native_scheduler_and_segment_loop():
    from test_scheduler import run_segments_serial_strict, run_sessions_different_chunking
    run_sessions_different_chunking(backend="native")
    run_segments_serial_strict(backend="native")


C_HOST = r"""
/* A plain C host of libscasr: packed model file + raw f32 PCM -> token ids of the best hypotheses, one line per
 * call that produced a decode block.  No Python, no torch. */
#include <stdio.h>
#include <stdlib.h>
#include "scasr.h"
int main(int argc, char **argv) {
  if (argc < 6) return 2;
  const int chunk = atoi(argv[3]), beam = atoi(argv[4]), bbd = atoi(argv[5]);
  sc_engine *eng = NULL; sc_streams *st = NULL;
  if (sc_version() != SC_ABI_VERSION) { fprintf(stderr, "libscasr ABI %d, header %d\n", sc_version(), SC_ABI_VERSION); return 3; }
  if (sc_engine_load(argv[1], 0, &eng) != SC_OK) { fprintf(stderr, "%s\n", sc_last_error()); return 1; }
  sc_stream_options o = {1, beam, 0.3f, bbd, 256, 200, 1 << 18, 32768, 1};
  if (sc_streams_create(eng, &o, &st) != SC_OK) { fprintf(stderr, "%s\n", sc_last_error()); return 1; }
  FILE *f = fopen(argv[2], "rb"); if (!f) return 1;
  fseek(f, 0, SEEK_END); long n = ftell(f) / 4; fseek(f, 0, SEEK_SET);
  float *pcm = (float *)malloc(n * 4);
  if (fread(pcm, 4, n, f) != (size_t)n) return 1;
  fclose(f);
  static int32_t ids[16 * 200]; int lens[16]; double sc[16];
  for (long pos = 0; pos < n; pos += chunk) {
    int sid = 0, cnt = (int)(pos + chunk < n ? chunk : n - pos), status = 0;
    uint8_t fin = pos + chunk >= n;
    const float *p = pcm + pos;
    if (sc_push(st, &sid, &p, &cnt, &fin, 1, &status) != SC_OK || status < 0) { fprintf(stderr, "%s\n", sc_last_error()); return 1; }
    sc_stream_info_t info; sc_stream_info(st, 0, &info);
    int nh = sc_get_hyps(st, 0, beam, 200, ids, NULL, lens, sc, NULL, NULL);
    printf("%d %d %d", status, info.enc_frames, info.processed_block);
    for (int h = 0; h < nh; ++h) { printf(" |"); for (int i = 0; i < lens[h]; ++i) printf(" %d", ids[h * 200 + i]); }
    printf("\n");
  }
  sc_streams_destroy(st); sc_engine_destroy(eng); free(pcm);
  return 0;
}
"""


def test_c_host_program_reproduces_the_reference_fixture(tmp_path):
    """gcc-compiled C program + libscasr.so: tiny_c10240_b10_bbd0 call by call (encoder frames, processed blocks,
    token ids of every live hypothesis)."""
    from speechcatcher_amd.config import TINY
    from speechcatcher_amd.weights import PackedWeights
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    js, _ = load_case("tiny_c10240_b10_bbd0")
    meta = js["meta"]
    sd = synth.make_state_dict(TINY, meta["seed"])
    mean, std = synth.stats_to_mean_std(synth.make_stats(TINY, kind=meta["stats"]))
    PackedWeights(sd, TINY, "cpu", mean, std).save_packed(tmp_path / "tiny.scpk")
    synth.synth_audio(meta["audio_stream"], meta["n_samples"]).astype("<f4").tofile(tmp_path / "audio.f32")
    (tmp_path / "host.c").write_text(C_HOST)
    libdir = ROOT / "speechcatcher_amd"
    subprocess.run([gcc, "-std=c99", "-O1", "-I", str(ROOT / "include"), str(tmp_path / "host.c"), "-L", str(libdir),
                    "-lscasr", f"-Wl,-rpath,{libdir}", "-o", str(tmp_path / "host")], check=True)
    res = subprocess.run([str(tmp_path / "host"), str(tmp_path / "tiny.scpk"), str(tmp_path / "audio.f32"),
                          str(meta["chunk"]), str(meta["beam"]), str(int(meta["bbd"]))], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.strip().splitlines()
    assert len(lines) == len(js["calls"])
    nblk = 0
    for line, call in zip(lines, js["calls"]):
        head, *hyps = line.split(" |")
        status, enc_frames, pblock = [int(x) for x in head.split()]
        assert enc_frames == call["enc_buffer_len"] and pblock == call["processed_block"]
        nblk += call["n_blocks"]
        if call["n_blocks"]:
            got = sorted(tuple(int(t) for t in h.split()) for h in hyps)
            assert got == sorted(tuple(y) for y in js["blocks"][nblk - 1]["yseq"])


C_HOST_CONTINUOUS = r"""
/* The same fixture through the continuous-batching entry points, from plain C: three streams get the SAME audio,
 * staggered (stream k's first chunk is submitted k polls late), each with one chunk outstanding: sc_submit, sc_poll,
 * sc_get_hyps_batch for the streams that answered, their next chunks.  One line per reply: stream, then as above. */
#include <stdio.h>
#include <stdlib.h>
#include "scasr.h"
#define NS 3
int main(int argc, char **argv) {
  if (argc < 6) return 2;
  const int chunk = atoi(argv[3]), beam = atoi(argv[4]), bbd = atoi(argv[5]);
  sc_engine *eng = NULL; sc_streams *st = NULL;
  if (sc_version() != SC_ABI_VERSION) { fprintf(stderr, "libscasr ABI %d, header %d\n", sc_version(), SC_ABI_VERSION); return 3; }
  if (sc_engine_load(argv[1], 0, &eng) != SC_OK) { fprintf(stderr, "%s\n", sc_last_error()); return 1; }
  sc_stream_options o = {NS, beam, 0.3f, bbd, 256, 200, 1 << 18, 32768, 1};
  if (sc_streams_create(eng, &o, &st) != SC_OK) { fprintf(stderr, "%s\n", sc_last_error()); return 1; }
  if (sc_streams_set_encoder_batch(st, 2) != SC_OK) return 1;
  FILE *f = fopen(argv[2], "rb"); if (!f) return 1;
  fseek(f, 0, SEEK_END); long n = ftell(f) / 4; fseek(f, 0, SEEK_SET);
  float *pcm = (float *)malloc(n * 4);
  if (fread(pcm, 4, n, f) != (size_t)n) return 1;
  fclose(f);
  static int32_t ids[NS * 16 * 200]; int lens[NS * 16], nh[NS]; double sc[NS * 16];
  long pos[NS] = {0, 0, 0}; int started[NS] = {0, 0, 0}; int polls = 0;
  while (1) {
    int sub[NS], cnt[NS], k = 0; const float *ptr[NS]; uint8_t fin[NS];
    for (int s = 0; s < NS; ++s) {
      if (started[s] == 1 || pos[s] >= n || polls < s) continue;       /* one chunk outstanding; staggered start */
      sub[k] = s; ptr[k] = pcm + pos[s]; cnt[k] = (int)(pos[s] + chunk < n ? chunk : n - pos[s]);
      fin[k] = pos[s] + chunk >= n; pos[s] += chunk; started[s] = 1; ++k;
    }
    if (k && sc_submit(st, sub, ptr, cnt, fin, k) != SC_OK) { fprintf(stderr, "%s\n", sc_last_error()); return 1; }
    if (sc_streams_outstanding(st) == 0) { if (pos[0] >= n && pos[1] >= n && pos[2] >= n) break; ++polls; continue; }
    int done[NS], status[NS];
    const int nd = sc_poll(st, 1, NS, done, status);
    ++polls;
    if (nd < 0) { fprintf(stderr, "%s\n", sc_last_error()); return 1; }
    if (nd && sc_get_hyps_batch(st, done, nd, beam, 200, ids, NULL, lens, nh, sc, NULL, NULL) != SC_OK) return 1;
    for (int i = 0; i < nd; ++i) {
      if (status[i] < 0) { fprintf(stderr, "%s\n", sc_stream_last_error(st, done[i])); return 1; }
      sc_stream_info_t info; sc_stream_info(st, done[i], &info);
      printf("%d %d %d %d", done[i], status[i], info.enc_frames, info.processed_block);
      for (int h = 0; h < nh[i]; ++h) { printf(" |"); for (int j = 0; j < lens[i * beam + h]; ++j) printf(" %d", ids[(i * beam + h) * 200 + j]); }
      printf("\n");
      started[done[i]] = 0;
    }
  }
  sc_streams_destroy(st); sc_engine_destroy(eng); free(pcm);
  return 0;
}
"""


def test_c_host_program_with_continuous_batching(tmp_path):
    """sc_submit / sc_poll / sc_get_hyps_batch from a gcc-compiled C program: three staggered streams with the fixture
    audio; EVERY stream reproduces the reference fixture reply by reply."""
    from speechcatcher_amd.config import TINY
    from speechcatcher_amd.weights import PackedWeights
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    js, _ = load_case("tiny_c10240_b10_bbd0")
    meta = js["meta"]
    sd = synth.make_state_dict(TINY, meta["seed"])
    mean, std = synth.stats_to_mean_std(synth.make_stats(TINY, kind=meta["stats"]))
    PackedWeights(sd, TINY, "cpu", mean, std).save_packed(tmp_path / "tiny.scpk")
    synth.synth_audio(meta["audio_stream"], meta["n_samples"]).astype("<f4").tofile(tmp_path / "audio.f32")
    (tmp_path / "hostc.c").write_text(C_HOST_CONTINUOUS)
    libdir = ROOT / "speechcatcher_amd"
    subprocess.run([gcc, "-std=c99", "-O1", "-I", str(ROOT / "include"), str(tmp_path / "hostc.c"), "-L", str(libdir),
                    "-lscasr", f"-Wl,-rpath,{libdir}", "-o", str(tmp_path / "hostc")], check=True)
    res = subprocess.run([str(tmp_path / "hostc"), str(tmp_path / "tiny.scpk"), str(tmp_path / "audio.f32"),
                          str(meta["chunk"]), str(meta["beam"]), str(int(meta["bbd"]))], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    per = {0: [], 1: [], 2: []}
    for line in res.stdout.strip().splitlines():
        per[int(line.split()[0])].append(line.split(" ", 1)[1])
    for sid, lines in per.items():
        assert len(lines) == len(js["calls"]), sid
        nblk = 0
        for line, call in zip(lines, js["calls"]):
            head, *hyps = line.split(" |")
            status, enc_frames, pblock = [int(x) for x in head.split()]
            assert enc_frames == call["enc_buffer_len"] and pblock == call["processed_block"], sid
            nblk += call["n_blocks"]
            if call["n_blocks"]:
                got = sorted(tuple(int(t) for t in h.split()) for h in hyps)
                assert got == sorted(tuple(y) for y in js["blocks"][nblk - 1]["yseq"]), sid


def test_cli_round_trips_a_wav(tmp_path):
    """``python -m speechcatcher_amd -m <model dir> -b 3 recording.wav``: the reference CLI's file mode (flags of
    speechcatcher.py:756-808) as a child process; the .txt / .json next to the input carry what the library gives
    for the same recording (one slot = the reference's serial segment loop on one model)."""
    import sys
    import wave
    from speechcatcher_amd.config import TINY, SearchConfig
    from speechcatcher_amd.native import NativeStreamBatch
    from speechcatcher_amd.segmenter import recognize_recording
    from speechcatcher_amd.speech2text_streaming import load_model
    mdir = synth.write_model_dir(tmp_path / "tiny", TINY, seed=1234, stats_kind="meanstd")
    rate = 16000
    x = synth.synth_audio(40, 70 * rate) * 20000
    for t0 in (18, 41):
        x[t0 * rate:(t0 + 2) * rate] *= 0.01
    x = x.astype(np.int16)
    wav = tmp_path / "rec.wav"
    with wave.open(str(wav), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(rate)
        f.writeframes(x.tobytes())
    res = subprocess.run([sys.executable, "-m", "speechcatcher_amd", "-m", str(mdir), "-b", "3", "--quiet", "--no-progress",
                          str(wav)], cwd=str(ROOT), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "Wrote transcription to" in res.stdout
    out = json.loads((tmp_path / "rec.wav.json").read_text())
    assert (tmp_path / "rec.wav.txt").read_text() == out["complete_text"]
    s2t = load_model(str(mdir), device="cuda", beam_size=3, use_bbd=True)
    sb = NativeStreamBatch(s2t.weights, 1, SearchConfig(beam_size=3, use_bbd=True), max_frames=2000, max_tokens=1200,
                           pcm_capacity=1 << 21, engine=s2t.batch.engine)
    text, info = recognize_recording(sb, x, rate, chunk_length=8192, token_list=s2t.token_list, reference_finalize=True)
    assert out["complete_text"] == text and len(out["paragraphs"]) == len(info)
    assert out["paragraphs"][0]["tokens"] == info[0]["tokens"]
    # wrong input format is refused with the conversion hint
    bad = tmp_path / "bad.wav"
    with wave.open(str(bad), "wb") as f:
        f.setnchannels(2); f.setsampwidth(2); f.setframerate(8000)
        f.writeframes(x[:1000].tobytes())
    res = subprocess.run([sys.executable, "-m", "speechcatcher_amd", "-m", str(mdir), str(bad)], cwd=str(ROOT),
                         capture_output=True, text=True)
    assert res.returncode != 0 and "16 kHz mono" in (res.stderr + res.stdout)


def test_bench_two_ranks_on_one_device(tmp_path):
    """The N > 1 path of bench.py, launch-ready: two fresh child processes (one per rank, world size 2, gloo
    rendezvous on 127.0.0.1, both on the one GPU of this box: SC_BENCH_SINGLE_DEVICE=1) shard the streams, run the
    barrier / max-over-ranks timing contract and the final gather; rank 0 prints the whole-job JSON line."""
    import os
    import socket
    import sys
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), SC_DIST_BACKEND="gloo", SC_BENCH_SINGLE_DEVICE="1")
        procs.append(subprocess.Popen([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--streams", "8", "--steps", "3",
                                       "--warmup", "2", "--preroll", "3", "--roofline-steps", "0", "--no-cpu-baseline", "--no-long-context"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=600) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-1500:] for o in outs]
    line = json.loads(outs[0][0].strip().splitlines()[-1])
    assert not any(ln.startswith("{") for ln in outs[1][0].splitlines())     # only rank 0 prints the JSON line
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0
    assert abs(line["value"] - 2 * 8 * 3 * 0.64 / (line["ms_per_step"] * 3e-3)) < 1e-2 * line["value"]   # whole-job aggregate


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with NO launcher and no WORLD_SIZE in the environment (Next 6): bench.py
    itself starts the two rank processes (fresh children of a parent that never touches the GPU; gloo rendezvous on
    127.0.0.1, both ranks on this box's one GPU: SC_BENCH_SINGLE_DEVICE=1), each on its own slice of the host cores, and
    prints ONE line with n_gpus = 2 and the per-rank values."""
    import os
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(SC_DIST_BACKEND="gloo", SC_BENCH_SINGLE_DEVICE="1")
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--streams", "8", "--steps", "3", "--warmup", "2",
                          "--preroll", "3", "--roofline-steps", "0", "--no-cpu-baseline", "--no-long-context"], env=env,
                         capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0
    assert [r["rank"] for r in line["per_rank"]] == [0, 1] and all(r["audio_s_per_s"] > 0 for r in line["per_rank"])
    # whole-job value = all ranks' audio over the slowest rank's time
    slowest = max(r["ms_per_step"] for r in line["per_rank"])
    assert abs(line["ms_per_step"] - slowest) < 1e-3 * slowest + 1e-3
    # --gpus larger than the visible devices without the single-device switch: refused by the launcher itself
    env.pop("SC_BENCH_SINGLE_DEVICE")
    bad = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "64"], env=env, capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "GPU" in bad.stderr


def test_bench_dump_outputs_are_the_same_in_both_modes(tmp_path):
    """`bench.py --dump-outputs DIR`: the replies to the last timed chunk step.  The continuous closed loop (streams spread
    over the window by timing; the untimed catch-up feeds the capture too, and with --full the roofline leg before it),
    in a plain and in a --full run, and strict lock-step (one batched call per step) must write the same files, bit for
    bit, in float32 / float64 - and the line keeps `steps` and `ms_per_step` of the timed window.  Only --full runs the
    roofline leg."""
    import sys
    steps, warmup, preroll = 4, 2, 3
    got = {}
    for mode, full in (("continuous", False), ("continuous", True), ("strict", False)):
        d = tmp_path / f"{mode}_{int(full)}"
        res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--streams", "8", "--steps", str(steps),
                              "--warmup", str(warmup), "--preroll", str(preroll), "--roofline-steps", "1", "--legs", "none",
                              "--mode", mode, "--dump-outputs", str(d)] + (["--full"] if full else []),
                             capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        line = json.loads(res.stdout.strip().splitlines()[-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0
        assert line["full"] is full and (line["roofline"] is not None) is full
        assert line["dump_outputs"]["chunk"] == preroll + warmup + steps - 1
        got[mode, full] = {f: np.load(d / f) for f in line["dump_outputs"]["files"]}
        assert sum(a.nbytes for a in got[mode, full].values()) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) for a in got[mode, full].values())
    a = got["continuous", False]
    assert {"ids.npy", "xpos.npy", "lens.npy", "score.npy"} <= set(a)
    for b in (got["continuous", True], got["strict", False]):
        assert sorted(a) == sorted(b)
        for f in a:
            assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes(), f
    assert a["ids.npy"].shape[0] == 8 and (a["lens.npy"] > 1).all() and (a["ids.npy"][:, 0, 0] == 1023).all()   # sos first


@pytest.mark.parametrize("engine", ["native", "python"])
@pytest.mark.parametrize("name", XL_CASES)
def test_fp16_kv_caches_keep_the_token_ids_of_the_fp32_reference(name, engine):
    """BASELINE configs[4] (half-precision storage), first stage: the self- and cross-attention K|V caches in fp16,
    all arithmetic / softmax / scores in fp32.  Parity definition for this mode (no fp16 run of the reference's
    native decoder exists: speechcatcher.py:205-210 disables it): token ids, xpos and process_idx of every block
    of the six XL fixtures EQUAL the fp32 reference's, cumulative scores within 5e-3 (on sums of magnitude 1e2..1e3; measured: 7e-5 on best hypotheses)."""
    from test_engine_spec import run_case
    if engine == "native":
        run_case(name, backend="native", score_tol=5e-3, kv_dtype="float16")
    else:
        from speechcatcher_amd.hip_backend import HipBackend
        run_case(name, backend=HipBackend("cuda:0"), device="cuda:0", score_tol=5e-3, kv_dtype="float16")


@pytest.mark.parametrize("engine", ["native", "python"])
@pytest.mark.parametrize("name", XL_CASES)
def test_fp16_ffn_weights_on_the_xl_fixtures(name, engine):
    """BASELINE configs[4], second stage: feed-forward weights in fp16 and fp16 MFMA inputs (fp32 accumulation) in the
    fused FFN kernels of all 30 encoder and 14 decoder layers, next to the fp16 K|V caches.  (The fp16 attention
    projections of the encoder, round 3's `proj_dtype`, move the near-tied beams of two of these six fixtures: the whole
    fp16 mode is held to the fp32 engine statistically instead - tests/test_gpu_baseline_size.py, 256 streams.)  Parity definition for
    this mode (no fp16 run of the reference's native decoder exists): the token ids / positions of the BEST hypothesis
    of every block of the six XL fixtures equal the fp32 reference's and its score is within 0.05 (sums of magnitude
    1e2..1e3; the operands of two of the three big GEMMs of every layer carry 2^-11 rounding) - the engine checks
    this through check_against_blocks' tolerance window for reordering among near-equal hypotheses."""
    from test_engine_spec import run_case
    kw = dict(score_tol=0.05, kv_dtype="float16", ffn_dtype="float16")
    if engine == "native":
        run_case(name, backend="native", **kw)
    else:
        from speechcatcher_amd.hip_backend import HipBackend
        run_case(name, backend=HipBackend("cuda:0"), device="cuda:0", **kw)


@pytest.mark.parametrize("engine", ["native", "python"])
@pytest.mark.parametrize("name", XL_CASES)
def test_fp16_decoder_mode_on_the_xl_fixtures(name, engine):
    """BASELINE configs[4], the decoder side (round 4): fp16 weight fragments + fp16 MFMA inputs in the decoder layer
    kernels' projections (Q|K|V, cross-attention q, both output projections), the partial products between the decoder's
    kernels stored in fp16, fp16 K|V caches; accumulation, LayerNorm, softmax, the output layer, log-softmax, CTC and
    scores fp32 (an fp16 output layer moves 7 % of the best hypotheses of 256 test streams: measured, not used).  Bar (Next 5): the hypotheses of the six XL fixtures keep their token ids and positions
    (check_against_blocks with the fp16 modes' score window of 0.05 on sums of 1e2..1e3)."""
    from test_engine_spec import run_case
    kw = dict(score_tol=0.05, kv_dtype="float16", dec_dtype="float16")
    if engine == "native":
        sb, _, _ = run_case(name, backend="native", **kw)
        assert sb.w.dec[0]["wqkv_pph"].dtype == __import__("torch").float16
    else:
        from speechcatcher_amd.hip_backend import HipBackend
        run_case(name, backend=HipBackend("cuda:0"), device="cuda:0", **kw)


@pytest.mark.parametrize("engine", ["native", "python"])
@pytest.mark.parametrize("name", XL_CASES)
def test_split16_ffn_on_the_xl_fixtures(name, engine):
    """`ffn_dtype = proj_dtype = "split16"`: the fused feed-forward kernels of all encoder and decoder layers and the
    attention projections of the encoder layers evaluate their fp32 product sums on the fp16 matrix pipe from fp16
    hi + lo splits of BOTH operands (sc_ffn_ln_s, sc_rowtile_proj_s; 22-bit products, fp32 accumulation).  Held to the fp32 engine's own bar, unrelaxed: every hypothesis of every block of the six XL
    fixtures of the reference - ids, positions, order - and the scores within the fp32 tolerance (2e-3 on sums of
    1e2..1e3; the unit test bounds the kernel itself: tests/test_gpu_ops.py test_ffn_fused_split_weights)."""
    from test_engine_spec import run_case
    if engine == "native":
        run_case(name, backend="native", ffn_dtype="split16", proj_dtype="split16")
    else:
        from speechcatcher_amd.hip_backend import HipBackend
        run_case(name, backend=HipBackend("cuda:0"), device="cuda:0", ffn_dtype="split16", proj_dtype="split16")


@pytest.mark.parametrize("engine", ["native", "python"])
def test_m_like_dimensions_head_dim_64(engine):
    """The reference's no-config defaults (d = 256, 4 heads of 64: config.M_DEFAULTS, the stand-in for the `_m`
    checkpoints of BASELINE configs[0]) with fewer layers: decoder attention at head dim 64, row panels and fused
    FFN at d = 256; beam 10 and greedy, against the oracle run on the same box."""
    import helpers
    import test_engine_spec
    from oracle.ref_port import RefPortStreaming
    from speechcatcher_amd.config import ModelConfig
    from test_engine_spec import check_against_blocks, make_batch
    helpers.CFGS["M4"] = test_engine_spec.CFGS["M4"] = ModelConfig(d_model=256, enc_heads=4, enc_layers=3, dec_heads=4,
                                                                   dec_layers=2)
    for beam in (10, 1):
        ora = RefPortStreaming(helpers.oracle_model("M4", 1234, "meanstd"), beam_size=beam, use_bbd=False)
        backend = "native"
        if engine == "python":
            from speechcatcher_amd.hip_backend import HipBackend
            backend = HipBackend("cuda:0")
        sb = make_batch("M4", 1234, "meanstd", beam, False, backend=backend, device="cuda:0", max_frames=200,
                        max_tokens=400, pcm_capacity=1 << 18)
        audio = synth.synth_audio(77, 16000 * 6)
        for pos in range(0, len(audio), 8192):
            end = min(pos + 8192, len(audio))
            fin = end >= len(audio)
            ora(audio[pos:end], is_final=fin, finalize_all=fin)
            sb.push([(0, audio[pos:end], fin)])
        ref = ora.running_hyps
        blk = {"yseq": [list(h.yseq) for h in ref], "xpos": [list(h.xpos) for h in ref],
               "score": [h.score for h in ref], "score_dec": [h.scores.get("decoder", 0.0) for h in ref],
               "score_ctc": [h.scores.get("ctc", 0.0) for h in ref], "process_idx": ora.process_idx}
        check_against_blocks(sb, 0, blk, 1e-3)      # (round 6: the north star's 1e-3; 5e-3 while head dim 64 took the six-launch decoder)
        assert len(sb.hypotheses(0)[0]["yseq"]) > 5


@pytest.mark.parametrize("form", ["split16", "float16"])
def test_packed_model_file_carries_the_optional_weight_forms(tmp_path, form):
    """A packed model file saved from weights with split-precision (w1_s / w2_s / wqkv_s / wo_s) or fp16 (.._h)
    copies: an engine loaded from the file (sc_engine_load, no Python weights behind it) gives exactly the results of the
    engine built on the in-memory tensors - and those differ from the fp32 engine's scores, i.e. the copies are used."""
    from speechcatcher_amd.config import ModelConfig, SearchConfig
    from speechcatcher_amd.native import NativeEngine, NativeStreamBatch
    from speechcatcher_amd.weights import PackedWeights
    cfg = ModelConfig(d_model=256, enc_heads=4, enc_layers=2, dec_heads=4, dec_layers=2)
    sd = synth.make_state_dict(cfg, 4321)
    mean, std = synth.stats_to_mean_std(synth.make_stats(cfg, kind="meanstd"))
    audio = synth.synth_audio(55, 16000 * 4)
    kw = dict(max_frames=200, max_tokens=300, pcm_capacity=1 << 18)

    def run(sb):
        for pos in range(0, len(audio), 10240):
            end = min(pos + 10240, len(audio))
            sb.push([(0, audio[pos:end], end >= len(audio))])
        h = sb.hypotheses(0)
        sb.close()
        return h

    w = PackedWeights(sd, cfg, "cuda:0", mean, std, ffn_dtype=form, proj_dtype=form)
    assert any(k.endswith("_s" if form == "split16" else "_h") for k in w.enc[0]) and any(
        k.endswith("_s" if form == "split16" else "_h") for k in w.dec[0])
    mem = run(NativeStreamBatch(w, 1, SearchConfig(beam_size=5, use_bbd=False), **kw))
    w.save_packed(tmp_path / "m.scpk")
    eng = NativeEngine(packed_path=str(tmp_path / "m.scpk"))
    filed = run(NativeStreamBatch(None, 1, SearchConfig(beam_size=5, use_bbd=False), engine=eng, **kw))
    assert len(mem) == len(filed) > 0 and len(mem[0]["yseq"]) > 3
    for a, b in zip(mem, filed):
        assert a["yseq"] == b["yseq"] and a["xpos"] == b["xpos"] and a["score"] == b["score"]
    ref = run(NativeStreamBatch(PackedWeights(sd, cfg, "cuda:0", mean, std), 1, SearchConfig(beam_size=5, use_bbd=False), **kw))
    assert ref[0]["yseq"] == mem[0]["yseq"]
    d = abs(ref[0]["score"] - mem[0]["score"])
    assert 0.0 < d < (2e-3 if form == "split16" else 0.05), d   # not the fp32 kernels - and as close as the form promises


def test_native_pcm_ring_compaction_and_mixed_push_submit():
    """A PCM ring that holds only ~3 chunks (the carry-over is moved to the front again and again, also while encoder
    groups of other streams are pending), every admission issued as its own encoder group (no merging) and then
    merged groups of all streams, and sc_push calls mixed into a submit / poll session - all equal the plain
    lock-step run with a large ring."""
    from test_engine_spec import make_batch
    S, chunk, n, beam = 6, 10240, 9, 5
    audio = np.stack([synth.synth_audio(70 + s, chunk * n) for s in range(S)])

    def mk(pcap):
        return make_batch("TINY", 1234, "meanstd", beam, False, n_streams=S, backend="native", max_frames=400,
                          max_tokens=400, pcm_capacity=pcap, max_chunk_samples=chunk)

    ref = mk(1 << 18)
    for k in range(n):
        ref.push([(s, audio[s, k * chunk:(k + 1) * chunk], k == n - 1) for s in range(S)])
    want = ref.hypotheses_batch(list(range(S)))
    for enc_batch in (1, S):
        sb = mk(3 * chunk + 500)
        sb.set_encoder_batch(enc_batch)
        nxt = [0] * S

        def item(s):
            k = nxt[s]
            nxt[s] += 1
            return (s, audio[s, k * chunk:(k + 1) * chunk], k == n - 1)

        sb.submit([item(s) for s in range(0, S, 2)])           # even streams: continuous
        while any(k < n for k in nxt):
            odd = [item(s) for s in range(1, S, 2) if nxt[s] < n]
            if odd:
                assert all(v is True or v is False for v in sb.push(odd).values())   # odd streams: lock-step calls in between
            done = sb.poll(1) if sb.outstanding else {}
            again = [item(s) for s in done if nxt[s] < n]
            if again:
                sb.submit(again)
        while sb.outstanding:
            sb.poll(1)
        got = sb.hypotheses_batch(list(range(S)))
        for s in range(S):
            assert [(h["yseq"], h["xpos"]) for h in got[s]] == [(h["yseq"], h["xpos"]) for h in want[s]], (enc_batch, s)
            assert all(abs(x["score"] - y["score"]) < 1e-3 for x, y in zip(got[s], want[s])), (enc_batch, s)
        assert sb.st[0].pcm_buffered < 400


def test_rccl_collectives_with_a_world_of_one():
    """The path's collectives (timing all_reduce MAX, all_gather of the final-text payload: ids + positions + length +
    score) through RCCL on the GPU with a world of ONE rank - two RCCL ranks on one device are refused
    (docs/profiles_r1-r3/r03_rccl_two_ranks_one_device.txt), and the test boxes have one GPU.  Runs in a child process (a process
    group per interpreter)."""
    import sys
    code = '''
import os, sys, socket
sys.path.insert(0, %r)
import torch, torch.distributed as dist
from speechcatcher_amd.distributed import gather_final_hypotheses, max_over_ranks, pack_hypotheses, shard_streams
torch.cuda.set_device("cuda:0")
with socket.socket() as so:
    so.bind(("127.0.0.1", 0)); port = so.getsockname()[1]
dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda:0"))
assert list(shard_streams(5, 0, 1)) == [0, 1, 2, 3, 4]
ids, pos, sc = [[1023, 5, 7], [1023], []], [[0, 3, 9], [0], []], [-1.25, 0.0, 0.0]
payload = pack_hypotheses(ids, pos, sc, 16, "cuda:0")
out = gather_final_hypotheses(payload, 4)
assert len(out) == 1 and out[0][:3] == [(ids[i], pos[i], sc[i]) for i in range(3)] and out[0][3] == ([], [], 0.0), out
assert max_over_ranks(2.5, "cuda:0") == 2.5
dist.barrier()
dist.destroy_process_group()
print("rccl ok")
''' % str(ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rccl ok" in r.stdout, r.stderr[-2000:]

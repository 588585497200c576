"""Sample-rate conversion on the GPU (csrc/resample.hip, the staging step of csrc/streams.hip): the kernel
against the fp32 spec bit for bit, a stream's samples independent of how its audio is cut into calls, a 48 kHz stream
equal to a 16 kHz stream fed the converted signal, the state rules, and the CLI on an 8 kHz file."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import resample_ref as ref
from speechcatcher_amd import synth

pytestmark = pytest.mark.gpu

RATES = tuple(r for r in ref.RATES if r != 16000)


def tile_outputs(L):
    """outputs per workgroup of resample_kernel: 256 while the table lives in LDS (L <= 4), else four periods of L"""
    return 256 if L <= 4 else 4 * L


@functools.lru_cache(maxsize=None)
def lib_table(rate):
    from speechcatcher_amd import _abi
    lib = _abi.load()
    L, M, Wc = ref.params(rate)
    coef = np.zeros((L, 2 * Wc), np.float32)
    assert lib.sc_resample_design(rate, None, None, None, coef.ctypes.data_as(C.POINTER(C.c_float))) == 0
    coef.setflags(write=False)
    return coef


def gpu_resample(x, rate):
    from speechcatcher_amd.hip_backend import resample
    y = resample(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), rate)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("rate", RATES)
def test_kernel_equals_the_fp32_spec_bit_for_bit(rate):
    L, M, Wc = ref.params(rate)
    coef = lib_table(rate)
    K = 2 * Wc
    tile = tile_outputs(L)
    n_cross = next(n for n in range(1, 4 * tile) if ref.out_count(rate, n, True) > tile)
    assert tile < ref.out_count(rate, n_cross, True) <= tile + 2   # one past a tile boundary (two where every sample gives two)
    lengths = [1, Wc - 1, Wc, Wc + 1, 997, n_cross]
    if L > 4:
        lengths.append(2 * M + 7)                    # the phase index wraps twice
    rng = np.random.RandomState(rate)
    for n in lengths:
        signals = {"noise": rng.randn(n).astype(np.float32), "impulse0": np.zeros(n, np.float32),
                   "impulse_last": np.zeros(n, np.float32), "ones": np.ones(n, np.float32)}
        signals["impulse0"][0] = 1.0
        signals["impulse_last"][-1] = 1.0
        for name, x in signals.items():
            got, want = gpu_resample(x, rate), ref.eval_f32(x, rate, coef)
            assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (ref.out_count(rate, n, True),)
            assert got.tobytes() == want.tobytes(), (rate, n, name, int(np.argmax(got != want)))
            if name == "ones" and n == 997:
                m = np.arange(len(got), dtype=np.int64)
                n0 = (m * M) // L
                inner = (n0 - Wc + 1 >= 0) & (n0 + Wc <= n - 1)
                assert inner.sum() > 50
                dev = np.abs(got[inner].astype(np.float64) - 1.0).max()
                print(f"rate {rate}: all-ones deviates from 1 by {dev:.2e} (bound {K * 2.0 ** -24:.2e})")
                assert dev <= K * 2.0 ** -24


def _tiny_batch(n_streams, **kw):
    from test_engine_spec import make_batch
    args = dict(n_streams=n_streams, max_frames=160, max_tokens=128, pcm_capacity=1 << 16, strict_reference=False)
    args.update(kw)
    return make_batch("TINY", 1234, "meanstd", 5, False, backend="native", **args)


def _twin_calls(rate, calls):
    """the calls [(n_in, final)] of a stream at `rate` -> the 16 kHz sample counts the spec gives each of them"""
    out, n_in, n_out = [], 0, 0
    for n, fin in calls:
        n_in += n
        total = ref.out_count(rate, n_in, fin)
        out.append(total - n_out)
        n_out = total
    return out


def _state(sb, s):
    hy = sb.hypotheses(s)
    enc = sb.encoder_buffer(s)
    return ([(h["yseq"], h["xpos"], h["score"], h["score_dec"], h["score_ctc"]) for h in hy],
            b"" if enc is None else enc.tobytes())


@pytest.mark.parametrize("rate", [8000, 44100, 48000])
def test_stream_samples_do_not_depend_on_the_call_cuts(rate):
    """0.7 s of noise at `rate` in one call, in 640 ms chunks and in a ragged split (calls of 1 sample, of fewer than Wc
    samples, of a prime length), each non-final and closed by a final call.  Every such stream has a 16 kHz twin in the same
    batch that gets sc_resample of the WHOLE signal cut at the spec's per-call output counts: after every call both have
    buffered the same number of samples with the same bytes - the tail of the whole-signal conversion -, the same encoder
    output and the same hypotheses."""
    Wc = ref.params(rate)[2]
    n = int(0.7 * rate)
    x = (0.3 * np.random.RandomState(rate + 7).randn(n)).astype(np.float32)
    whole = gpu_resample(x, rate)
    assert whole.tobytes() == ref.eval_f32(x, rate, lib_table(rate)).tobytes()
    chunk = int(0.64 * rate)
    splits = [[(n, False), (0, True)],
              [(chunk, False), (n - chunk, True)],
              [(1, False), (Wc - 3, False), (997, False), (3, False), (n // 2, False), (n - n // 2 - 998 - Wc, True)]]
    for calls in splits:
        assert sum(c for c, _ in calls) == n and calls[-1][1]
    sb = _tiny_batch(6)
    for i in range(3):
        sb.set_input_rate(i, rate)
        assert sb.input_rate(i) == rate and sb.input_rate(3 + i) == 16000
    twins = [_twin_calls(rate, calls) for calls in splits]
    pos_in, pos_out, seen_frames = [0, 0, 0], [0, 0, 0], 0
    for k in range(max(len(c) for c in splits)):
        items = []
        for i, calls in enumerate(splits):
            if k < len(calls):
                n_in, fin = calls[k]
                items.append((i, x[pos_in[i]:pos_in[i] + n_in], fin))
                items.append((3 + i, whole[pos_out[i]:pos_out[i] + twins[i][k]], fin))
                pos_in[i] += n_in
                pos_out[i] += twins[i][k]
        out = sb.push(items)
        for i, calls in enumerate(splits):
            if k >= len(calls):
                continue
            assert out[i] == out[3 + i], (rate, i, k)
            buffered = sb.st[i].pcm_buffered
            assert buffered == sb.st[3 + i].pcm_buffered, (rate, i, k)
            buf = sb.waveform_buffer(i)
            assert buf.tobytes() == sb.waveform_buffer(3 + i).tobytes(), (rate, i, k)
            if not calls[k][1]:   # (a final call hands everything to the frontend)
                assert buf.tobytes() == whole[pos_out[i] - buffered:pos_out[i]].tobytes(), (rate, i, k)
            assert _state(sb, i) == _state(sb, 3 + i), (rate, i, k)
            seen_frames = max(seen_frames, sb.st[i].T_enc)
    assert pos_out == [len(whole)] * 3 and seen_frames > 0        # the encoder did run


def _equivalence_feeds(rate=48000, seconds=1.5, n_calls=5):
    n = int(seconds * rate)
    x = synth.synth_audio(21, n).astype(np.float32)
    whole = gpu_resample(x, rate)
    step = n // n_calls
    calls = [(step, k == n_calls - 1) for k in range(n_calls)]
    counts = _twin_calls(rate, calls)
    a, b, pa, pb = [], [], 0, 0
    for (n_in, fin), n16 in zip(calls, counts):
        a.append((x[pa:pa + n_in], fin))
        b.append((whole[pb:pb + n16], fin))
        pa += n_in
        pb += n16
    assert pb == len(whole)
    return a, b


def test_a_48k_stream_equals_a_16k_stream_fed_the_converted_signal_push():
    a, b = _equivalence_feeds()
    sb = _tiny_batch(2)
    sb.set_input_rate(0, 48000)
    for (xa, fin), (xb, _) in zip(a, b):
        out = sb.push([(0, xa, fin), (1, xb, fin)])
        assert out[0] == out[1]
        sa, sbb = _state(sb, 0), _state(sb, 1)
        assert sa == sbb
    assert len(sa[0]) > 0 and len(sa[0][0][0]) > 3 and len(sa[1]) > 0       # it did decode something


def _run_queued(sb, feeds, depth=2):
    """submit ahead up to `depth` chunks per stream, poll one reply at a time -> {stream: [(status, hypotheses)]} and
    the final encoder buffers"""
    sub = {s: 0 for s in feeds}
    rep = {s: [] for s in feeds}
    while any(len(rep[s]) < len(feeds[s]) for s in feeds):
        for _ in range(depth):
            items = []
            for s, chunks in feeds.items():
                if sub[s] - len(rep[s]) < depth and sub[s] < len(chunks):
                    items.append((s, chunks[sub[s]][0], chunks[sub[s]][1]))
                    sub[s] += 1
            if items:
                sb.submit(items)
        got = sb.poll(1)
        assert got
        for s, has in got.items():
            assert not isinstance(has, Exception), (s, has)
            rep[s].append((bool(has), _state(sb, s)[0]))
    return rep, {s: _state(sb, s)[1] for s in feeds}


def test_a_48k_stream_equals_a_16k_stream_fed_the_converted_signal_queued():
    """... with sc_submit / sc_poll at queue depth 2, next to two untouched 16 kHz streams whose replies equal those of a
    run without the 48 kHz stream"""
    a, b = _equivalence_feeds()
    others = {s: [(synth.synth_audio(30 + s, 8000 * 5)[k * 8000:(k + 1) * 8000], k == 4) for k in range(5)] for s in (2, 3)}
    sb = _tiny_batch(4)
    sb.set_queue_depth(2)
    sb.set_input_rate(0, 48000)
    rep, enc = _run_queued(sb, {0: a, 1: b, 2: others[2], 3: others[3]})
    assert rep[0] == rep[1] and enc[0] == enc[1] and len(enc[0]) > 0
    assert any(len(h) and len(h[0][0]) > 3 for _, h in rep[0])
    base = _tiny_batch(4)
    base.set_queue_depth(2)
    rep0, enc0 = _run_queued(base, {1: b, 2: others[2], 3: others[3]})
    for s in (1, 2, 3):
        assert rep[s] == rep0[s] and enc[s] == enc0[s], s


def test_state_rules():
    from speechcatcher_amd.engine import EngineError
    rate = 8000
    sb = _tiny_batch(3, max_chunk_samples=8192)
    x = (0.3 * np.random.RandomState(3).randn(6000)).astype(np.float32)
    whole = gpu_resample(x[:2000], rate)
    # an unsupported rate; a stream with buffered audio; a stream with an outstanding chunk
    with pytest.raises(EngineError, match="unsupported"):
        sb.set_input_rate(0, 7999)
    sb.set_input_rate(0, rate)
    sb.push([(0, x[:150], False)])
    n16 = ref.out_count(rate, 150, False)
    assert sb.st[0].pcm_buffered == n16 and sb.waveform_buffer(0).tobytes() == whole[:n16].tobytes()
    with pytest.raises(EngineError, match="buffered"):
        sb.set_input_rate(0, 48000)
    sb.submit([(1, x[:150], False)])
    with pytest.raises(EngineError, match="outstanding"):
        sb.set_input_rate(1, rate)
    while sb.outstanding:
        sb.poll(1)
    # device-resident PCM is 16 kHz by definition
    with pytest.raises(EngineError, match="16 kHz only"):
        sb.push([(0, 100, False)], pcm_resident=True)
    # reset keeps the rate and the first output equals a fresh stream's
    sb.reset(0)
    assert sb.input_rate(0) == rate and sb.st[0].pcm_buffered == 0
    sb.push([(0, x[:150], False)])
    assert sb.waveform_buffer(0).tobytes() == whole[:n16].tobytes()
    # an over-long call fails that stream alone (8192 + 16 hops = 10752 samples at either rate); the stream then behaves
    # like a fresh one, its neighbour is untouched
    sb.reset(1)
    sb.set_input_rate(1, 16000)
    y = synth.synth_audio(5, 4000)
    lim = 8192 + 16 * sb.cfg.hop_length
    out = sb.push([(0, np.zeros(lim + 1, np.float32), False), (1, y, False)], isolate_faults=True)
    assert isinstance(out[0], EngineError) and "max_chunk_samples" in str(out[0]) and not isinstance(out[1], Exception)
    assert sb.st[1].pcm_buffered > 0 and sb.input_rate(0) == rate and sb.st[0].pcm_buffered == 0
    sb.push([(0, x[:150], False)])
    assert sb.waveform_buffer(0).tobytes() == whole[:n16].tobytes()
    # ... and so does a call whose OUTPUT is too long (8 kHz doubles the count)
    sb.reset(0)
    n_in = lim // 2 + 40
    assert n_in <= lim < ref.out_count(rate, n_in, False)
    out = sb.push([(0, np.zeros(n_in, np.float32), False)], isolate_faults=True)
    assert isinstance(out[0], EngineError) and "max_chunk_samples" in str(out[0])
    sb.push([(0, x[:150], False)])
    assert sb.waveform_buffer(0).tobytes() == whole[:n16].tobytes()
    # eight distinct rates per handle: a ninth is refused
    sb.reset(2)
    for r in (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000):
        sb.set_input_rate(2, r)
    with pytest.raises(EngineError, match="8 distinct"):
        sb.set_input_rate(2, 36000)
    sb.set_input_rate(2, 11025)     # a known rate is still fine


def test_cli_decodes_an_8k_wav(tmp_path):
    import subprocess
    import sys
    import wave
    from conftest import ROOT
    from speechcatcher_amd.config import TINY
    mdir = synth.write_model_dir(tmp_path / "tiny", TINY, seed=1234, stats_kind="meanstd")
    t = np.arange(5 * 16000) / 16000.0
    x16 = synth.synth_audio(41, len(t)) * 8000 + 4000 * np.sin(2 * np.pi * 440 * t)
    x8 = x16[::2].astype(np.int16)                 # decimated: a mono 8 kHz recording
    wav = tmp_path / "rec8k.wav"
    with wave.open(str(wav), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(8000)
        f.writeframes(x8.tobytes())
    res = subprocess.run([sys.executable, "-m", "speechcatcher_amd", "-m", str(mdir), "-b", "3", "--quiet", "--no-progress",
                          str(wav)], cwd=str(ROOT), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads((tmp_path / "rec8k.wav.json").read_text())
    assert (tmp_path / "rec8k.wav.txt").read_text() == out["complete_text"]
    stereo = tmp_path / "stereo.wav"
    with wave.open(str(stereo), "wb") as f:
        f.setnchannels(2); f.setsampwidth(2); f.setframerate(8000)
        f.writeframes(x8[:1000].tobytes())
    res = subprocess.run([sys.executable, "-m", "speechcatcher_amd", "-m", str(mdir), str(stereo)], cwd=str(ROOT),
                         capture_output=True, text=True)
    assert res.returncode != 0 and "16 kHz mono" in (res.stderr + res.stdout)

"""Wire-format audio in on the GPU (csrc/pcm.hip: sc_pcm_decode; hip_backend.decode_pcm / decode_recording; the CLI's
reader) against the contract of tests/pcm_ref.py: fp32 outputs compared as uint32, every integer of the level equal, the
second copy of the level the same, nothing written behind dst + n.  No case is excluded and there is no tolerance.

Values compared on an MI355X: all 256 codes of u8 / mu-law / A-law, all 65 536 s16 values under both
scales, the s24 edges and 4096 random s24 codes, f32 with NaN / inf / denormals, 432 jobs over every format x channels
{1, 2, 3, 8} x every channel and the mix x byte offsets 0..3 and 288 jobs over every format x n in {0, 1, 255, 256, 257,
1025} x byte offsets 0..3: bits equal."""
from ctypes import c_int32 as C_int32, c_uint8 as C_uint8, c_void_p as C_void_p

import numpy as np
import pytest
import torch

import pcm_ref as R

pytestmark = pytest.mark.gpu

GUARD = 4
SENTINEL = 0x7FC0DEAD
NS = (0, 1, 255, 256, 257, 1025)   # the tile edges of a 256-thread loop


@pytest.fixture(scope="module")
def be():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend("cuda:0", use_graphs=False)


def _scales(fmt):
    return (R.SCALE_FULL, R.SCALE_SERVER) if R.BITS.get(fmt) == 15 else (R.SCALE_FULL,)


def _check(be, jobs, names):
    """jobs as hip_backend.decode_pcm takes them, ONE launch; every job against the contract"""
    got, lv, after = be.decode_pcm(jobs, guard=GUARD)
    compared = 0
    for name, (src, off, fmt, ch, sel, scale, n, prev), g, l, a in zip(names, jobs, got, lv, after):
        chunk = bytes(src)[off: off + n * R.bytes_per_frame(fmt, ch)]
        want = R.decode(chunk, fmt, ch, sel, scale)
        bits = g.view(np.uint32)
        assert bits.size == n + GUARD and (bits[n:] == SENTINEL).all(), f"{name}: written behind dst + n"
        bad = np.nonzero(bits[:n] != want.view(np.uint32))[0]
        assert bad.size == 0, (name, int(bad[0]), hex(int(bits[bad[0]])), hex(int(want.view(np.uint32)[bad[0]])))
        wl = R.level(chunk, fmt, ch, sel, scale, prev)
        assert l == wl, (name, l, wl)
        assert a == l, (name, a, l)
        compared += n
    return compared


def test_every_code_of_the_8_bit_formats(be):
    codes = bytes(range(256))
    jobs, names = [], []
    for fmt in (R.U8, R.MULAW, R.ALAW):
        for scale in _scales(fmt):
            jobs.append((codes, 0, fmt, 1, 0, scale, 256, None))
            names.append(f"fmt {fmt} scale {scale}")
    assert _check(be, jobs, names) == 5 * 256


def test_every_s16_value_under_both_scales(be):
    codes = np.arange(-32768, 32768, dtype="<i2").tobytes()
    jobs = [(codes, 0, R.S16LE, 1, 0, scale, 65536, None) for scale in _scales(R.S16LE)]
    assert _check(be, jobs, ["s16 full", "s16 server"]) == 2 * 65536
    # ... which are the host conversions they replace, bit for bit
    from speechcatcher_amd.server_session import scale_server_pcm
    got, _, _ = be.decode_pcm(jobs, guard=0)
    v = np.arange(-32768, 32768, dtype=np.int16)
    assert (got[0].view(np.uint32) == (v.astype(np.float32) / 32768.0).view(np.uint32)).all()
    assert (got[1].view(np.uint32) == scale_server_pcm(v).view(np.uint32)).all()


def _s24(vals):
    return b"".join(int(v).to_bytes(3, "little", signed=True) for v in vals)


def test_s24_edges_and_random(be):
    lo, hi = -(1 << 23), (1 << 23) - 1
    edges = [lo, lo + 1, hi, hi - 1, -1, 0, 1, 255, 256, -256, 65535, 65536, -65536, hi, hi, lo, lo, lo]
    rng = np.random.default_rng(24)
    rand = _s24(rng.integers(lo, hi + 1, 4096))
    jobs, names = [], []
    for ch in (1, 2, 3):
        for sel in list(range(ch)) + [R.MIX]:
            e = _s24(edges)
            jobs.append((e, 0, R.S24LE, ch, sel, R.SCALE_FULL, len(edges) // ch, None))
            names.append(f"s24 edges ch {ch} sel {sel}")
    # the mix whose sum passes 2^24: rounding m to fp32 before the division would differ (C = 3)
    jobs.append((_s24([hi, hi, 7, hi, hi, 9, hi, hi, 11] * 2), 0, R.S24LE, 3, R.MIX, R.SCALE_FULL, 6, None))
    names.append("s24 mix above 2^24")
    for ch, sel in ((1, 0), (3, R.MIX), (8, R.MIX), (8, 5)):
        jobs.append((rand, 0, R.S24LE, ch, sel, R.SCALE_FULL, 4096 // ch, None))
        names.append(f"s24 random ch {ch} sel {sel}")
    _check(be, jobs, names)


def test_f32_specials_select_and_mix(be):
    special = np.array([np.nan, np.inf, -np.inf, 1e-41, -1e-45, 0.0, -0.0, 1.0, -1.0, 3.4e38, 3.4e38, 1e-38, 0.1, 0.2, 0.3, -0.7],
                       np.float32)
    bits = special.view(np.uint32).copy()
    bits[0] = 0xFFC12345   # a NaN with a sign and a payload: a selected channel passes it through
    rng = np.random.default_rng(32)
    rand = rng.standard_normal(2048).astype(np.float32)
    rand[rng.integers(0, 2048, 32)] = special[rng.integers(0, special.size, 32)]
    jobs, names = [], []
    for data, tag in ((bits.tobytes(), "special"), (rand.tobytes(), "random"), (rng.bytes(4096), "bytes")):
        for ch in (1, 2, 3, 8):
            for sel in list(range(ch)) + [R.MIX]:
                jobs.append((data, 0, R.F32, ch, sel, R.SCALE_FULL, len(data) // 4 // ch, None))
                names.append(f"f32 {tag} ch {ch} sel {sel}")
    _check(be, jobs, names)
    got, lv, _ = be.decode_pcm([(bits.tobytes(), 0, R.F32, 1, 0, R.SCALE_FULL, 16, None)])
    assert got[0].view(np.uint32)[0] == 0xFFC12345
    assert lv[0] == R.ZERO_LEVEL


def test_channels_sizes_and_byte_offsets(be):
    rng = np.random.default_rng(8)
    blob = rng.bytes(1025 * 8 * 4 + 3)
    # every extreme of every format occurs among the random codes often enough at 1 byte; s16 / s24 get theirs planted
    blob = bytearray(blob)
    for i in range(0, 4000, 97):
        blob[i:i + 3] = b"\xff\xff\x7f"
        blob[i + 40:i + 43] = b"\x00\x00\x80"
    blob = bytes(blob)
    jobs, names = [], []
    for fmt in R.FORMATS:
        for ch in (1, 2, 3, 8):
            for sel in list(range(ch)) + [R.MIX]:
                for off in range(4):
                    scale = _scales(fmt)[(off + ch) % len(_scales(fmt))]
                    jobs.append((blob, off, fmt, ch, sel, scale, 257, None))
                    names.append(f"fmt {fmt} ch {ch} sel {sel} off {off} scale {scale}")
    assert len(jobs) == 432
    _check(be, jobs, names)
    jobs, names = [], []
    for fmt in R.FORMATS:
        for n in NS:
            for off in range(4):
                for ch, sel in ((3, R.MIX), (2, 1)):
                    jobs.append((blob, off, fmt, ch, sel, R.SCALE_FULL, n, None))
                    names.append(f"fmt {fmt} n {n} off {off} ch {ch} sel {sel}")
    assert len(jobs) == 288
    _check(be, jobs, names)


def test_the_level_carries_between_jobs_and_restart_clears_it(be):
    rng = np.random.default_rng(5)
    for fmt, ch, sel in ((R.S16LE, 2, R.MIX), (R.MULAW, 2, 1), (R.S24LE, 3, R.MIX), (R.U8, 1, 0)):
        bpf = R.bytes_per_frame(fmt, ch)
        n1, n2 = 300, 513
        data = rng.bytes((n1 + n2) * bpf)
        first = R.level(data[:n1 * bpf], fmt, ch, sel)
        whole = R.level(data, fmt, ch, sel)
        jobs = [(data, 0, fmt, ch, sel, 0, n1 + n2, None),          # one job
                (data, n1 * bpf, fmt, ch, sel, 0, n2, first),        # the second of two chained ones
                (data, n1 * bpf, fmt, ch, sel, 0, n2, None),         # the same span starting an utterance
                (data, 0, fmt, ch, sel, 0, 0, first)]                # n == 0 rewrites the level unchanged
        _check(be, jobs, ["whole", "chained", "restart", "empty"])
        _, lv, _ = be.decode_pcm(jobs)
        assert lv[0] == lv[1] == whole
        assert lv[2] == R.level(data[n1 * bpf:], fmt, ch, sel) and lv[2] != whole
        assert lv[3] == first
        # ... and through the device: the level the first launch left is what the second is handed
        _, l1, _ = be.decode_pcm([(data, 0, fmt, ch, sel, 0, n1, None)])
        _, l2, _ = be.decode_pcm([(data, n1 * bpf, fmt, ch, sel, 0, n2, l1[0])])
        assert l2[0] == whole


MALFORMED = {
    "null src": lambda j: setattr(j, "src", None),
    "null dst": lambda j: setattr(j, "dst", None),
    "null level": lambda j: setattr(j, "level", None),
    "format 6": lambda j: setattr(j, "format", 6),
    "format -1": lambda j: setattr(j, "format", -1),
    "channels 0": lambda j: setattr(j, "channels", 0),
    "channels 9": lambda j: setattr(j, "channels", 9),
    "channel == channels": lambda j: setattr(j, "channel", j.channels),
    "channel -2": lambda j: setattr(j, "channel", -2),
    "scale 2": lambda j: setattr(j, "scale", 2),
    "scale -1": lambda j: setattr(j, "scale", -1),
    "server scale with s24": lambda j: (setattr(j, "format", R.S24LE), setattr(j, "scale", R.SCALE_SERVER)),
    "server scale with u8": lambda j: (setattr(j, "format", R.U8), setattr(j, "scale", R.SCALE_SERVER)),
    "server scale with f32": lambda j: (setattr(j, "format", R.F32), setattr(j, "scale", R.SCALE_SERVER)),
    "n -1": lambda j: setattr(j, "n", -1),
    "offset -1": lambda j: setattr(j, "offset", -1),
}


def test_a_malformed_job_writes_nothing_and_its_neighbours_are_served(be):
    rng = np.random.default_rng(13)
    data = rng.bytes(300 * 8 * 4)
    kinds = list(MALFORMED)
    jobs = [(data, 1, R.S16LE, 2, R.MIX, 0, 300, None)]
    for _ in kinds:
        jobs.append((data, 0, R.S16LE, 2, 0, 0, 300, None))        # made malformed below
        jobs.append((data, 1, R.S16LE, 2, R.MIX, 0, 300, None))

    def tweak(k, j):
        if k % 2 == 1:
            MALFORMED[kinds[k // 2]](j)

    got, lv, after = be.decode_pcm(jobs, tweak=tweak, guard=GUARD)
    want = R.decode(data[1:1 + 1200], R.S16LE, 2, R.MIX)
    wl = R.level(data[1:1 + 1200], R.S16LE, 2, R.MIX)
    q = int(np.array([-7, -7], np.int32).view(np.int64)[0])   # a level handed over as int32 -7 throughout
    untouched = dict(frames=q, clipped=q, sum_abs=q, peak=-7, full_scale=-7)
    for k in range(len(jobs)):
        bits = got[k].view(np.uint32)
        if k % 2 == 1:
            name = kinds[k // 2]
            assert (bits == SENTINEL).all(), f"{name}: wrote samples"
            assert lv[k] == untouched and after[k] == untouched, (name, lv[k], after[k])
        else:
            assert (bits[:300] == want.view(np.uint32)).all() and (bits[300:] == SENTINEL).all(), k
            assert lv[k] == wl and after[k] == wl, k


def test_job_table_arguments(be):
    lib = be.lib
    assert lib.sc_pcm_decode(None, 0, None) == 0
    assert lib.sc_pcm_decode(None, 1, None) == -1 and b"null job table" in lib.sc_last_error()
    assert lib.sc_pcm_decode(None, -1, None) == -1
    t = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    assert lib.sc_pcm_decode(t.data_ptr(), 65536, None) == -1 and b"SC_PCM_MAX_JOBS" in lib.sc_last_error()


def test_a_whole_recording_in_jobs_of_any_size(be):
    """decode_recording (the CLI's path): the samples and the level do not depend on how the recording is cut into jobs"""
    from speechcatcher_amd import pcm
    from speechcatcher_amd.hip_backend import decode_recording
    rng = np.random.default_rng(77)
    data = rng.bytes(5000 * 2)
    want, wl = R.decode(data, R.MULAW, 2, R.MIX), R.level(data, R.MULAW, 2, R.MIX)
    for per_job in (1 << 16, 1024, 999):
        x, lv = decode_recording(data, pcm.MULAW, 2, pcm.MIX, frames_per_job=per_job)
        assert (x.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all(), per_job
        assert lv == wl, (per_job, lv, wl)
    x, lv = decode_recording(b"", pcm.S16LE, 1, 0)
    assert x.numel() == 0 and lv == R.level(b"", R.S16LE, 1, 0)


# ---- stream level ----------------------------------------------------------------------------------------------------
CHUNK_MS = 640
N_CHUNKS = 7
KW = dict(max_frames=160, max_tokens=200, pcm_capacity=1 << 17, strict_reference=False)
# name -> (format, channels, channel, scale, rate)
CASES = {
    "s16-full": (R.S16LE, 1, 0, R.SCALE_FULL, 16000),
    "s16-server": (R.S16LE, 1, 0, R.SCALE_SERVER, 16000),
    "mulaw-stereo-ch1-8k": (R.MULAW, 2, 1, R.SCALE_FULL, 8000),
    "s24-3ch-mix": (R.S24LE, 3, R.MIX, R.SCALE_FULL, 16000),
}


def _tiny_batch(n_streams, cfg="TINY", **kw):
    from test_engine_spec import make_batch
    args = dict(KW, n_streams=n_streams)
    args.update(kw)
    return make_batch(cfg, 1234, "meanstd", 5, True, backend="native", **args)


def _state(sb, s):
    hy = sb.hypotheses(s)
    enc = sb.encoder_buffer(s)
    return ([(h["yseq"], h["xpos"], h["score"], h["score_dec"], h["score_ctc"]) for h in hy],
            b"" if enc is None else enc.tobytes())


def _encode(x, fmt):
    """a float signal in +-1 -> the codes of one channel (uint8 [n, code bytes])"""
    from speechcatcher_amd import synth  # noqa: F401
    if fmt == R.S16LE:
        return np.clip(np.round(x * 32767), -32768, 32767).astype("<i2").view(np.uint8).reshape(-1, 2)
    if fmt == R.S24LE:
        v = np.clip(np.round(x * 8388607), -8388608, 8388607).astype("<i4")
        return v.view(np.uint8).reshape(-1, 4)[:, :3].copy()
    table = np.array([R.ulaw_value(b) if fmt == R.MULAW else R.alaw_value(b) for b in range(256)], np.float64)
    return np.abs(table[None, :] - (x * 32768)[:, None]).argmin(axis=1).astype(np.uint8).reshape(-1, 1)


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def case(request):
    """per case, computed once: the chunks' bytes (every channel another signal, peaks that clip planted in the selected
    one), the contract's samples and the contract's cumulative level after every chunk"""
    from speechcatcher_amd import synth
    fmt, ch, sel, scale, rate = CASES[request.param]
    n = rate * CHUNK_MS // 1000
    total = n * N_CHUNKS
    chans = []
    for c in range(ch):
        x = synth.synth_audio(60 + c, total * 16000 // rate)[::16000 // rate][:total].astype(np.float64)
        x = x / max(1e-9, np.abs(x).max()) * (0.5 if ch > 1 else 0.9)
        x[100 + c::5000] = 1.5 if c % 2 == 0 else -1.5          # clipped samples
        chans.append(_encode(x, fmt))
    data = np.concatenate(chans, axis=1).tobytes()               # interleaved
    bpf = R.bytes_per_frame(fmt, ch)
    assert len(data) == total * bpf
    chunks = [data[k * n * bpf:(k + 1) * n * bpf] for k in range(N_CHUNKS)]
    floats = [R.decode(c, fmt, ch, sel, scale) for c in chunks]
    levels, lv = [], None
    for c in chunks:
        lv = R.level(c, fmt, ch, sel, scale, lv)
        levels.append(lv)
    assert levels[-1]["clipped"] > 0 and levels[-1]["peak"] > 0
    return dict(name=request.param, fmt=fmt, ch=ch, sel=sel, scale=scale, rate=rate, n=n, bpf=bpf, data=data, chunks=chunks,
                floats=floats, levels=levels)


def _ring(sb):
    """the device PCM ring [S, capacity] through sc_streams_pcm"""
    import ctypes as C
    cap = C.c_long()
    ptr = sb.lib.sc_streams_pcm(sb.handle, C.byref(cap))

    class _View:
        __cuda_array_interface__ = {"shape": (sb.S, cap.value), "typestr": "<f4", "data": (int(ptr), False), "version": 2}

    torch.cuda.synchronize()
    return torch.as_tensor(_View(), device="cuda:0").cpu().numpy().copy()


def _setup(sb, case, floats=(0,), coded=(1,)):
    for s in tuple(floats) + tuple(coded):
        if case["rate"] != 16000:
            sb.set_input_rate(s, case["rate"])
    for s in coded:
        sb.set_input_format(s, case["fmt"], case["ch"], case["sel"], case["scale"])
        assert sb.input_format(s) == (case["fmt"], case["ch"], case["sel"], case["scale"])
    for s in floats:
        assert sb.input_format(s)[:2] == (R.F32, 1)


def test_a_coded_stream_equals_a_float_stream_fed_the_decoded_samples_push(case):
    """lock-step: stream 0 floats (pcm.decode of the bytes), stream 1 the bytes, stream 2 other float audio, in ONE admission;
    then stream 3 the same bytes cut into calls of other lengths"""
    from speechcatcher_amd import pcm, synth
    other = synth.synth_audio(33, 10240 * N_CHUNKS)
    sb = _tiny_batch(4)
    _setup(sb, case, floats=(0,), coded=(1, 3))
    for k in range(N_CHUNKS):
        fin = k == N_CHUNKS - 1
        assert pcm.decode(case["chunks"][k], case["fmt"], case["ch"], case["sel"], case["scale"]).tobytes() == case["floats"][k].tobytes()
        out = sb.push([(0, case["floats"][k], fin), (1, case["chunks"][k], fin), (2, other[k * 10240:(k + 1) * 10240], fin)])
        assert out[0] == out[1], (case["name"], k)
        assert _state(sb, 0) == _state(sb, 1), (case["name"], k)
        assert sb.waveform_buffer(0).tobytes() == sb.waveform_buffer(1).tobytes()
        assert sb.input_level(1) == case["levels"][k], (case["name"], k, sb.input_level(1), case["levels"][k])
        assert sb.input_level(0) == R.ZERO_LEVEL and sb.input_level(2) == R.ZERO_LEVEL
    st = _state(sb, 1)
    assert len(st[0]) > 0 and len(st[0][0][0]) > 3 and len(st[1]) > 0       # it did decode something
    # the same bytes in ragged calls: 1 frame, a prime count, the rest - the ring holds the same samples
    bpf, total = case["bpf"], case["n"] * N_CHUNKS
    cuts, pos = [1, 997, 3, case["n"] // 2], 0
    rest = total - sum(cuts)
    lim = 8000          # frames per call, within max_chunk_samples at either rate
    cuts += [lim] * (rest // lim) + ([rest % lim] if rest % lim else [])
    for i, c in enumerate(cuts):
        sb.push([(3, case["data"][pos * bpf:(pos + c) * bpf], i == len(cuts) - 1)])
        pos += c
    assert pos == total and sb.input_level(3) == case["levels"][-1]
    ring = _ring(sb)
    n16 = total * 16000 // case["rate"]
    assert ring[0, :n16].tobytes() == ring[1, :n16].tobytes() == ring[3, :n16].tobytes(), case["name"]
    if case["rate"] == 16000:
        assert ring[1, :n16].tobytes() == np.concatenate(case["floats"]).tobytes()
    assert np.abs(ring[1, :n16]).max() > 0.1
    # after the final the level starts over; reset keeps the format
    sb.reset(1)
    assert sb.input_format(1) == (case["fmt"], case["ch"], case["sel"], case["scale"]) and sb.input_level(1) == R.ZERO_LEVEL
    sb.push([(1, case["chunks"][0], False)])
    assert sb.input_level(1) == case["levels"][0]
    # ... also without a reset in between (hosts that keep the reference's no-reset-after-final): the first job after a
    # final chunk carries restart, the one after it carries the level on
    args = (case["fmt"], case["ch"], case["sel"], case["scale"])
    sb.reset(3)
    sb.push([(3, case["chunks"][1], True)])
    assert sb.input_level(3) == R.level(case["chunks"][1], *args)
    sb.push([(3, case["chunks"][2], False)])                                   # no reset behind the final
    first = R.level(case["chunks"][2], *args)
    assert sb.input_level(3) == first, (case["name"], sb.input_level(3), first)
    sb.push([(3, case["chunks"][3], False)])
    assert sb.input_level(3) == R.level(case["chunks"][3], *args, prev=first)


def _run_queued(sb, feeds, level_of=(), depth=2):
    """submit ahead up to `depth` chunks per stream, poll one reply at a time -> {stream: [(status, hypotheses)]}, the
    final encoder buffers and {stream: [level after every reply]}"""
    sub = {s: 0 for s in feeds}
    rep = {s: [] for s in feeds}
    lv = {s: [] for s in level_of}
    while any(len(rep[s]) < len(feeds[s]) for s in feeds):
        for _ in range(depth):
            items = []
            for s, chunks in feeds.items():
                if sub[s] - len(rep[s]) < depth and sub[s] < len(chunks):
                    items.append((s, chunks[sub[s]][0], chunks[sub[s]][1]))
                    sub[s] += 1
            if items:
                sb.submit_raw(items)
        got = sb.poll(1)
        assert got
        for s, has in got.items():
            assert not isinstance(has, Exception), (s, has)
            rep[s].append((bool(has), _state(sb, s)[0]))
            if s in lv:
                lv[s].append(sb.input_level(s))       # (the stream's next chunk is already staged)
    return rep, {s: _state(sb, s)[1] for s in feeds}, lv


def test_a_coded_stream_equals_a_float_stream_fed_the_decoded_samples_queued(case):
    """sc_submit_raw / sc_poll at queue depth 2: the replies of the twins are equal, the level after every reply is the
    contract's over the bytes of the REPORTED chunks"""
    fins = [k == N_CHUNKS - 1 for k in range(N_CHUNKS)]
    sb = _tiny_batch(2)
    sb.set_queue_depth(2)
    _setup(sb, case)
    rep, enc, lv = _run_queued(sb, {0: list(zip(case["floats"], fins)), 1: list(zip(case["chunks"], fins))}, level_of=(1,))
    assert rep[0] == rep[1] and enc[0] == enc[1] and len(enc[0]) > 0, case["name"]
    assert lv[1] == case["levels"], case["name"]
    assert any(len(h) and len(h[0][0]) > 3 for _, h in rep[1])


def test_an_untouched_float_stream_does_not_see_the_formats():
    """stream 2 of a batch with a coded stream against stream 2 of a batch where no format was ever set (the coded
    stream's place taken by its float twin): bit-identical replies, chunk by chunk"""
    from speechcatcher_amd import synth
    fmt, ch, sel, scale = R.S16LE, 2, R.MIX, R.SCALE_FULL
    n = 10240
    data = [np.clip(synth.synth_audio(70 + k, n * 2) * 20000, -32768, 32767).astype("<i2").tobytes() for k in range(5)]
    floats = [R.decode(d, fmt, ch, sel, scale) for d in data]
    other = synth.synth_audio(34, n * 5)
    runs = []
    for coded in (True, False):
        sb = _tiny_batch(3)
        if coded:
            sb.set_input_format(1, fmt, ch, sel, scale)
        states = []
        for k in range(5):
            sb.push([(0, floats[k], k == 4), (1, data[k] if coded else floats[k], k == 4), (2, other[k * n:(k + 1) * n], k == 4)])
            states.append([_state(sb, s) for s in range(3)])
        runs.append(states)
    assert runs[0] == runs[1]
    assert len(runs[0][-1][2][0]) > 0


def test_xl_dims_coded_streams_equal_their_float_twins():
    """the XL-dims engine once, 8 streams x 4 chunks: streams 4..7 take the s16 bytes of the audio streams 0..3 take as
    floats (the CLI's conversion, / 32768)"""
    from speechcatcher_amd import synth
    n = 10240
    sb = _tiny_batch(8, cfg="XL")
    pcm16 = [np.clip(synth.synth_audio(80 + i, n * 4) * 20000, -32768, 32767).astype("<i2") for i in range(4)]
    for i in range(4):
        sb.set_input_format(4 + i, R.S16LE, 1, 0, R.SCALE_FULL)
    for k in range(4):
        items = []
        for i in range(4):
            c = pcm16[i][k * n:(k + 1) * n]
            items += [(i, c.astype(np.float32) / 32768.0, k == 3), (4 + i, c, k == 3)]
        sb.push(items)
        for i in range(4):
            assert _state(sb, i) == _state(sb, 4 + i), (k, i)
    assert all(len(_state(sb, i)[0]) > 0 and len(_state(sb, i)[0][0][0]) > 2 for i in range(4))


def test_refusals():
    from speechcatcher_amd.engine import EngineError
    from speechcatcher_amd import synth
    sb = _tiny_batch(3, max_chunk_samples=8192)
    x = np.clip(synth.synth_audio(5, 4000) * 20000, -32768, 32767).astype("<i2")
    # values out of range; a scale the format does not take
    for args in ((6, 1, 0, 0), (-1, 1, 0, 0), (R.S16LE, 0, 0, 0), (R.S16LE, 9, 0, 0), (R.S16LE, 2, 2, 0), (R.S16LE, 2, -2, 0),
                 (R.S16LE, 1, 0, 2), (R.S24LE, 1, 0, R.SCALE_SERVER), (R.U8, 1, 0, R.SCALE_SERVER), (R.F32, 2, 0, R.SCALE_SERVER)):
        with pytest.raises(EngineError):
            sb.set_input_format(0, *args)
    assert sb.input_format(0) == (R.F32, 1, 0, R.SCALE_FULL)
    # a stream with buffered audio; a stream with an outstanding chunk
    sb.push([(0, x[:150].astype(np.float32) / 32768.0, False)])
    with pytest.raises(EngineError, match="buffered"):
        sb.set_input_format(0, R.S16LE, 1, 0, 0)
    sb.submit([(1, x[:150].astype(np.float32) / 32768.0, False)])
    with pytest.raises(EngineError, match="outstanding"):
        sb.set_input_format(1, R.S16LE, 1, 0, 0)
    while sb.outstanding:
        sb.poll(1)
    # sc_submit / sc_push on a coded stream name the _raw call; device-resident PCM is mono float only
    sb.reset(0)
    sb.set_input_format(0, R.S16LE, 1, 0, 0)
    ids, cnt, fin = (C_int32 * 1)(0), (C_int32 * 1)(100), (C_uint8 * 1)(0)
    buf = np.zeros(100, np.float32)
    ptr = (C_void_p * 1)(buf.ctypes.data)
    assert sb.lib.sc_submit(sb.handle, ids, ptr, cnt, fin, 1) == -1 and b"sc_submit_raw" in sb.lib.sc_last_error()
    assert sb.lib.sc_push(sb.handle, ids, ptr, cnt, fin, 1, None) == -1 and b"sc_push_raw" in sb.lib.sc_last_error()
    with pytest.raises(EngineError, match="mono float only"):
        sb.push([(0, 100, False)], pcm_resident=True)
    with pytest.raises(EngineError, match="whole number"):
        sb.push([(0, b"\0\0\0", False)])
    with pytest.raises(EngineError, match="coded bytes"):
        sb.push([(0, buf, False)])
    # a chunk longer than max_chunk_samples allows fails that stream alone
    lim = 8192 + 16 * sb.cfg.hop_length
    y = synth.synth_audio(6, 4000)
    out = sb.push([(0, np.zeros(lim + 1, "<i2"), False), (2, y, False)], isolate_faults=True)
    assert isinstance(out[0], EngineError) and "max_chunk_samples" in str(out[0]) and not isinstance(out[2], Exception)
    # bytes that overflow the byte region: 3 streams x lim frames x 4 bytes per slot; 8 channels of f32 are 32 bytes a frame
    sb.reset(1)
    sb.set_input_format(1, R.F32, 8, R.MIX, 0)
    sb.reset(2)
    before = sb.st[2].pcm_buffered
    assert before == 0
    big = np.zeros(lim * 8, np.float32)               # lim frames: 8 x the float span, more than the 3 x of the region
    out = sb.push([(0, x[:4000], False), (1, big, False), (2, y, False)], isolate_faults=True)
    assert isinstance(out[1], EngineError) and "byte region" in str(out[1]), out[1]
    assert not isinstance(out[0], Exception) and not isinstance(out[2], Exception)
    assert sb.st[0].pcm_buffered > 0 and sb.st[2].pcm_buffered > 0 and sb.st[1].pcm_buffered == 0
    assert sb.input_level(0) == R.level(x[:4000].tobytes(), R.S16LE, 1, 0)
    # ... and a chunk of that format that fits is served
    small = (0.1 * np.random.default_rng(3).standard_normal(8 * 2000)).astype(np.float32)
    out = sb.push([(1, small, False)])
    assert sb.waveform_buffer(1)[-5:].tobytes() == R.decode(small.tobytes(), R.F32, 8, R.MIX)[-5:].tobytes()


C_HOST_RAW = r"""
/* A plain C host of libscasr that feeds s16le bytes: two streams get the same audio, stream 0 as floats through sc_submit,
 * stream 1 as the bytes through sc_submit_raw; one line per reply: stream, status, token ids of the best hypothesis, and for
 * stream 1 the input level. */
#include <stdio.h>
#include <stdlib.h>
#include "scasr.h"
int main(int argc, char **argv) {
  if (argc < 4) return 2;
  const int chunk = atoi(argv[3]);
  sc_engine *eng = NULL; sc_streams *st = NULL;
  if (sc_version() != SC_ABI_VERSION) { fprintf(stderr, "libscasr ABI %d, header %d\n", sc_version(), SC_ABI_VERSION); return 3; }
  if (sc_engine_load(argv[1], 0, &eng) != SC_OK) { fprintf(stderr, "%s\n", sc_last_error()); return 1; }
  sc_stream_options o = {2, 5, 0.3f, 1, 256, 200, 1 << 18, 32768, 0};
  if (sc_streams_create(eng, &o, &st) != SC_OK) { fprintf(stderr, "%s\n", sc_last_error()); return 1; }
  if (sc_stream_set_input_format(st, 1, SC_PCM_S16LE, 1, 0, SC_PCM_SCALE_FULL) != SC_OK) { fprintf(stderr, "%s\n", sc_last_error()); return 1; }
  int fmt = -1, ch = -1, sel = -1, scale = -1;
  if (sc_stream_input_format(st, 1, &fmt, &ch, &sel, &scale) != SC_OK || fmt != SC_PCM_S16LE || ch != 1) return 4;
  FILE *f = fopen(argv[2], "rb"); if (!f) return 1;
  fseek(f, 0, SEEK_END); long n = ftell(f) / 2; fseek(f, 0, SEEK_SET);
  int16_t *pcm = (int16_t *)malloc(n * 2);
  float *flt = (float *)malloc(n * 4);
  if (fread(pcm, 2, n, f) != (size_t)n) return 1;
  fclose(f);
  for (long i = 0; i < n; ++i) flt[i] = (float)pcm[i] / 32768.0f;
  static int32_t ids[5 * 200]; int lens[5]; double sc[5];
  for (long pos = 0; pos < n; pos += chunk) {
    int cnt = (int)(pos + chunk < n ? chunk : n - pos);
    uint8_t fin = pos + chunk >= n;
    int s0 = 0, s1 = 1;
    const float *pf = flt + pos; const void *pr = pcm + pos;
    if (sc_submit(st, &s0, &pf, &cnt, &fin, 1) != SC_OK) { fprintf(stderr, "%s\n", sc_last_error()); return 1; }
    if (sc_submit_raw(st, &s1, &pr, &cnt, &fin, 1) != SC_OK) { fprintf(stderr, "%s\n", sc_last_error()); return 1; }
    int got = 0;
    while (got < 2) {
      int done[2], status[2];
      const int nd = sc_poll(st, 1, 2, done, status);
      if (nd < 0) { fprintf(stderr, "%s\n", sc_last_error()); return 1; }
      for (int i = 0; i < nd; ++i, ++got) {
        if (status[i] < 0) { fprintf(stderr, "%s\n", sc_stream_last_error(st, done[i])); return 1; }
        int nh = sc_get_hyps(st, done[i], 1, 200, ids, NULL, lens, sc, NULL, NULL);
        printf("%d %d |", done[i], status[i]);
        for (int k = 0; nh > 0 && k < lens[0]; ++k) printf(" %d", ids[k]);
        sc_input_level_t lv;
        if (sc_stream_input_level(st, done[i], &lv) != SC_OK) return 5;
        printf(" | %lld %lld %lld %d %d\n", (long long)lv.frames, (long long)lv.clipped, (long long)lv.sum_abs, lv.peak, lv.full_scale);
      }
    }
  }
  sc_streams_destroy(st); sc_engine_destroy(eng); free(pcm); free(flt);
  return 0;
}
"""


def test_c_host_program_feeds_raw_bytes(tmp_path):
    """sc_stream_set_input_format + sc_submit_raw + sc_stream_input_level from a gcc-compiled C program: the coded stream's
    replies equal its float twin's, its level is the contract's"""
    import shutil
    import subprocess
    from conftest import ROOT
    from speechcatcher_amd import synth
    from speechcatcher_amd.config import TINY
    from speechcatcher_amd.weights import PackedWeights
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    sd = synth.make_state_dict(TINY, 1234)
    mean, std = synth.stats_to_mean_std(synth.make_stats(TINY, kind="meanstd"))
    PackedWeights(sd, TINY, "cpu", mean, std).save_packed(tmp_path / "tiny.scpk")
    chunk, n = 10240, 5
    x = np.clip(np.round(synth.synth_audio(5, chunk * n) * 32767.0), -32768, 32767).astype("<i2")
    x.tofile(tmp_path / "audio.s16")
    (tmp_path / "host.c").write_text(C_HOST_RAW)
    libdir = ROOT / "speechcatcher_amd"
    subprocess.run([gcc, "-std=c99", "-O1", "-Wall", "-I", str(ROOT / "include"), str(tmp_path / "host.c"), "-L", str(libdir),
                    "-lscasr", f"-Wl,-rpath,{libdir}", "-o", str(tmp_path / "host")], check=True)
    res = subprocess.run([str(tmp_path / "host"), str(tmp_path / "tiny.scpk"), str(tmp_path / "audio.s16"), str(chunk)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    per = {0: [], 1: []}
    for line in res.stdout.strip().splitlines():
        head, ids, lv = line.split("|")
        per[int(head.split()[0])].append((int(head.split()[1]), ids.split(), [int(v) for v in lv.split()]))
    assert len(per[0]) == len(per[1]) == n
    assert [(a, b) for a, b, _ in per[0]] == [(a, b) for a, b, _ in per[1]]
    assert any(len(ids) > 3 for _, ids, _ in per[1])
    want = None
    for k in range(n):
        want = R.level(x[k * chunk:(k + 1) * chunk].tobytes(), R.S16LE, 1, 0, prev=want)
        assert per[1][k][2] == [want[f] for f in ("frames", "clipped", "sum_abs", "peak", "full_scale")], k
        assert per[0][k][2] == [0, 0, 0, 0, 0]


def test_cli_reads_a_stereo_mulaw_wav(tmp_path):
    """a stereo mu-law 8 kHz WAV and a mono s16 16 kHz WAV that holds the former's decoded, downmixed and converted samples
    go through recognize_file (--channel mix): the same text; --channel N picks one side"""
    from speechcatcher_amd import pcm, synth
    from speechcatcher_amd.__main__ import read_wav_16k_mono, recognize_file, to_16k
    from speechcatcher_amd.config import TINY
    from speechcatcher_amd.speech2text_streaming import load_model
    mdir = synth.write_model_dir(tmp_path / "tiny", TINY, seed=1234, stats_kind="meanstd")
    n = 8000 * 4
    sides = [synth.synth_audio(41 + c, 2 * n)[::2] * 0.8 for c in range(2)]
    codes = np.stack([_encode(s.astype(np.float64), R.MULAW)[:, 0] for s in sides], axis=1)
    stereo = tmp_path / "call.wav"
    pcm.write_wav(stereo, codes.tobytes(), pcm.MULAW, 2, 8000)
    with pytest.raises(SystemExit, match="16 kHz mono"):       # a multichannel recording needs --channel
        read_wav_16k_mono(str(stereo))
    raw, rate = read_wav_16k_mono(str(stereo), channel="mix")
    assert rate == 8000 and raw.cpu().numpy().tobytes() == R.decode(codes.tobytes(), R.MULAW, 2, R.MIX).tobytes()
    x16 = to_16k(raw, rate)
    assert x16.dtype == np.int16 and len(x16) == 2 * n and np.abs(x16).max() > 1000
    mono = tmp_path / "mono.wav"
    pcm.write_wav(mono, x16.astype("<i2").tobytes(), pcm.S16LE, 1, 16000)
    m_raw, m_rate = read_wav_16k_mono(str(mono))
    assert m_rate == 16000 and isinstance(m_raw, np.ndarray) and m_raw.tobytes() == x16.tobytes()   # today's path
    s2t = load_model(str(mdir), device="cuda", beam_size=3, use_bbd=True)
    a = recognize_file(s2t, str(stereo), quiet=True, progress=False, channel="mix")
    b = recognize_file(s2t, str(mono), quiet=True, progress=False)
    assert a["complete_text"] == b["complete_text"] and a["paragraphs"] == b["paragraphs"]
    left, _ = read_wav_16k_mono(str(stereo), channel=0)
    assert left.cpu().numpy().tobytes() == R.decode(codes.tobytes(), R.MULAW, 2, 0).tobytes()
    with pytest.raises(SystemExit, match="channel"):
        read_wav_16k_mono(str(stereo), channel=2)

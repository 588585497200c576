"""Wire-format audio in, on the CPU: the contract of tests/pcm_ref.py against audioop and the host
conversions it replaces, the product-side restatement (speechcatcher_amd/pcm.py) against the contract, the RIFF/WAVE
reader, the argument errors of the new ABI calls, and the scheduler / server surfaces on the Python engine."""
import ctypes as C
import struct

import numpy as np
import pytest

import pcm_ref as R
from speechcatcher_amd import pcm, synth


def test_g711_equals_audioop_on_every_code():
    audioop = pytest.importorskip("audioop")
    codes = bytes(range(256))
    u = np.frombuffer(audioop.ulaw2lin(codes, 2), "<i2")
    a = np.frombuffer(audioop.alaw2lin(codes, 2), "<i2")
    assert [R.ulaw_value(b) for b in range(256)] == u.tolist()
    assert [R.alaw_value(b) for b in range(256)] == a.tolist()
    assert pcm.ULAW_TABLE.tolist() == u.tolist() and pcm.ALAW_TABLE.tolist() == a.tolist()


def test_g711_spot_values():
    assert [R.ulaw_value(b) for b in (0x00, 0x80, 0xFF, 0x7F)] == [-32124, 32124, 0, 0]
    assert [R.alaw_value(b) for b in (0xD5, 0x55, 0xAA, 0x2A)] == [8, -8, 32256, -32256]
    assert max(abs(R.ulaw_value(b)) for b in range(256)) == 32124
    assert max(abs(R.alaw_value(b)) for b in range(256)) == 32256


def test_s16_scales_are_the_host_conversions_bit_for_bit():
    from speechcatcher_amd.server_session import scale_server_pcm
    v = np.arange(-32768, 32768, dtype=np.int16)
    raw = v.astype("<i2").tobytes()
    full = R.decode(raw, R.S16LE, 1, 0, R.SCALE_FULL)
    server = R.decode(raw, R.S16LE, 1, 0, R.SCALE_SERVER)
    assert (full.view(np.uint32) == (v.astype(np.float32) / 32768.0).view(np.uint32)).all()
    assert (server.view(np.uint32) == scale_server_pcm(v).view(np.uint32)).all()
    assert float(np.float16(32767.0)) == 32768.0


def _same(got, want):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_the_product_decode_and_level_equal_the_contract(fmt):
    rng = np.random.default_rng(100 + fmt)
    for ch in (1, 2, 3, 8):
        bpf = R.bytes_per_frame(fmt, ch)
        assert pcm.bytes_per_frame(fmt, ch) == bpf
        data = bytearray(rng.bytes(300 * bpf))
        if fmt == R.S16LE:
            data[0:4] = b"\xff\x7f\x00\x80"
        if fmt == R.S24LE:
            data[0:6] = b"\xff\xff\x7f\x00\x00\x80"
        data = bytes(data)
        for sel in list(range(ch)) + [R.MIX]:
            for scale in ((R.SCALE_FULL, R.SCALE_SERVER) if R.BITS.get(fmt) == 15 else (R.SCALE_FULL,)):
                _same(pcm.decode(data, fmt, ch, sel, scale), R.decode(data, fmt, ch, sel, scale))
                half = 100 * bpf
                first = R.level(data[:half], fmt, ch, sel, scale)
                assert pcm.level(data[:half], fmt, ch, sel, scale) == first
                assert pcm.level(data[half:], fmt, ch, sel, scale, prev=first) == R.level(data, fmt, ch, sel, scale)
                assert R.level(data[half:], fmt, ch, sel, scale, prev=first) == R.level(data, fmt, ch, sel, scale)
                if fmt != R.F32:
                    assert pcm.add_levels(first, R.level(data[half:], fmt, ch, sel, scale)) == R.level(data, fmt, ch, sel, scale)
    # memoryview, bytearray and integer arrays are taken like bytes
    raw = rng.bytes(64 * R.bytes_per_frame(fmt, 2))
    want = R.decode(raw, fmt, 2, 0)
    for buf in (memoryview(raw), bytearray(raw), np.frombuffer(raw, np.uint8), np.frombuffer(raw, "<i2")):
        _same(pcm.decode(buf, fmt, 2, 0), want)
    assert pcm.level(b"", fmt, 2, R.MIX) == R.level(b"", fmt, 2, R.MIX)
    assert pcm.decode(b"", fmt, 2, R.MIX).shape == (0,)


def test_f32_nan_handling():
    bits = np.array([0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x3F800000, 0x7FC00000], np.uint32)
    raw = bits.tobytes()
    assert (R.decode(raw, R.F32, 1, 0).view(np.uint32) == bits).all()            # a selected channel: the bits
    assert (pcm.decode(raw, R.F32, 2, 1).view(np.uint32) == bits[1::2]).all()
    mix = R.decode(raw, R.F32, 2, R.MIX).view(np.uint32)
    assert mix[0] == R.CANONICAL_NAN                                              # NaN + inf
    assert mix[1] == 0xFF800000                                                   # -inf + a denormal
    assert mix[2] == R.CANONICAL_NAN
    _same(pcm.decode(raw, R.F32, 2, R.MIX), R.decode(raw, R.F32, 2, R.MIX))
    assert R.decode((np.float32(np.inf)).tobytes() + np.float32(-np.inf).tobytes(), R.F32, 2, R.MIX).view(np.uint32)[0] == R.CANONICAL_NAN
    assert R.level(raw, R.F32, 2, R.MIX) == R.ZERO_LEVEL


def test_the_s24_mix_is_divided_before_it_is_rounded():
    """|m| passes 2^24 in a three-channel s24 mix: fp32(m) / fp32(C) differs from RN_fp32(m / C)"""
    hi = (1 << 23) - 1
    vals = [hi, hi, 7]
    m = sum(vals)
    assert m > 1 << 24
    early = np.float32(m) / np.float32(3)
    once = np.float32(np.float64(m) / 3.0)
    assert early != once                                   # the reference distinguishes the two
    raw = b"".join(v.to_bytes(3, "little", signed=True) for v in vals)
    got = R.decode(raw, R.S24LE, 3, R.MIX)
    assert got[0] == once * np.float32(2.0 ** -23) and got[0] != early * np.float32(2.0 ** -23)
    _same(pcm.decode(raw, R.S24LE, 3, R.MIX), got)
    lv = R.level(raw, R.S24LE, 3, R.MIX)
    assert lv == dict(frames=1, clipped=1, sum_abs=m, peak=m, full_scale=3 << 23) and m == 16777221


def test_the_level_counts_clipped_frames_by_contributing_channel():
    x = np.array([[32767, 0], [0, -32768], [5, 5], [-32768, 32767]], "<i2").tobytes()
    assert R.level(x, R.S16LE, 2, 0)["clipped"] == 2 and R.level(x, R.S16LE, 2, 1)["clipped"] == 2
    assert R.level(x, R.S16LE, 2, R.MIX) == dict(frames=4, clipped=3, sum_abs=32767 + 32768 + 10 + 1, peak=32768,
                                                  full_scale=2 << 15)
    assert R.level(bytes([0x00, 0x80, 0xFF]), R.MULAW)["clipped"] == 2 and R.level(bytes([0xAA, 0x2A, 0xD5]), R.ALAW)["clipped"] == 2
    assert R.level(bytes([0, 255, 128]), R.U8) == dict(frames=3, clipped=2, sum_abs=255, peak=128, full_scale=128)


def test_argument_errors():
    for args in ((6, 1, 0, 0), (-1, 1, 0, 0), (R.S16LE, 0, 0, 0), (R.S16LE, 9, 0, 0), (R.S16LE, 2, 2, 0), (R.S16LE, 2, -2, 0),
                 (R.S16LE, 1, 0, 2), (R.S24LE, 1, 0, R.SCALE_SERVER), (R.U8, 1, 0, R.SCALE_SERVER), (R.F32, 1, 0, R.SCALE_SERVER)):
        with pytest.raises(ValueError):
            R.decode(b"", *args)
        with pytest.raises(ValueError):
            pcm.decode(b"", *args)
        with pytest.raises(ValueError):
            pcm.level(b"", *args)
    with pytest.raises(ValueError, match="whole number"):
        pcm.decode(b"\0\0\0", R.S16LE)
    with pytest.raises(ValueError, match="whole number"):
        R.decode(b"\0\0\0", R.S16LE)


# ---- RIFF/WAVE ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,ch,rate", [(R.S16LE, 1, 16000), (R.S16LE, 2, 44100), (R.U8, 1, 8000), (R.S24LE, 3, 48000),
                                         (R.F32, 2, 16000), (R.MULAW, 2, 8000), (R.ALAW, 1, 8000), (R.S24LE, 8, 16000)])
def test_riff_reader_reads_every_tag(tmp_path, fmt, ch, rate):
    rng = np.random.default_rng(fmt * 10 + ch)
    data = rng.bytes(101 * R.bytes_per_frame(fmt, ch))
    for ext in (False, True):
        path = tmp_path / f"a{int(ext)}.wav"
        pcm.write_wav(path, data, fmt, ch, rate, extensible=ext)
        w = pcm.read_wav(path)
        assert (w.format, w.channels, w.sample_rate, w.data) == (fmt, ch, rate, data)
    if fmt in (R.S16LE, R.U8):          # what the stdlib writes is read the same
        import wave
        path = tmp_path / "std.wav"
        with wave.open(str(path), "wb") as f:
            f.setnchannels(ch); f.setsampwidth(R.CODE_BYTES[fmt]); f.setframerate(rate)
            f.writeframes(data)
        w = pcm.read_wav(path)
        assert (w.format, w.channels, w.sample_rate, w.data) == (fmt, ch, rate, data)


def test_riff_reader_skips_unknown_chunks_and_honours_padding(tmp_path):
    data = bytes(range(1, 8)) * 3                # 21 mu-law frames: an odd-sized data chunk
    path = tmp_path / "odd.wav"
    pcm.write_wav(path, data, R.MULAW, 1, 8000, extra_chunks=[(b"LIST", b"abc"), (b"fact", struct.pack("<I", 21)), (b"junk", b"")])
    blob = path.read_bytes()
    assert blob.index(b"LIST") + 8 + 3 + 1 == blob.index(b"fact")          # the pad byte behind the odd chunk
    w = pcm.read_wav(path)
    assert (w.format, w.channels, w.sample_rate, w.data) == (R.MULAW, 1, 8000, data)
    # a chunk behind data is not looked at; a trailing partial frame is dropped; a data chunk cut short is read as far as it goes
    path2 = tmp_path / "tail.wav"
    pcm.write_wav(path2, b"\1\2\3\4\5", R.S16LE, 2, 16000)
    assert pcm.read_wav(path2).data == b"\1\2\3\4"
    assert pcm.parse_wav(blob[:-5]).data == data[:-4]
    for bad, msg in ((b"RIFX" + blob[4:], "RIFF"), (blob[:12], "no fmt"), (blob[:blob.index(b"data")], "no data")):
        with pytest.raises(ValueError, match=msg):
            pcm.parse_wav(bad)
    with pytest.raises(ValueError, match="unsupported"):           # 32-bit integer PCM
        pcm.parse_wav(b"RIFF" + struct.pack("<I", 36) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, 16000, 64000, 4, 32)
                      + b"data" + struct.pack("<I", 0))
    with pytest.raises(ValueError, match="channels"):
        pcm.parse_wav(b"RIFF" + struct.pack("<I", 36) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 9, 16000, 288000, 18, 16)
                      + b"data" + struct.pack("<I", 0))


# ---- the ABI without a GPU -------------------------------------------------------------------------------------------
def test_argument_errors_of_the_new_calls_do_not_need_a_gpu():
    from speechcatcher_amd import _abi
    lib = _abi.load()
    assert lib.sc_pcm_decode(None, 1, None) == -1 and b"null job table" in lib.sc_last_error()
    assert lib.sc_pcm_decode(None, -1, None) == -1 and b"negative" in lib.sc_last_error()
    assert lib.sc_pcm_decode(None, 0, None) == 0
    assert lib.sc_pcm_bytes_per_frame(6, 1) == -1 and lib.sc_pcm_bytes_per_frame(1, 9) == -1 and lib.sc_pcm_bytes_per_frame(1, 0) == -1
    for fmt in R.FORMATS:
        for ch in (1, 2, 3, 8):
            assert lib.sc_pcm_bytes_per_frame(fmt, ch) == R.bytes_per_frame(fmt, ch)
    lv = _abi.InputLevel()
    v = C.c_int32()
    assert lib.sc_stream_set_input_format(None, 0, 1, 1, 0, 0) == -1
    assert lib.sc_stream_input_format(None, 0, C.byref(v), C.byref(v), C.byref(v), C.byref(v)) == -1
    assert lib.sc_stream_input_level(None, 0, C.byref(lv)) == -1
    assert lib.sc_push_raw(None, None, None, None, None, 0, None) == -1 and b"null" in lib.sc_last_error()
    assert lib.sc_submit_raw(None, None, None, None, None, 0) == -1 and b"null" in lib.sc_last_error()
    assert C.sizeof(_abi.InputLevel) == 32 and C.sizeof(_abi.PcmJob) == 64
    assert (pcm.F32, pcm.S16LE, pcm.S24LE, pcm.U8, pcm.MULAW, pcm.ALAW, pcm.MIX, pcm.SCALE_FULL, pcm.SCALE_SERVER) == \
        (R.F32, R.S16LE, R.S24LE, R.U8, R.MULAW, R.ALAW, R.MIX, R.SCALE_FULL, R.SCALE_SERVER)
    import re
    from conftest import ROOT
    hdr = (ROOT / "include" / "scasr.h").read_text()
    for name, val in (("F32", 0), ("S16LE", 1), ("S24LE", 2), ("U8", 3), ("MULAW", 4), ("ALAW", 5), ("SCALE_FULL", 0),
                      ("SCALE_SERVER", 1), ("MAX_CHANNELS", 8), ("N_FORMATS", 6), ("MAX_JOBS", 65535)):
        assert int(re.search(rf"#define SC_PCM_{name} (\d+)", hdr).group(1)) == val, name
    assert re.search(r"#define SC_PCM_MIX \(-1\)", hdr)


def test_struct_layouts_match_the_header(tmp_path):
    import shutil
    import subprocess
    from conftest import ROOT
    from speechcatcher_amd import _abi
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    structs = {"sc_input_level_t": _abi.InputLevel, "sc_pcm_job": _abi.PcmJob}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "scasr.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(out[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(out[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


# ---- the Python engine, the scheduler and the server -------------------------------------------------------------------
def _batch(n_streams=2, **kw):
    from test_engine_spec import make_batch
    args = dict(max_frames=400, max_tokens=300, pcm_capacity=1 << 18)
    args.update(kw)
    return make_batch("TINY", 1234, "meanstd", 3, True, n_streams=n_streams, **args)


def _pcm16(seed, n):
    return np.clip(np.round(synth.synth_audio(seed, n) * 32767.0), -32768, 32767).astype(np.int16)


def _hyps(sb, s):
    return [(h["yseq"], h["xpos"], h["score"]) for h in sb.hypotheses(s)]


def test_python_engine_decodes_on_the_host():
    from speechcatcher_amd.engine import EngineError
    sb = _batch(2)
    x = _pcm16(5, 10240 * 3)
    stereo = np.stack([x, _pcm16(6, 10240 * 3)], axis=1)         # [n, 2] interleaved
    sb.set_input_format(1, pcm.S16LE, 2, 0, pcm.SCALE_FULL)
    assert sb.input_format(1) == (pcm.S16LE, 2, 0, pcm.SCALE_FULL) and sb.input_format(0) == (pcm.F32, 1, 0, pcm.SCALE_FULL)
    lv = None
    for k in range(3):
        sl = slice(k * 10240, (k + 1) * 10240)
        chunk = stereo[sl].tobytes()
        out = sb.push([(0, x[sl].astype(np.float32) / 32768.0, k == 2), (1, chunk, k == 2)])
        assert out[0] == out[1] and _hyps(sb, 0) == _hyps(sb, 1)
        lv = R.level(chunk, R.S16LE, 2, 0, prev=lv)
        assert sb.input_level(1) == lv and sb.input_level(0) == R.ZERO_LEVEL
    assert len(_hyps(sb, 1)) > 0
    sb.reset(1)
    assert sb.input_level(1) == R.ZERO_LEVEL and sb.input_format(1)[0] == pcm.S16LE
    sb.push([(1, stereo[:4000].tobytes(), False)])
    assert sb.input_level(1) == R.level(stereo[:4000].tobytes(), R.S16LE, 2, 0)
    # a final chunk ends the utterance: the next chunk starts the level over, also without a reset in between
    sb.reset(1)
    a, b, c = (stereo[k * 10240:(k + 1) * 10240].tobytes() for k in range(3))
    sb.push([(1, a, True)])
    assert sb.input_level(1) == R.level(a, R.S16LE, 2, 0)
    sb.push([(1, b, False)])
    assert sb.input_level(1) == R.level(b, R.S16LE, 2, 0)
    sb.push([(1, c, False)])
    assert sb.input_level(1) == R.level(c, R.S16LE, 2, 0, prev=R.level(b, R.S16LE, 2, 0))
    # a chunk that is not whole frames fails that stream alone when faults are isolated
    sb.reset(0)
    sb.reset(1)
    out = sb.push([(0, x[:4000].astype(np.float32) / 32768.0, False), (1, b"\0\0\0", False)], isolate_faults=True)
    assert isinstance(out[1], EngineError) and "whole number" in str(out[1]) and not isinstance(out[0], Exception)
    assert sb.st[0].pcm_end == 4000 and sb.st[1].pcm_end == 0
    with pytest.raises(EngineError, match="whole number"):
        sb.push([(1, b"\0\0\0", False)])
    sb.push([(1, b, False)])
    with pytest.raises(EngineError, match="buffered"):
        sb.set_input_format(1, pcm.MULAW)
    with pytest.raises(EngineError, match="coded bytes"):
        sb.push([(1, np.zeros(100, np.float32), False)])
    with pytest.raises(EngineError):
        sb.set_input_format(0, pcm.S24LE, 1, 0, pcm.SCALE_SERVER)


def test_scheduler_opens_sessions_with_a_format():
    from speechcatcher_amd.scheduler import LevelResults, StreamScheduler
    sb = _batch(2)
    sch = StreamScheduler(sb, None, result_format="espnet", input_level=True)
    x = _pcm16(7, 10240 * 2)
    codes = np.abs(pcm.ULAW_TABLE[None, :].astype(np.int64) - x[:, None]).argmin(axis=1).astype(np.uint8)
    a = sch.open()
    b = sch.open(format=pcm.MULAW, channels=1, channel=0, scale=pcm.SCALE_SERVER)
    assert sch.input_format(b) == (pcm.MULAW, 1, 0, pcm.SCALE_SERVER) and sch.input_format(a)[0] == pcm.F32
    with pytest.raises(ValueError):
        sch.open(format=9)
    lv = None
    for k in range(2):
        sl = slice(k * 10240, (k + 1) * 10240)
        sch.feed(a, pcm.decode(codes[sl], pcm.MULAW, 1, 0, pcm.SCALE_SERVER), is_final=k == 1)
        sch.feed(b, codes[sl].tobytes(), is_final=k == 1)
        res = sch.step()
        assert isinstance(res[b], LevelResults) and list(res[a]) == list(res[b])
        lv = R.level(codes[sl].tobytes(), R.MULAW, 1, 0, R.SCALE_SERVER, prev=lv)
        assert res[b].level == lv and res[a].level == R.ZERO_LEVEL
    sch.close(a)
    sch.close(b)
    d = sch.open(format=pcm.S16LE)
    with pytest.raises(ValueError, match="whole number"):
        sch.feed(d, b"\0\0\0")
    sch.close(d)
    c = sch.open()                       # the slot goes back to float samples
    assert sch.input_format(c)[0] == pcm.F32 and sb.input_format(sch._slot_of[c])[:2] == (pcm.F32, 1)
    sch.feed(c, x[:4000].astype(np.float32) / 32768.0)
    assert not isinstance(sch.step()[c], Exception)
    with pytest.raises(ValueError, match="before its first audio"):
        sch.set_input_format(c, pcm.S16LE)


def _serve(loop, plans):
    sids = {c: loop.connect() for c in plans}
    for c, msgs in plans.items():
        for m in msgs:
            loop.submit(sids[c], m)
    got = {c: [] for c in plans}
    inv = {v: k for k, v in sids.items()}
    while loop.pending():
        for sid, replies in loop.step().items():
            got[inv[sid]] += replies
    return got


def _loop(**kw):
    from speechcatcher_amd.scheduler import StreamScheduler
    from speechcatcher_amd.server_session import ServerLoop
    return ServerLoop(StreamScheduler(_batch(2), None, result_format="espnet"), vosk_output_format=True,
                      finalize_update_iters=2, max_partial_iters=5, **kw)


def test_server_raw_input_replies_equal_the_defaults():
    chunks = [_pcm16(5, 10240) for _ in range(5)]
    plans = {0: [c.tobytes() for c in chunks] + ['{"eof" : 1}'], 1: list(chunks[:3])}
    base = _serve(_loop(), plans)
    raw = _serve(_loop(raw_input=True), plans)
    assert raw == base
    assert any("result" in r or r.get("partial") for r in base[0])
    lvl = _serve(_loop(raw_input=True, input_level=True), plans)
    strip = lambda rs: [{k: v for k, v in r.items() if k != "level"} for r in rs]   # noqa: E731
    assert strip(lvl[0]) == base[0] and strip(lvl[1]) == base[1]
    assert all("level" in r for r in lvl[0] + lvl[1])
    # the level of client 1 after each of its chunks: cumulative (none of them was finalised by the endpointer: two replies in)
    want, lv = [], None
    for c in chunks[:2]:
        lv = R.level(c.tobytes(), R.S16LE, 1, 0, R.SCALE_SERVER, prev=lv)
        want.append(lv)
    assert [r["level"] for r in lvl[1][:2]] == want
    off = _serve(_loop(input_level=True), plans)                    # converted on the host: the record stays zero
    assert all(r["level"] == R.ZERO_LEVEL for r in off[0])


def test_server_honours_a_format_config_before_the_first_audio():
    x = _pcm16(8, 5120 * 4)                                      # 8 kHz
    other = _pcm16(9, 5120 * 4)
    to_ulaw = lambda v: np.abs(pcm.ULAW_TABLE[None, :].astype(np.int64) - v[:, None]).argmin(axis=1).astype(np.uint8)   # noqa: E731
    stereo = np.stack([to_ulaw(other), to_ulaw(x)], axis=1)      # the speaker on channel 1
    cfg = '{"config": {"sample_rate": 16000, "format": "mulaw", "channels": 2, "channel": 1}}'
    msgs = [stereo[k * 5120:(k + 1) * 5120].tobytes() for k in range(4)]
    got = _serve(_loop(input_level=True), {0: [cfg] + msgs})
    # ... equals a session that sends channel 1's decoded samples through today's path (s16 whose server conversion is the same
    # float16 rounding of the same integers)
    mono = pcm.ULAW_TABLE[to_ulaw(x)].astype(np.int16)
    base = _serve(_loop(), {0: ['{"config": {"sample_rate": 16000}}'] + [mono[k * 5120:(k + 1) * 5120] for k in range(4)]})
    assert [{k: v for k, v in r.items() if k != "level"} for r in got[0]] == base[0]
    assert got[0][1]["level"] == R.level(msgs[0], R.MULAW, 2, 1, R.SCALE_SERVER)
    # unknown values and a change after audio are this client's ValueError
    for bad in ('{"config": {"format": "opus"}}', '{"config": {"channels": 9}}', '{"config": {"format": "s24le", "channels": 2, "channel": 2}}',
                '{"config": {"channels": "two"}}'):
        out = _serve(_loop(), {0: [bad]})
        assert len(out[0]) == 1 and isinstance(out[0][0], ValueError), (bad, out)
    out = _serve(_loop(), {0: [msgs[0][:10240], cfg]})
    assert isinstance(out[0][-1], ValueError) and "first audio" in str(out[0][-1])
    # "mix" and a config that names nothing leave the session as it was
    loop = _loop()
    sid = loop.connect()
    loop.submit(sid, '{"config": {"format": "alaw", "channels": 2, "channel": "mix"}}')
    loop.step()
    assert loop.sch.input_format(sid) == (pcm.ALAW, 2, pcm.MIX, pcm.SCALE_SERVER)
    loop.submit(sid, '{"config": {"words": true}}')
    loop.step()
    assert loop.sch.input_format(sid) == (pcm.ALAW, 2, pcm.MIX, pcm.SCALE_SERVER)

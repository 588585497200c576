"""Wire-format audio in (include/scasr.h: sc_pcm_decode): the format constants, the host-side decode of
the contract (vectorised numpy; tests/pcm_ref.py is the contract, pcm.hip the device code) and a small RIFF/WAVE reader.

A stream's input is (format, channels, channel, scale); a chunk is n sample frames of ``channels`` interleaved
little-endian codes.  ``decode`` gives the float32 samples the engine sees, ``level`` the cumulative input level."""
import struct
from typing import NamedTuple

import numpy as np

F32, S16LE, S24LE, U8, MULAW, ALAW = range(6)
N_FORMATS = 6
MIX = -1
MAX_CHANNELS = 8
SCALE_FULL, SCALE_SERVER = 0, 1
FORMAT_NAMES = {"f32": F32, "s16le": S16LE, "s24le": S24LE, "u8": U8, "mulaw": MULAW, "alaw": ALAW}
NAME_OF = {v: k for k, v in FORMAT_NAMES.items()}
_CODE_BYTES = (4, 2, 3, 1, 1, 1)
_BITS = (None, 15, 23, 7, 15, 15)
_EXTREME = (None, (-32768, 32767), (-(1 << 23), (1 << 23) - 1), (-128, 127), (-32124, 32124), (-32256, 32256))
LEVEL_FIELDS = ("frames", "clipped", "sum_abs", "peak", "full_scale")


def _g711_tables():
    b = np.arange(256, dtype=np.int64)
    u = ~b & 0xFF
    mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84
    ulaw = np.where(u & 0x80, -mag, mag)
    a = (b ^ 0x55) & 0xFF
    e = (a >> 4) & 7
    mag = np.where(e == 0, ((a & 15) << 4) + 8, (((a & 15) << 4) + 0x108) << np.maximum(e - 1, 0))
    alaw = np.where(a & 0x80, mag, -mag)
    return ulaw.astype(np.int32), alaw.astype(np.int32)


ULAW_TABLE, ALAW_TABLE = _g711_tables()


def check_args(fmt, channels, channel, scale):
    if not (isinstance(fmt, (int, np.integer)) and 0 <= fmt < N_FORMATS):
        raise ValueError(f"input format {fmt!r} out of range")
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"channels {channels} outside 1..{MAX_CHANNELS}")
    if not MIX <= channel < channels:
        raise ValueError(f"channel {channel} outside [-1, {channels})")
    if scale not in (SCALE_FULL, SCALE_SERVER) or (scale == SCALE_SERVER and _BITS[fmt] != 15):
        raise ValueError(f"scale {scale} is not taken by format {NAME_OF[int(fmt)]}")


def bytes_per_frame(fmt, channels=1):
    check_args(fmt, channels, 0, SCALE_FULL)
    return _CODE_BYTES[fmt] * channels


def as_bytes(buf):
    """bytes / bytearray / memoryview / a numpy array of any integer or float dtype -> a 1-D uint8 view of its bytes"""
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    return np.frombuffer(buf, np.uint8)


def silence(fmt, channels=1, n=1):
    """n frames of digital silence in a format (uint8 array): zeros, 0x80 for u8, 0xff for mu-law (0), 0xd5 for A-law (+8)"""
    check_args(fmt, channels, 0, SCALE_FULL)
    fill = {U8: 0x80, MULAW: 0xFF, ALAW: 0xD5}.get(fmt, 0)
    return np.full(n * _CODE_BYTES[fmt] * channels, fill, np.uint8)


def _values(buf, fmt, channels):
    """-> int32 [n, channels] of an integer format"""
    raw = as_bytes(buf)
    bpf = _CODE_BYTES[fmt] * channels
    if raw.size % bpf:
        raise ValueError(f"{raw.size} bytes are not a whole number of {bpf}-byte frames")
    n = raw.size // bpf
    if fmt == S16LE:
        v = raw.view("<i2").astype(np.int32) if raw.ctypes.data % 2 == 0 else np.frombuffer(raw.tobytes(), "<i2").astype(np.int32)
    elif fmt == S24LE:
        t = raw.reshape(-1, 3).astype(np.int32)
        v = ((t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)) << 8) >> 8
    elif fmt == U8:
        v = raw.astype(np.int32) - 128
    elif fmt == MULAW:
        v = ULAW_TABLE[raw]
    else:
        v = ALAW_TABLE[raw]
    return v.reshape(n, channels)


def _m(buf, fmt, channels, channel):
    v = _values(buf, fmt, channels)
    used = v if channel == MIX else v[:, channel:channel + 1]
    lo, hi = _EXTREME[fmt]
    return used.sum(axis=1, dtype=np.int32), ((used == lo) | (used == hi)).any(axis=1)


def decode(buf, fmt, channels=1, channel=MIX, scale=SCALE_FULL):
    """coded bytes -> float32 [n], the samples sc_pcm_decode writes (bit for bit)"""
    check_args(fmt, channels, channel, scale)
    if fmt == F32:
        raw = as_bytes(buf)
        if raw.size % (4 * channels):
            raise ValueError(f"{raw.size} bytes are not a whole number of {4 * channels}-byte frames")
        x = np.frombuffer(raw.tobytes(), "<f4").reshape(-1, channels)
        if channel != MIX:
            return x[:, channel].copy()   # the bits, NaNs included
        with np.errstate(all="ignore"):
            s = x[:, 0].copy()
            for c in range(1, channels):
                s = s + x[:, c]           # float32 adds, ascending, each rounded
            r = (s.astype(np.float64) / np.float64(channels)).astype(np.float32)
        r.view(np.uint32)[np.isnan(r)] = 0x7FC00000
        return r
    m, _ = _m(buf, fmt, channels, channel)
    C = channels if channel == MIX else 1
    x = (m.astype(np.float64) / np.float64(C)).astype(np.float32)   # the exact quotient, rounded once
    if scale == SCALE_SERVER:
        return x.astype(np.float16).astype(np.float32) * np.float32(2.0 ** -15)
    return x * np.float32(2.0 ** -_BITS[fmt])


def zero_level():
    return dict.fromkeys(LEVEL_FIELDS, 0)


def level(buf, fmt, channels=1, channel=MIX, scale=SCALE_FULL, prev=None):
    """the cumulative level record after ``buf`` (prev None: the chunk starts an utterance)"""
    check_args(fmt, channels, channel, scale)
    lv = zero_level() if prev is None else dict(prev)
    if fmt == F32:
        lv["full_scale"] = 0
        return lv
    m, clip = _m(buf, fmt, channels, channel)
    a = np.abs(m.astype(np.int64))
    lv["frames"] += int(m.size)
    lv["peak"] = max(lv["peak"], int(a.max()) if a.size else 0)
    lv["sum_abs"] += int(a.sum())
    lv["clipped"] += int(clip.sum())
    lv["full_scale"] = (channels if channel == MIX else 1) << _BITS[fmt]
    return lv


def add_levels(a, b):
    """the level of two stretches of one utterance from the levels of each (all integer: exact in any order)"""
    out = {k: a[k] + b[k] for k in ("frames", "clipped", "sum_abs")}
    out["peak"] = max(a["peak"], b["peak"])
    out["full_scale"] = b["full_scale"] or a["full_scale"]
    return out


# ---- RIFF/WAVE -----------------------------------------------------------------------------------------------------
# (the stdlib wave module refuses every format tag but PCM)
WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT, WAVE_FORMAT_ALAW, WAVE_FORMAT_MULAW, WAVE_FORMAT_EXTENSIBLE = 1, 3, 6, 7, 0xFFFE
_KSDATAFORMAT_TAIL = bytes.fromhex("000000001000800000aa00389b71")   # GUID bytes 2..15 of the KSDATAFORMAT_SUBTYPE_* family


class WavInfo(NamedTuple):
    format: int        # F32 .. ALAW
    channels: int
    sample_rate: int
    data: bytes        # whole sample frames


def _wav_format(tag, bits, where):
    if tag == WAVE_FORMAT_PCM and bits in (8, 16, 24):
        return {8: U8, 16: S16LE, 24: S24LE}[bits]
    if tag == WAVE_FORMAT_IEEE_FLOAT and bits == 32:
        return F32
    if tag == WAVE_FORMAT_ALAW and bits == 8:
        return ALAW
    if tag == WAVE_FORMAT_MULAW and bits == 8:
        return MULAW
    raise ValueError(f"{where}: unsupported WAVE format (tag {tag:#x}, {bits} bits): 8 / 16 / 24-bit PCM, 32-bit float, "
                     "A-law and mu-law are read")


def parse_wav(blob, where="wav") -> WavInfo:
    """A RIFF/WAVE file's bytes -> WavInfo.  Format tags 1 (PCM 8 / 16 / 24 bit), 3 (float 32), 6 (A-law), 7 (mu-law) and
    0xFFFE (extensible, with those sub-formats), 1..8 channels; unknown chunks are skipped, a chunk of odd size is followed
    by its pad byte; a data chunk that runs past the end of the file (a stream cut short) is read as far as it goes."""
    blob = bytes(blob)
    if len(blob) < 12 or blob[:4] != b"RIFF" or blob[8:12] != b"WAVE":
        raise ValueError(f"{where}: not a RIFF/WAVE file")
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(blob):
        cid, size = blob[pos:pos + 4], struct.unpack_from("<I", blob, pos + 4)[0]
        body = blob[pos + 8: pos + 8 + size]
        if cid == b"fmt ":
            if len(body) < 16:
                raise ValueError(f"{where}: fmt chunk of {len(body)} bytes")
            tag, channels, rate, _, align, bits = struct.unpack_from("<HHIIHH", body)
            if tag == WAVE_FORMAT_EXTENSIBLE:
                if len(body) < 40 or body[26:40] != _KSDATAFORMAT_TAIL:
                    raise ValueError(f"{where}: extensible fmt chunk without a known sub-format")
                tag = struct.unpack_from("<H", body, 24)[0]
            if not 1 <= channels <= MAX_CHANNELS:
                raise ValueError(f"{where}: {channels} channels (1..{MAX_CHANNELS} are read)")
            f = _wav_format(tag, bits, where)
            if align != _CODE_BYTES[f] * channels:
                raise ValueError(f"{where}: block align {align} for {channels} channels of {bits} bits")
            fmt = (f, channels, rate)
        elif cid == b"data":
            if fmt is None:
                raise ValueError(f"{where}: data chunk before the fmt chunk")
            data = body
            break
        pos += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError(f"{where}: no {'fmt' if fmt is None else 'data'} chunk")
    bpf = _CODE_BYTES[fmt[0]] * fmt[1]
    return WavInfo(fmt[0], fmt[1], fmt[2], data[:len(data) // bpf * bpf])


def read_wav(path) -> WavInfo:
    with open(path, "rb") as f:
        return parse_wav(f.read(), str(path))


def write_wav(path, data, fmt, channels, sample_rate, extensible=False, extra_chunks=()):
    """coded bytes -> a RIFF/WAVE file (tools and tests; ``extra_chunks``: (id, body) pairs written before ``data``)"""
    tag, bits = {F32: (3, 32), S16LE: (1, 16), S24LE: (1, 24), U8: (1, 8), MULAW: (7, 8), ALAW: (6, 8)}[fmt]
    align = _CODE_BYTES[fmt] * channels
    head = struct.pack("<HHIIHH", WAVE_FORMAT_EXTENSIBLE if extensible else tag, channels, sample_rate, sample_rate * align,
                       align, bits)
    if extensible:
        head += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + _KSDATAFORMAT_TAIL
    elif tag != 1:
        head += struct.pack("<H", 0)
    chunks = [(b"fmt ", head)] + list(extra_chunks) + [(b"data", bytes(data))]
    body = b"".join(cid + struct.pack("<I", len(b)) + b + (b"\0" if len(b) & 1 else b"") for cid, b in chunks)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WAVE" + body)

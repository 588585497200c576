"""Wire-format audio in: the numpy contract of sc_pcm_decode (include/scasr.h).

A stream's input is described by (format, channels, channel, scale).  A chunk is n sample frames of ``channels``
interleaved little-endian codes.  Every step below is written out one code at a time, in Python integers and numpy scalars,
so that it can be read against the text of the contract; speechcatcher_amd/pcm.py restates it vectorised and the kernel
reproduces it bit for bit."""
import numpy as np

F32, S16LE, S24LE, U8, MULAW, ALAW = range(6)
FORMATS = (F32, S16LE, S24LE, U8, MULAW, ALAW)
MIX = -1
SCALE_FULL, SCALE_SERVER = 0, 1
CODE_BYTES = {F32: 4, S16LE: 2, S24LE: 3, U8: 1, MULAW: 1, ALAW: 1}
BITS = {S16LE: 15, S24LE: 23, U8: 7, MULAW: 15, ALAW: 15}
EXTREMES = {S16LE: (-32768, 32767), S24LE: (-(1 << 23), (1 << 23) - 1), U8: (-128, 127), MULAW: (-32124, 32124),
            ALAW: (-32256, 32256)}
CANONICAL_NAN = 0x7FC00000
ZERO_LEVEL = dict(frames=0, clipped=0, sum_abs=0, peak=0, full_scale=0)


def ulaw_value(b):
    u = ~b & 0xFF
    mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84
    return -mag if u & 0x80 else mag


def alaw_value(b):
    a = (b ^ 0x55) & 0xFF
    e = (a >> 4) & 7
    mag = ((a & 15) << 4) + 8 if e == 0 else (((a & 15) << 4) + 0x108) << (e - 1)
    return mag if a & 0x80 else -mag


def check_args(fmt, channels, channel, scale):
    if fmt not in FORMATS:
        raise ValueError(f"format {fmt} out of range")
    if not 1 <= channels <= 8:
        raise ValueError(f"channels {channels} outside 1..8")
    if not -1 <= channel < channels:
        raise ValueError(f"channel {channel} outside [-1, {channels})")
    if scale not in (SCALE_FULL, SCALE_SERVER) or (scale == SCALE_SERVER and BITS.get(fmt) != 15):
        raise ValueError(f"scale {scale} is not taken by format {fmt}")


def bytes_per_frame(fmt, channels):
    return CODE_BYTES[fmt] * channels


def code_value(code, fmt):
    """bytes of one integer code -> v"""
    if fmt == S16LE:
        return int.from_bytes(code, "little", signed=True)
    if fmt == S24LE:
        return int.from_bytes(code, "little", signed=True)
    if fmt == U8:
        return code[0] - 128
    if fmt == MULAW:
        return ulaw_value(code[0])
    if fmt == ALAW:
        return alaw_value(code[0])
    raise ValueError(fmt)


def frames_of(buf, fmt, channels):
    """-> list of frames, each a list of ``channels`` codes (bytes objects); trailing bytes of a partial frame are an error"""
    buf = bytes(buf)
    cb = CODE_BYTES[fmt]
    bpf = cb * channels
    if len(buf) % bpf:
        raise ValueError(f"{len(buf)} bytes are not a whole number of {bpf}-byte frames")
    return [[buf[i + c * cb: i + (c + 1) * cb] for c in range(channels)] for i in range(0, len(buf), bpf)]


def integer_m(frame, fmt, channel):
    """-> (m, C, clipped) of one frame of an integer format"""
    vs = [code_value(c, fmt) for c in frame]
    used = vs if channel == MIX else [vs[channel]]
    lo, hi = EXTREMES[fmt]
    return sum(used), len(used), any(v in (lo, hi) for v in used)


def decode(buf, fmt, channels=1, channel=MIX, scale=SCALE_FULL):
    """bytes -> float32 [n]"""
    check_args(fmt, channels, channel, scale)
    frames = frames_of(buf, fmt, channels)
    out = np.zeros(len(frames), np.float32)
    bits = out.view(np.uint32)
    for i, frame in enumerate(frames):
        if fmt == F32:
            if channel != MIX:
                bits[i] = int.from_bytes(frame[channel], "little")   # the bits, NaNs included
                continue
            vals = [np.frombuffer(c, "<f4")[0] for c in frame]
            with np.errstate(all="ignore"):
                s = np.float32(vals[0])
                for v in vals[1:]:
                    s = np.float32(s + v)                            # every add rounded
                r = np.float32(np.float64(s) / np.float64(channels))  # RN_fp32(s / C)
            if np.isnan(r):
                bits[i] = CANONICAL_NAN
            else:
                out[i] = r
            continue
        m, C, _ = integer_m(frame, fmt, channel)
        x = np.float32(np.float64(m) / np.float64(C))   # the exact quotient rounded once: 53 >= 2 * 24 + 2
        if scale == SCALE_SERVER:
            out[i] = np.float32(np.float16(x)) * np.float32(2.0 ** -15)
        else:
            out[i] = x * np.float32(2.0 ** -BITS[fmt])
    return out


def level(buf, fmt, channels=1, channel=MIX, scale=SCALE_FULL, prev=None):
    """the level record after ``buf``, continuing ``prev`` (None: the chunk starts an utterance)"""
    check_args(fmt, channels, channel, scale)
    lv = dict(ZERO_LEVEL if prev is None else prev)
    if fmt == F32:
        lv["full_scale"] = 0
        return lv
    C = channels if channel == MIX else 1
    for frame in frames_of(buf, fmt, channels):
        m, _, clip = integer_m(frame, fmt, channel)
        lv["frames"] += 1
        lv["peak"] = max(lv["peak"], abs(m))
        lv["sum_abs"] += abs(m)
        lv["clipped"] += 1 if clip else 0
    lv["full_scale"] = C << BITS[fmt]
    return lv

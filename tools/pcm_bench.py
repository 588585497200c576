"""Time of one sc_pcm_decode launch (one workgroup of 256 threads per job: coded bytes -> mono fp32 samples and the input
level) by hipEvents around the launch, with an empty event pair and the 16 kHz scatter copy of a float admission of the
same shape (sc_stage_bench) beside it in the same session.  The shapes are the headline regime's admissions: 58 and 128
jobs of 10 240 frames (640 ms at 16 kHz), as s16le mono, mu-law stereo with one channel selected and a three-channel
s24le mix.  Before every timed launch the bytes are written again by a device copy, as the admission's host-to-device
copy would have just done.  Prints one JSON line per shape and format.

    python tools/pcm_bench.py [--iters 20] [--frames 10240]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechcatcher_amd import _abi, pcm  # noqa: E402

FORMATS = (("s16le mono", pcm.S16LE, 1, 0, pcm.SCALE_FULL), ("mulaw stereo, channel 1", pcm.MULAW, 2, 1, pcm.SCALE_FULL),
           ("s24le 3 channels, mix", pcm.S24LE, 3, pcm.MIX, pcm.SCALE_FULL))


def bench(n, frames, fmt, iters, lib):
    name, f, ch, sel, scale = fmt
    dev = torch.device("cuda:0")
    bpf = pcm.bytes_per_frame(f, ch)
    stride = (frames * bpf + 3) & ~3                     # every chunk at a multiple of 4, as the engine stages them
    rng = np.random.default_rng(n * 7 + f)
    host = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    fresh = torch.from_numpy(host).to(dev)
    src = torch.zeros_like(fresh)
    dst = torch.zeros((n, frames), dtype=torch.float32, device=dev)
    level = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    after = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    tab = (_abi.PcmJob * n)()
    for k in range(n):
        j = tab[k]
        j.src, j.dst, j.level, j.level_after = src.data_ptr(), dst[k].data_ptr(), level[k].data_ptr(), after[k].data_ptr()
        j.offset, j.format, j.channels, j.channel, j.scale, j.n, j.restart = k * stride, f, ch, sel, scale, frames, 1
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
    s = torch.cuda.current_stream(dev)

    def launch():
        _abi.check(lib.sc_pcm_decode(tab_dev.data_ptr(), n, s.cuda_stream), "sc_pcm_decode")

    for _ in range(3):
        src.copy_(fresh)
        launch()
    torch.cuda.synchronize(dev)
    want = pcm.decode(host[0, :frames * bpf], f, ch, sel, scale)
    assert dst[0].cpu().numpy().tobytes() == want.tobytes()
    lv = np.frombuffer(after.cpu().numpy().tobytes(), [("q", "<i8", 3), ("i", "<i4", 2)])
    assert (lv["q"][:, 0] == frames).all()
    times = []
    for _ in range(iters):
        src.copy_(fresh)                                     # the bytes have just arrived
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        launch()
        b.record(s)
        b.synchronize()
        times.append(a.elapsed_time(b))
    t = np.array(times) * 1e3
    ms = (C.c_double * iters)()
    _abi.check(lib.sc_stage_bench(16000, n, frames, iters, ms), "sc_stage_bench")
    return {"jobs": n, "frames_per_job": frames, "format": name, "bytes_in": int(n * frames * bpf), "bytes_out": int(n * frames * 4),
            "us_median": round(float(np.median(t)), 2), "us_min": round(float(t.min()), 2), "us_max": round(float(t.max()), 2),
            "us_scatter_copy_median": round(float(np.median(np.array(ms[:]))) * 1e3, 2),
            "us_empty_event_pair": round(float(lib.sc_prof_event_overhead_ms(s.cuda_stream)) * 1e3, 2), "iters": iters,
            "source": "hipEvent around one sc_pcm_decode launch, the bytes rewritten before it; sc_stage_bench(16000) beside it"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=10240)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pcm_bench needs a ROCm GPU")
    lib = _abi.load()
    for n in (58, 128):
        for fmt in FORMATS:
            print(json.dumps(bench(n, args.frames, fmt, args.iters, lib)), flush=True)


if __name__ == "__main__":
    main()

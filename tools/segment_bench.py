"""Cost of the energy curve in front of file mode's cut search, host against GPU, for seeded int16
recordings of 10 min and 1 h: wall time of the host path (segmenter.smoothed_negative_energy), wall time of
hip_backend.segment_energy (upload and read-back included) and the hipEvent time of its two launches alone on
device-resident samples - all three in ONE process per length, each the median of --iters runs after one warm-up.  One
JSON line per length; it also carries the largest difference between the two curves and whether the cuts agree.

Every length runs in a child process of its own under `timeout`; a child that fails ends the run.

    python tools/segment_bench.py [--seconds 600 3600] [--iters 5]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def recording(seconds, seed=1):
    """speech-like envelope (on 0.3 + 0.002 of the time scale of sentences) times Gaussian noise at amplitude 8000"""
    import numpy as np
    n = seconds * 16000
    rng = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    env = (np.sin(2 * np.pi * t / 7.3) > 0.2) * 0.3 + 0.002
    return np.clip(np.rint(env * rng.standard_normal(n) * 8000.0), -32768, 32767).astype(np.int16)


def median_of(fn, iters):
    import numpy as np
    fn()                                   # warm-up
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def case(seconds, iters):
    import numpy as np
    import torch
    from speechcatcher_amd import _abi
    from speechcatcher_amd.hip_backend import segment_energy
    from speechcatcher_amd.segmenter import CutSearch, constrain_segments, smoothed_negative_energy
    if not torch.cuda.is_available():
        raise SystemExit("segment_bench needs a ROCm GPU")
    lib = _abi.load()
    x = recording(seconds)
    host_s = median_of(lambda: smoothed_negative_energy(x), iters)
    gpu_s = median_of(lambda: segment_energy(x), iters)
    # the two launches alone: samples and output resident, hipEvents around sc_segment_energy
    xd = torch.from_numpy(x).cuda()
    F = int(lib.sc_segment_frame_count(len(x)))
    out = torch.empty(F, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ms = []
    for it in range(iters + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        got = lib.sc_segment_energy(xd.data_ptr(), len(x), 1, out.data_ptr(), F, st)
        b.record()
        b.synchronize()
        if got != F:
            _abi.check(int(got) if got < 0 else -1, "sc_segment_energy")
        if it:
            ms.append(a.elapsed_time(b))
    host, gpu = smoothed_negative_energy(x), out.cpu().numpy()
    search = CutSearch(ideal_segment_len=6000, len_reward_weight=12.0)
    t0 = time.perf_counter()
    cuts_host = constrain_segments(search.search(host, len(host)))
    search_s = time.perf_counter() - t0
    cuts_gpu = constrain_segments(search.search(gpu, len(gpu)))
    return {"seconds": seconds, "frames": F, "host_wall_s": round(host_s, 4), "gpu_wall_s": round(gpu_s, 4),
            "gpu_launches_ms": round(float(np.median(ms)), 4), "host_over_gpu": round(host_s / gpu_s, 1),
            "cut_search_s": round(search_s, 4), "max_abs_diff": float(np.abs(host - gpu).max()),
            "same_cuts": cuts_host == cuts_gpu, "segments": len(cuts_host), "iters": iters,
            "source": "perf_counter around the call (wall), hipEvents around sc_segment_energy (launches)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, nargs="*", default=[600, 3600])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--case", type=int, default=0, help="(internal) run one length in this process")
    args = ap.parse_args()
    if args.case:
        print(json.dumps(case(args.case, args.iters)), flush=True)
        return 0
    for seconds in args.seconds:
        limit = 120 + seconds // 6        # the host path dominates: about 7 s per run for an hour of audio
        res = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", str(seconds),
                              "--iters", str(args.iters)], cwd=ROOT)
        if res.returncode != 0:
            print(f"segment_bench: the {seconds} s case ended with status {res.returncode}; stopping", file=sys.stderr)
            return res.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

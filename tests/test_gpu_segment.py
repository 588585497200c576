"""The energy curve of file mode on the GPU (csrc/segment.hip): both kernels against the float64 numpy
restatement of the contract (tests/segment_ref.py) at every length where they take another path, one frame's provenance,
the cuts of structured recordings against the host path, repeatability, the error paths and the CLI option."""
import functools
import json

import numpy as np
import pytest
import torch

import segment_ref as ref
from speechcatcher_amd import synth

pytestmark = pytest.mark.gpu

KERNEL_BAR = 1e-9    # absolute, on values of O(10-100): 5000 x what two float64 formulations differ by, 1/5000 of fp32's error


def energy_tile():
    """frames per workgroup of seg_energy_kernel (SEG_TILE)"""
    return 8


def smooth_tile():
    """outputs per workgroup of seg_smooth_kernel (SM_TILE), with a halo of 80 frames on each side"""
    return 256


def frame_counts():
    et, st = energy_tile(), smooth_tile()
    return (et - 1, et, et + 1, st - 1, st, st + 1, 2 * st + 81)


LENGTHS = ref.EDGE_LENGTHS + tuple(ref.samples_for_frames(F) for F in frame_counts())
SIGNALS = ("noise", "zeros", "alternating", "impulse_last", "constant")


def make(name, n):
    if name == "noise":
        x = np.random.RandomState(n).randn(n) * 3000.0
    elif name == "zeros":
        x = np.zeros(n)
    elif name == "alternating":
        x = np.where(np.arange(n) % 2 == 0, 32767.0, -32768.0)
    elif name == "impulse_last":
        x = np.zeros(n)
        x[-1] = 25000.0
    else:
        x = np.full(n, -4321.0)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """(p, y) of the contract for one test signal, computed once"""
    p = ref.raw_curve(make(name, n))
    y = ref.smooth(p)
    p.setflags(write=False)
    y.setflags(write=False)
    return p, y


def gpu_curve(x, smoothed):
    from speechcatcher_amd.hip_backend import segment_energy
    return segment_energy(x, smoothed=smoothed)


@pytest.mark.parametrize("smoothed", [0, 1])
def test_kernels_equal_the_float64_reference(smoothed):
    assert [ref.frame_count(n) for n in LENGTHS[len(ref.EDGE_LENGTHS):]] == list(frame_counts())
    worst = (-1.0, (0, ""))
    for n in LENGTHS:
        for name in SIGNALS:
            got, want = gpu_curve(make(name, n), bool(smoothed)), reference(name, n)[smoothed]
            assert got.dtype == np.float64 and got.shape == want.shape == (ref.frame_count(n),), (n, name)
            assert np.isfinite(got).all(), (n, name)
            err = float(np.abs(got - want).max())
            worst = max(worst, (err, (n, name)))
    print(f"smoothed={smoothed}: max |gpu - segment_ref| = {worst[0]:.3e} at {worst[1]} (bar {KERNEL_BAR:.0e})")
    assert worst[0] <= KERNEL_BAR, worst
    # the eps rule held in every frame of digital silence
    p0 = 26 * np.log(ref.EPS) / 10.0
    zeros = gpu_curve(make("zeros", LENGTHS[-1]), bool(smoothed))
    assert np.abs(zeros - (-p0 if smoothed else p0)).max() <= 1e-12


def test_one_frames_provenance():
    """zeros with one burst at samples 399..401: frame 0 sees sample 399 alone, frame 1 (samples 160..559) all three and
    their pre-emphasis tails, frame 2 (320..719) too, frame 3 (480..879) nothing - a wrong hop, a pre-emphasis slip at a
    frame start or a wrong padding moves a value from one frame to another."""
    n = ref.samples_for_frames(6) - 50                  # the last frame is padded behind the end
    x = np.zeros(n, np.int16)
    x[399:402] = (9000, -32768, 17000)
    got, want = gpu_curve(x, False), ref.raw_curve(x)
    assert got.shape == want.shape == (6,)
    silent = 26 * np.log(ref.EPS) / 10.0
    assert np.abs(got - want).max() <= KERNEL_BAR, (got, want)
    assert abs(want[3] - silent) < 1e-12 and np.all(want[:3] > silent + 50)        # what the reference itself says
    assert np.abs(got[3:] - silent).max() <= 1e-12 and np.all(got[:3] > silent + 50)
    # the burst as the LAST samples: the tail -0.97 x[n-1] is not part of the signal (zeros are appended after the pre-emphasis)
    x = np.zeros(561, np.int16)
    x[558:] = (9000, -32768, 17000)
    assert np.abs(gpu_curve(x, False) - ref.raw_curve(x)).max() <= KERNEL_BAR
    # ... and as the first: x[-1] is absent
    x = np.zeros(561, np.int16)
    x[:3] = (9000, -32768, 17000)
    assert np.abs(gpu_curve(x, False) - ref.raw_curve(x)).max() <= KERNEL_BAR


@pytest.mark.parametrize("kind", ["speechlike", "gaps"])
@pytest.mark.parametrize("seconds", [200, 300])
def test_cuts_of_structured_recordings_equal_the_host_cuts(kind, seconds):
    from speechcatcher_amd.segmenter import segment_speech
    x = ref.make_signal(kind, seconds * 16000, seed=seconds)
    host = segment_speech(x)
    assert len(host) >= 3 and host[0][0] == 0 and all(a[1] == b[0] for a, b in zip(host[:-1], host[1:]))
    assert segment_speech(x, segmentation="gpu") == host


def test_two_calls_return_identical_bytes():
    x = ref.make_signal("speechlike", 40 * 16000 + 123, seed=9)
    for smoothed in (False, True):
        a, b = gpu_curve(x, smoothed), gpu_curve(torch.from_numpy(x), smoothed)
        assert a.tobytes() == b.tobytes() and len(a) == ref.frame_count(len(x))
    from speechcatcher_amd.hip_backend import HipBackend, segment_energy
    assert callable(HipBackend.segment_energy) and segment_energy(x).tobytes() == gpu_curve(x, True).tobytes()


def test_error_paths_launch_nothing():
    from speechcatcher_amd import _abi
    from speechcatcher_amd.segmenter import smoothed_negative_energy
    lib = _abi.load()
    n = 13121                                                    # 81 frames
    x = torch.from_numpy(make("noise", n)).cuda()
    out = torch.full((128,), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for smoothed in (0, 1):
        assert lib.sc_segment_energy(x.data_ptr(), n, smoothed, out.data_ptr(), 80, st) == -1        # SC_ERR_ARG
        assert b"81" in lib.sc_last_error()
        assert lib.sc_segment_energy(None, n, smoothed, out.data_ptr(), 128, st) == -1
        assert lib.sc_segment_energy(x.data_ptr(), n, smoothed, None, 128, st) == -1
        assert lib.sc_segment_energy(x.data_ptr(), 0, smoothed, out.data_ptr(), 128, st) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                          # nothing was written
    with pytest.raises(ValueError, match="16 kHz"):
        smoothed_negative_energy(make("noise", n), 8000, backend="gpu")
    # a good call after the refused ones
    assert lib.sc_segment_energy(x.data_ptr(), n, 1, out.data_ptr(), 128, st) == 81
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.abs(got[:81] - reference("noise", n)[1]).max() <= KERNEL_BAR and np.isnan(got[81:]).all()


def test_cli_segmentation_option_round_trip(tmp_path):
    """a 61 s WAV (built like test_gpu_native.test_cli_round_trips_a_wav builds its own) through the CLI with
    --segmentation gpu and with the default: the .json files are equal"""
    import subprocess
    import sys
    import wave
    from conftest import ROOT
    from speechcatcher_amd.config import TINY
    mdir = synth.write_model_dir(tmp_path / "tiny", TINY, seed=1234, stats_kind="meanstd")
    rate = 16000
    x = synth.synth_audio(40, 61 * rate) * 20000
    for t0 in (18, 41):
        x[t0 * rate:(t0 + 2) * rate] *= 0.01
    x = x.astype(np.int16)
    outs = {}
    for mode in ("gpu", "host"):
        wav = tmp_path / f"rec_{mode}.wav"
        with wave.open(str(wav), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(rate)
            f.writeframes(x.tobytes())
        opt = ["--segmentation", "gpu"] if mode == "gpu" else []
        res = subprocess.run([sys.executable, "-m", "speechcatcher_amd", "-m", str(mdir), "-b", "3", "--quiet", "--no-progress",
                              *opt, str(wav)], cwd=str(ROOT), capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        outs[mode] = json.loads((tmp_path / f"rec_{mode}.wav.json").read_text())
    assert outs["gpu"] == outs["host"] and len(outs["gpu"]["complete_text"]) > 10

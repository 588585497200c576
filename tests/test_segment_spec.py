"""The energy curve of file mode without a GPU: the numpy restatement of the contract
(tests/segment_ref.py) against the host path, the host-side entry points of csrc/segment.hip (frame count, tables),
and the ``segmentation`` option of the segmenter."""
import ctypes as C
import functools

import numpy as np
import pytest

import segment_ref as ref
from speechcatcher_amd import segmenter

HOST_BAR = 1e-11     # absolute; two float64 formulations measured <= 1.5e-13 apart, fp32 lies 6e-6 .. 1.3e-5 away


@functools.lru_cache(maxsize=None)
def lib():
    from speechcatcher_amd import _abi
    if not _abi.LIB_PATH.exists():
        _abi.build()
    return _abi.load()


def _gap(x):
    got, want = ref.energy_curve(x), segmenter.smoothed_negative_energy(x)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape == (ref.frame_count(len(x)),)
    return float(np.abs(got - want).max())


@pytest.mark.parametrize("kind", ref.KINDS)
def test_reference_equals_the_host_path_on_90_s(kind):
    x = ref.make_signal(kind, 90 * 16000 + 37, seed=5)
    gap = _gap(x)
    print(f"{kind}: max |segment_ref - host| = {gap:.3e} over {ref.frame_count(len(x))} frames")
    assert gap <= HOST_BAR


def test_reference_equals_the_host_path_at_the_edge_lengths():
    assert [ref.frame_count(n) for n in ref.EDGE_LENGTHS] == [1, 1, 1, 2, 2, 3, 24, 80, 81]
    worst = 0.0
    for n in ref.EDGE_LENGTHS:
        for kind in ref.KINDS:
            gap = _gap(ref.make_signal(kind, n, seed=n))
            worst = max(worst, gap)
            assert gap <= HOST_BAR, (n, kind, gap)
    print(f"edge lengths: max |segment_ref - host| = {worst:.3e}")


def test_reflection_rule_equals_scipy():
    from scipy.ndimage import gaussian_filter1d
    for F in (1, 2, 3, 24, 80, 81):
        p = np.random.RandomState(F).randn(F) * 30.0
        assert np.abs(ref.smooth(p) + gaussian_filter1d(p, sigma=20)).max() <= 1e-12, F


def test_frame_count_entry_point():
    for n in ref.EDGE_LENGTHS + (16000 * 3600, 230_400_000):
        want = 1 if n <= 400 else 1 + -((-(n - 400)) // 160)
        assert lib().sc_segment_frame_count(n) == want == ref.frame_count(n), n
    for n in (0, -5):
        assert lib().sc_segment_frame_count(n) == -1          # SC_ERR_ARG
        assert b"sc_segment_frame_count" in lib().sc_last_error()


def test_design_tables():
    fb = np.full((26, 257), np.nan)
    gauss = np.full(161, np.nan)
    dp = C.POINTER(C.c_double)
    assert lib().sc_segment_design(fb.ctypes.data_as(dp), gauss.ctypes.data_as(dp)) == 0
    want = segmenter._mel_filterbank(26, 512, 16000)
    assert fb.shape == want.shape and fb.tobytes() == want.tobytes()      # ratios of small integers over equal bin edges
    w = ref.gauss_weights()
    assert np.abs(gauss / w - 1.0).max() <= 1e-15
    assert abs(gauss.sum() - 1.0) <= 1e-15 and gauss.tobytes() == gauss[::-1].tobytes()
    # either output may be left out
    fb2, g2 = np.zeros((26, 257)), np.zeros(161)
    assert lib().sc_segment_design(fb2.ctypes.data_as(dp), None) == 0 and fb2.tobytes() == fb.tobytes()
    assert lib().sc_segment_design(None, g2.ctypes.data_as(dp)) == 0 and g2.tobytes() == gauss.tobytes()
    assert lib().sc_segment_design(None, None) == 0


def test_kernel_level_argument_errors_launch_nothing():
    """null pointers, no samples, an output that is too small: refused on the host (this test has no GPU)"""
    L = lib()
    assert L.sc_segment_energy(None, 1000, 1, 8, 100, None) == -1 and b"null" in L.sc_last_error()
    assert L.sc_segment_energy(8, 1000, 1, None, 100, None) == -1 and b"null" in L.sc_last_error()
    assert L.sc_segment_energy(8, 0, 1, 8, 100, None) == -1
    assert L.sc_segment_energy(8, 13121, 0, 8, 80, None) == -1 and b"81" in L.sc_last_error()


def test_unknown_options_are_refused():
    x = ref.make_signal("speechlike", 4000, seed=1)
    with pytest.raises(ValueError, match="nonsense"):
        segmenter.segment_speech(x, 16000, segmentation="nonsense")
    with pytest.raises(ValueError, match="nonsense"):
        segmenter.smoothed_negative_energy(x, 16000, backend="nonsense")
    with pytest.raises(ValueError, match="16 kHz"):
        segmenter.smoothed_negative_energy(x, 8000, backend="gpu")
    with pytest.raises(ValueError, match="int16"):
        segmenter.smoothed_negative_energy(x.astype(np.float32), 16000, backend="gpu")
    assert segmenter.segment_speech(x, 16000, segmentation="host") == segmenter.segment_speech(x, 16000)
    from speechcatcher_amd.__main__ import make_parser
    assert make_parser().parse_args(["a.wav"]).segmentation == "host"
    assert make_parser().parse_args(["--segmentation", "gpu", "a.wav"]).segmentation == "gpu"


def test_recognize_recording_takes_the_host_option_and_gives_todays_result(monkeypatch):
    """61 s with digital-silence gaps on the scheduler's spec backend (CPU): the option spelled out gives what the
    default gives.  The spec backend is deterministic and slow (about 15 s for this recording), so the decode runs once:
    the second call must hand recognize_segments byte-identical audio, ranges and options, and then gets the first
    call's decode back."""
    from test_engine_spec import make_batch
    rate = 16000
    x = ref.make_signal("gaps", 61 * rate, seed=3)
    sb = make_batch("TINY", 1234, "meanstd", 1, True, n_streams=4, backend=None, device="cpu", max_frames=2000,
                    max_tokens=1200, pcm_capacity=1 << 21)
    real, calls = segmenter.recognize_segments, []

    def once(batch, speech, ranges, **kw):
        key = (np.asarray(speech).tobytes(), tuple(ranges), tuple(sorted((k, repr(v)) for k, v in kw.items())))
        if not calls:
            calls.append((key, real(batch, speech, ranges, **kw)))
        else:
            assert key == calls[0][0]
            calls.append((key, calls[0][1]))
        return calls[-1][1]

    monkeypatch.setattr(segmenter, "recognize_segments", once)
    today = segmenter.recognize_recording(sb, x, rate, chunk_length=8192, average_segment_length=20.0)
    spelled = segmenter.recognize_recording(sb, x, rate, chunk_length=8192, average_segment_length=20.0,
                                            segmentation="host")
    assert len(calls) == 2 and len(calls[0][0][1]) >= 2               # it was cut into segments
    assert today == spelled and len(today[1]) >= 1 and len(today[1][0]["tokens"]) > 10
    with pytest.raises(ValueError, match="nonsense"):
        segmenter.recognize_recording(sb, x, rate, segmentation="nonsense")
    assert len(calls) == 2

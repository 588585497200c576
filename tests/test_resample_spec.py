"""Sample-rate conversion without a GPU: the library's pure-host design and output counts against the
numpy spec (tests/resample_ref.py), the quality of the filter the library designs, the fp32 evaluation order's error
bound, and the plumbing of a session's sample rate through the scheduler, the server loop and the Python engine."""
import ctypes as C
import json

import numpy as np
import pytest

import resample_ref as ref

RATES = ref.RATES


def _lib():
    from speechcatcher_amd import _abi
    if not _abi.LIB_PATH.exists():
        _abi.build()
    return _abi.load()


_TABLES = {}


def lib_design(rate):
    """(L, M, Wc, f32 table [L][K]) of sc_resample_design, designed once per rate"""
    if rate not in _TABLES:
        lib = _lib()
        L, M, Wc = C.c_int32(), C.c_int32(), C.c_int32()
        assert lib.sc_resample_design(rate, C.byref(L), C.byref(M), C.byref(Wc), None) == 0
        coef = np.zeros((L.value, 2 * Wc.value), np.float32)
        assert lib.sc_resample_design(rate, None, None, None, coef.ctypes.data_as(C.POINTER(C.c_float))) == 0
        coef.setflags(write=False)
        _TABLES[rate] = (L.value, M.value, Wc.value, coef)
    return _TABLES[rate]


def test_spec_reproduces_the_sizes_of_the_contract():
    """the table of DESIGN 8b: (L, M, Wc) per rate"""
    want = {48000: (1, 3, 77), 44100: (160, 441, 71), 32000: (1, 2, 52), 22050: (320, 441, 36), 11025: (640, 441, 26),
            8000: (2, 1, 26)}
    for rate, lmw in want.items():
        assert ref.params(rate) == lmw


@pytest.mark.parametrize("rate", RATES)
def test_library_design_matches_the_spec(rate):
    L, M, Wc, coef = lib_design(rate)
    assert (L, M, Wc) == ref.params(rate)
    spec = ref.design(rate)
    assert coef.shape == spec.shape == (L, 2 * Wc)
    err = np.abs(coef.astype(np.float64) - spec).max()
    print(f"rate {rate}: max |coef - spec| = {err:.3e}")
    # two correct float64 evaluations round to neighbouring floats at worst: two f32 ulps at 1.0
    assert err <= 2.0 ** -23
    rows = np.abs(coef.astype(np.float64).sum(axis=1) - 1.0).max()
    print(f"rate {rate}: max |row sum - 1| = {rows:.3e}")
    assert rows <= 2 * Wc * 2.0 ** -24


@pytest.mark.parametrize("rate", [7999, 16001, 96000, 0])
def test_unsupported_rates_are_refused(rate):
    lib = _lib()
    L = C.c_int32()
    assert ref.params(rate) is None
    assert lib.sc_resample_design(rate, C.byref(L), None, None, None) == -1
    assert b"unsupported" in lib.sc_last_error()
    assert lib.sc_resample_out_count(rate, 1000, 1) < 0


@pytest.mark.parametrize("rate", RATES)
def test_output_counts(rate):
    lib = _lib()
    Wc = ref.params(rate)[2]
    for N in (0, 1, Wc - 1, Wc, Wc + 1, 997, 30720):
        for fin in (False, True):
            assert lib.sc_resample_out_count(rate, N, int(fin)) == ref.out_count(rate, N, fin), (rate, N, fin)
    # a call's output is the difference of the counts: over any split they add up to the one-shot count
    rng = np.random.RandomState(rate)
    cuts = np.sort(rng.randint(0, 30721, size=17))
    total = prev = 0
    for i, n in enumerate(list(cuts) + [30720]):
        cur = lib.sc_resample_out_count(rate, int(n), int(i == len(cuts)))
        assert cur >= prev
        total += cur - prev
        prev = cur
    assert total == ref.out_count(rate, 30720, True)


@pytest.mark.parametrize("rate", RATES)
def test_filter_quality_of_the_library_table(rate):
    """half a second of a unit sine through the library's f32 table, evaluated in float64: pass-band tones come out as the
    same sine sampled at 16 kHz (2e-5), tones above 8.6 kHz - which would alias - below -100 dB"""
    coef = lib_design(rate)[3]
    n = rate // 2
    t_in = np.arange(n) / rate
    for f in (100, 1000, 3000, 6000):
        if f >= rate / 2:
            continue
        y = ref.eval_f64(np.sin(2 * np.pi * f * t_in), rate, coef)
        want = np.sin(2 * np.pi * f * np.arange(len(y)) / 16000.0)
        err = np.abs(y - want)[200:-200].max()
        print(f"rate {rate}: {f} Hz pass-band error {err:.2e}")
        assert err <= 2e-5, (rate, f, err)
    for f in (8600, 9000, 12000, 20000):
        if f >= rate / 2:
            continue
        y = ref.eval_f64(np.sin(2 * np.pi * f * t_in), rate, coef)
        peak = np.abs(y)[200:-200].max()
        db = 20 * np.log10(max(peak, 1e-300))
        print(f"rate {rate}: {f} Hz stop-band {db:.1f} dB")
        assert db < -100.0, (rate, f, db)


@pytest.mark.parametrize("rate", RATES)
def test_fp32_order_is_within_the_bound_of_a_k_term_sum(rate):
    coef = lib_design(rate)[3]
    K = coef.shape[1]
    x = np.random.RandomState(rate + 1).randn(3000).astype(np.float32)
    y32 = ref.eval_f32(x, rate, coef)
    assert y32.dtype == np.float32
    y64 = ref.eval_f64(x, rate, coef)
    bound = (K + 1) * 2.0 ** -24 * ref.abs_products_f64(x, rate, coef)
    worst = (np.abs(y32.astype(np.float64) - y64) / np.maximum(bound, 1e-300)).max()
    print(f"rate {rate}: worst error / bound = {worst:.3f}")
    assert np.all(np.abs(y32.astype(np.float64) - y64) <= bound)


# ---- plumbing: scheduler, server loop, Python engine ---------------------------------------------------------------------
class _StubBatch:
    """records what the scheduler asks of a batch; every chunk is answered without output"""

    def __init__(self, n):
        self.S = n
        self.calls = []
        self.rates = {}

    def reset(self, slot):
        self.calls.append(("reset", slot))

    def set_input_rate(self, slot, rate):
        self.calls.append(("rate", slot, rate))
        self.rates[slot] = rate

    def push(self, items, isolate_faults=False):
        self.calls.append(("push", [(s, len(p), f) for s, p, f in items]))
        return {s: False for s, _, _ in items}


def test_scheduler_sets_the_slots_rate_and_sets_it_back():
    from speechcatcher_amd.scheduler import StreamScheduler
    b = _StubBatch(1)
    sch = StreamScheduler(b, result_format="espnet")
    sid = sch.open(sample_rate=8000)
    assert ("rate", 0, 8000) in b.calls and sch.sample_rate(sid) == 8000
    assert b.calls.index(("reset", 0)) < b.calls.index(("rate", 0, 8000))   # the rate is set on a reset stream
    sch.feed(sid, np.zeros(4000, np.float32), is_final=True)
    assert sch.step() == {sid: []}
    assert ("push", [(0, 4000, True)]) in b.calls                          # PCM goes down at the session's rate
    sch.close(sid)
    sid2 = sch.open()
    assert b.rates[0] == 16000 and sch.sample_rate(sid2) == 16000           # the next session did not ask: 16 kHz
    n_rate_calls = sum(1 for c in b.calls if c[0] == "rate")
    sch.close(sid2)
    sch.close(sch.open())
    assert sum(1 for c in b.calls if c[0] == "rate") == n_rate_calls        # nothing to set when it does not change
    with pytest.raises(ValueError, match="8000..48000"):
        sch.open(sample_rate=7000)
    assert len(sch._free) == 1                                              # the refused open took no slot


def test_scheduler_rate_changes_only_before_the_first_audio():
    from speechcatcher_amd.scheduler import StreamScheduler
    b = _StubBatch(2)
    sch = StreamScheduler(b, result_format="espnet")
    sid = sch.open()
    sch.set_sample_rate(sid, 48000)
    assert b.rates[0] == 48000
    sch.feed(sid, np.zeros(100, np.float32))
    sch.set_sample_rate(sid, 48000)                 # unchanged: fine
    with pytest.raises(ValueError, match="before its first audio"):
        sch.set_sample_rate(sid, 8000)


def test_server_session_honours_config_sample_rate():
    from speechcatcher_amd.scheduler import StreamScheduler
    from speechcatcher_amd.server_session import ServerLoop
    b = _StubBatch(2)
    loop = ServerLoop(StreamScheduler(b, result_format="espnet"), vosk_output_format=True, continuous=False)
    sid = loop.connect()
    loop.submit(sid, json.dumps({"config": {"sample_rate": 48000}}))
    loop.submit(sid, np.zeros(4800, np.int16).tobytes())
    replies = loop.step()[sid]
    assert not any(isinstance(r, Exception) for r in replies), replies     # 48000 no longer raises
    assert ("rate", 0, 48000) in b.calls
    assert ("push", [(0, 4800, False)]) in b.calls
    # an unsupported rate: this client's error reply names the supported range
    sid2 = loop.connect()
    loop.submit(sid2, json.dumps({"config": {"sample_rate": 7000}}))
    (err,) = loop.step()[sid2]
    assert isinstance(err, ValueError) and "8000..48000" in str(err)
    # ... and so does a change after the session's first audio
    loop.submit(sid, json.dumps({"config": {"sample_rate": 8000}}))
    (err,) = loop.step()[sid]
    assert isinstance(err, ValueError) and "before its first audio" in str(err)


def test_python_engine_refuses_other_rates():
    from speechcatcher_amd.engine import StreamBatch
    eng = object.__new__(StreamBatch)               # set_input_rate reads no state
    eng.set_input_rate(0, 16000)
    assert eng.input_rate(0) == 16000
    with pytest.raises(NotImplementedError, match="native engine"):
        eng.set_input_rate(0, 8000)


def test_output_clock_follows_the_count_formula():
    from speechcatcher_amd.resample import OutputClock, out_count, rate_params
    for rate in RATES:
        assert rate_params(rate) == ref.params(rate)
        clock, total = OutputClock(rate), 0
        for n, fin in ((1, False), (25, False), (997, False), (0, False), (4000, True)):
            total += clock.call(n, fin)
        assert total == (ref.out_count(rate, 5023, True) if rate != 16000 else 5023)
        assert out_count(rate, 5023, False) == (ref.out_count(rate, 5023, False) if rate != 16000 else 5023)

"""The float64 references of tests/frontend_ref.py against the torch spec on the CPU: the measured kappa of the fp32
reference arithmetic (kappa_ref), the golden log-mel fixture, deliberately wrong front-ends that the bound must reject,
the fp32 error of the spec's encoder layers, and the references of conv1 / block assembly / hand-off against their specs.
tests/test_gpu_encoder_input.py holds the HIP kernels to the same references."""
import numpy as np
import pytest
import torch

import frontend_ref as fr
from conftest import GOLDEN
from speechcatcher_amd import synth


@pytest.fixture(scope="module", autouse=True)
def _release_xl_weights():
    """the cached XL weights (host and device copies) go when this module is done"""
    yield
    fr._xl_packed.cache_clear()
    fr.xl_state_dict.cache_clear()


def _spec():
    from oracle.kernel_spec import SpecBackend
    return SpecBackend()


def _kappa_ref():
    """the smallest kappa at which the spec's fp32 torch.stft front-end holds the bound on every signal, job, geometry
    and MVN mode"""
    return max(fr.measure_kappa("spec", _spec().logmel).values())


# ---------------------------------------------------------------------------------------------------------------------
# an fp32 front-end in numpy with one switch per near-miss
# ---------------------------------------------------------------------------------------------------------------------
def _radix2_power_f32(xw, tw):
    """|X|^2 of float32 frames [n][N] by a decimation-in-time radix-2 transform in float32, every product and sum rounded
    (the order of an in-place LDS transform); tw [N/2][2] = (cos, -sin)"""
    n, N = xw.shape
    log2n = N.bit_length() - 1
    rev = np.array([int(format(i, f"0{log2n}b")[::-1], 2) for i in range(N)])
    re = np.zeros((n, N), np.float32)
    im = np.zeros((n, N), np.float32)
    re[:, rev] = xw
    t = np.arange(N // 2)
    for sft in range(1, log2n + 1):
        m, hm, tstep = 1 << sft, 1 << (sft - 1), N >> sft
        j = t % hm
        i0 = (t // hm) * m + j
        i1 = i0 + hm
        wr, wi = tw[j * tstep, 0][None, :], tw[j * tstep, 1][None, :]
        xr, xi = re[:, i1], im[:, i1]
        vr, vi = xr * wr - xi * wi, xr * wi + xi * wr
        ur, ui = re[:, i0].copy(), im[:, i0].copy()
        re[:, i0], im[:, i0] = ur + vr, ui + vi
        re[:, i1], im[:, i1] = ur - vr, ui - vi
    k = slice(0, N // 2 + 1)
    return re[:, k] * re[:, k] + im[:, k] * im[:, k]


def _variant_logmel(window_shift=0, bad_reflect=False, hop=None, twiddle_swap=None, mel_shift=0, fft="torch"):
    """-> a logmel(ns, pcm, pcap, jobs, n_jobs, max_keep, featbuf) in float32 with the kernel's framing; every switch at
    its default: a correct front-end"""
    def logmel(ns, pcm, pcap, jobs, n_jobs, max_keep, featbuf):
        cfg = ns.cfg
        N, win, half = cfg.n_fft, cfg.win_length, cfg.n_fft // 2
        hp = hop or cfg.hop_length
        w = np.zeros(N, np.float32)
        off = (N - win) // 2 + window_shift
        w[off:off + win] = ns.window.numpy()
        fb = ns.mel_fb.numpy()
        if mel_shift:
            fb = np.roll(fb, mel_shift, axis=0)
        tw = ns.twiddle.numpy().copy()
        if twiddle_swap is not None:
            tw[twiddle_swap] = tw[twiddle_swap + 1]
        x_all = pcm.numpy()
        for s, start, seg_len, eff, lo, keep, dst0, _ in jobs.numpy()[:n_jobs].tolist():
            n = np.abs((lo + np.arange(keep))[:, None] * hp + np.arange(N)[None, :] - half)
            n = np.where(n >= eff, (2 * eff if bad_reflect else 2 * (eff - 1)) - n, n)
            inside = (n >= 0) & (n < seg_len)
            v = np.where(inside, x_all[s, start + np.clip(n, 0, seg_len - 1)], np.float32(0))
            xw = (v * w[None, :]).astype(np.float32)
            if fft == "torch":
                X = torch.fft.rfft(torch.from_numpy(xw), dim=1)
                power = (X.real ** 2 + X.imag ** 2).numpy()
            else:
                power = _radix2_power_f32(xw, tw)
            mel = torch.from_numpy(np.maximum(power @ fb, np.float32(1e-10))).log()
            if ns.has_mvn and ns.mvn_is_f64:
                mel = ((mel.to(torch.float64) - ns.mean64) / ns.std64).to(torch.float32)
            elif ns.has_mvn:
                mel = (mel - ns.mean64.to(torch.float32)) / ns.std64.to(torch.float32)
            featbuf[dst0:dst0 + keep] = mel
    return logmel


NEAR_MISSES = {
    "window_shifted_one_sample": dict(window_shift=1),
    "reflection_without_minus_one": dict(bad_reflect=True),
    "hop_159": dict(hop=159),
    "twiddle_entry_is_its_neighbour": dict(twiddle_swap=37, fft="radix2"),
    "mel_matrix_shifted_one_bin": dict(mel_shift=1),
}


# ---------------------------------------------------------------------------------------------------------------------
def test_signals_sit_where_they_are_meant_to():
    """zeros and sigma = 1e-6 noise: every bin at the clamp; sigma = 1e-5: some bins clamp and some do not; the int16
    signal holds both ends of the grid"""
    def clamped(sig):
        return fr.logmel_ref_of("model", sig)[1].M < fr.CLAMP
    assert clamped("zeros").all() and clamped("noise_1e-6").all()
    c = clamped("noise_1e-5")
    assert c.any() and not c.all()
    assert not clamped("noise")[:26].any()      # (the 26 frames of the whole-signal job)
    s = fr.signals()
    assert all(v.dtype == np.float32 and len(v) == fr.SIG_LEN for v in s.values()) and len(s) == 12
    sp = s["speech_int16"].astype(np.float64) * 32768
    assert np.array_equal(sp, np.round(sp)) and sp.min() == -32768 and sp.max() == 32767


def test_job_table_covers_the_cases():
    n_fft, win, hop, _ = fr.GEOMS["model"]
    case = fr.logmel_case("model", fr.signals()["noise"])
    j = case.jobs
    assert case.stride > j[:, 2].max() and len(set(j[:, 0])) == len(j) > 1
    assert 1 in j[:, 5] and case.max_keep in j[:, 5] and case.max_keep > 1
    assert (j[:, 4] > 0).any() and (j[:, 1] > 0).any()
    short = j[j[:, 3] == win]
    assert sorted(short[:, 2]) == [1, 159, 400]
    assert ((j[:, 2] == 4000) & (j[:, 3] == 4000)).any()
    for s, start, seg_len, *_ in j.tolist():      # NaN everywhere outside the segment, finite inside
        fin = np.isfinite(case.pcm[s])
        assert fin[start:start + seg_len].all() and fin.sum() == seg_len


def test_float64_reference_reproduces_the_golden_logmel():
    """tests/golden/frontend.npz logmel_10480 (recorded from the reference implementation) within the tolerance
    test_frontend_counts_and_values uses"""
    want = np.load(GOLDEN / "frontend.npz")["logmel_10480"]
    audio = synth.synth_audio(7, 64000)[:10480]
    t = fr.frontend_tables("model")
    jobs = np.array([[0, 0, 10480, 10480, 0, 1 + 10480 // 160, 0, 0]], np.int32)
    ref = fr.logmel_ref(audio[None, :], jobs, "model", t.window.numpy(), t.mel_fb.numpy())
    assert ref.lg.shape == want.shape
    np.testing.assert_allclose(ref.lg, want, atol=1e-4, rtol=0)


def test_kappa_ref_of_the_spec_front_end(capsys):
    """kappa_ref: measured on SpecBackend.logmel (fp32 torch.stft, the reference's own arithmetic).  The spec also leaves
    every row outside the jobs alone and never reads outside a segment (the NaN canaries)."""
    spec = _spec()
    table = fr.measure_kappa("spec", spec.logmel)
    assert all(np.isfinite(v) for v in table.values()), {k: v for k, v in table.items() if not np.isfinite(v)}
    kref = _kappa_ref()
    per_signal = {sig: max(v for (g, m, s), v in table.items() if s == sig) for sig in fr.signals()}
    per_geom = {g: max(v for (gg, m, s), v in table.items() if gg == g) for g in fr.GEOMS}
    with capsys.disabled():
        print(f"\nkappa_ref = {kref:.3f}; per geometry: " + ", ".join(f"{g} {v:.3f}" for g, v in per_geom.items()))
        print("per signal: " + ", ".join(f"{s} {v:.3f}" for s, v in per_signal.items()))
    assert kref > 0
    for geom in fr.GEOMS:
        case, ref = fr.logmel_ref_of(geom, "noise")
        feat = fr.run_logmel(spec.logmel, fr.frontend_namespace(geom, 1), case)
        assert fr.untouched_rows_intact(feat, ref) and np.isfinite(feat[ref.rows]).all()


@pytest.mark.parametrize("fft", ["torch", "radix2"])
def test_correct_fp32_front_ends_hold_the_bound(fft, capsys):
    """the numpy front-end the near-misses are cut from, with every switch off: within 4 x kappa_ref on every signal,
    geometry and MVN mode - with torch's transform and with the float32 radix-2 in-place order"""
    table = fr.measure_kappa(None, _variant_logmel(fft=fft))
    kref = _kappa_ref()
    with capsys.disabled():
        print(f"\n{fft}: kappa {max(table.values()):.3f} (kappa_ref {kref:.3f}); worst " + str(max(table, key=table.get)))
    assert max(table.values()) <= 4 * kref, sorted(table.items(), key=lambda kv: -kv[1])[:5]


@pytest.mark.parametrize("name", list(NEAR_MISSES))
def test_the_bound_rejects_near_misses(name, capsys):
    """each wrong front-end must break the bound at 4 x kappa_ref on the noise and on the speech-like signal"""
    kref = _kappa_ref()
    got = fr.measure_kappa(None, _variant_logmel(**NEAR_MISSES[name]), geoms=("model",), modes=(0, 1, 2),
                           names=("noise", "speech_int16"))
    with capsys.disabled():
        print(f"\n{name}: " + ", ".join(f"{s}/mvn{m} {v:.3g}" for (g, m, s), v in got.items()) + f" (4 kappa_ref = {4 * kref:.3f})")
    for key, v in got.items():
        assert v > 4 * kref, (key, v, kref)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels,d", [(80, 64), (83, 256), (7, 320)])
def test_conv1_reference_against_the_spec(n_mels, d):
    case = fr.conv1_case(n_mels, d)
    rows, val, tol = fr.conv1_ref(case)
    assert len(set(rows.tolist())) == len(rows)
    assert 0.35 < float((val == 0).mean()) < 0.65          # about half the pre-activations are negative
    c1 = fr.run_conv1(_spec().conv1, case)
    assert (np.abs(c1[rows] - val) <= tol).all()
    rest = np.ones(case.n_rows, bool)
    rest[rows] = False
    assert rest.any() and (c1[rest] == np.float32(fr.SENTINEL)).all()


@pytest.mark.parametrize("name", list(fr.BLOCK_PACK_LAUNCHES))
@pytest.mark.parametrize("d", [64, 320])
def test_block_pack_reference_against_the_spec(name, d):
    case = fr.block_pack_case(name, d)
    val, tol, written = fr.block_pack_ref(case)
    x = fr.run_block_pack(_spec().block_pack, case)
    assert (np.abs(x[written] - val[written]) <= tol[written]).all()
    assert (x[~written] == np.float32(fr.SENTINEL)).all() and (~written).sum() >= 2
    zero = written & (tol.max(axis=1) == 0)
    assert (x[zero] == 0).all() and (zero.any() or name != "regular")


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("layer", [0, 2])
def test_ctx_handoff_reference_is_the_spec(layer, flip):
    R, d, n_layers = 6, 64, 3
    jobs, free, n_streams = fr.chain_table(12, n_layers, flip)
    rng = np.random.RandomState(5)
    x0 = rng.randn(12 * R, d).astype(np.float32)
    st0 = rng.randn(n_streams * n_layers, d).astype(np.float32)
    x, st = x0.copy(), st0.copy()
    fr.ctx_handoff_ref(x, R, jobs, st, layer)
    xs, ss = torch.from_numpy(x0.copy()), torch.from_numpy(st0.copy())
    _spec().ctx_handoff(xs, R, torch.from_numpy(jobs), len(jobs), ss, layer)
    assert x.tobytes() == xs.numpy().tobytes() and st.tobytes() == ss.numpy().tobytes()
    assert x.tobytes() != x0.tobytes()
    for b in free:
        assert x[b * R:(b + 1) * R].tobytes() == x0[b * R:(b + 1) * R].tobytes()


@pytest.mark.parametrize("n_layers", [1, 3])
def test_fp32_error_of_the_spec_encoder_layers(n_layers, capsys):
    """max abs error of SpecBackend.encoder_layers (fp32 torch) against the float64 layer on the inputs of the GPU test:
    the yardstick the HIP layers are held to (4 x this)"""
    w = fr.xl_weights(n_layers)
    cfg = w.cfg
    worst = 0.0
    for flip in (False, True):
        case = fr.encoder_case(n_layers, flip)
        x32, s32 = fr.run_encoder_layers(_spec(), w, case)
        x64, s64 = fr.encoder_layers_f64(fr.enc_layers_as_numpy(w), case.x0, case.nblk, case.R, cfg.enc_heads, True,
                                         case.jobs, case.state0, cfg.ln_eps)
        ex, es = float(np.abs(x32 - x64).max()), float(np.abs(s32 - s64).max())
        scale = float(np.abs(x64).max())
        with capsys.disabled():
            print(f"\nspec encoder layers, {n_layers} layer(s), flip {flip}: max|x err| {ex:.3e}, max|state err| {es:.3e}, "
                  f"max|x| {scale:.3f}")
        assert 0 < ex <= 1e-3 * scale and es <= 1e-3 * scale
        worst = max(worst, ex, es)
    assert np.isfinite(worst)

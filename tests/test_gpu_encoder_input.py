"""What every frame passes before the first matrix kernel, each HIP kernel on its own against the float64 references of
tests/frontend_ref.py: sc_logmel (error model with a measured kappa), sc_conv1 and sc_block_pack (derived tolerances),
the context hand-off bit for bit - sc_ctx_handoff alone and both forms inside sc_encoder_layers (fused into the
feed-forward's reduce / separate launches) - and the matrix-core encoder attention at its 16-row tile edges.
tests/test_frontend_ref_spec.py holds the references themselves to the torch spec on the CPU."""
import functools

import numpy as np
import pytest
import torch

import frontend_ref as fr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend(DEV)


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
    and MVN mode (measured here, on the CPU of the machine the kernels run on)"""
    return max(fr.measure_kappa("spec", _spec().logmel).values())


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("geom", list(fr.GEOMS))
def test_logmel_against_float64(hip, geom, mode, capsys):
    """sc_logmel per signal: one launch over six jobs on six streams (keep_n = 1 beside max_keep, trimmed head,
    zero-padded final short segments, the right-hand reflection, seg_start > 0).  Every output is finite although all PCM
    outside the segments is NaN, lies within the error model at 4 x kappa_ref, and no row outside the jobs is written."""
    kref = _kappa_ref()
    ns = fr.frontend_namespace(geom, mode, DEV)
    mean, std = fr.mvn_stats(ns.cfg.n_mels, mode)
    kappas, bad = {}, []
    for sig in fr.signals():
        case, ref = fr.logmel_ref_of(geom, sig)
        feat = fr.run_logmel(hip.logmel, ns, case, DEV)
        if not fr.untouched_rows_intact(feat, ref):
            bad.append((sig, "a row outside the jobs was written"))
        if not np.isfinite(feat[ref.rows]).all():
            bad.append((sig, "non-finite output: read outside the segment"))
        kappas[sig] = ref.kappa_needed(feat[ref.rows], mode, mean, std)
        if not kappas[sig] <= 4 * kref:
            err = np.abs(feat[ref.rows] - ref.value(mode, mean, std)) / ref.tol(4 * kref, mode, mean, std)
            bad.append((sig, f"kappa {kappas[sig]:.3g} > 4 x {kref:.3f}; worst element {np.unravel_index(np.nanargmax(err), err.shape)}"))
    with capsys.disabled():
        print(f"\nsc_logmel {geom} mvn{mode}: kappa_ref {kref:.3f}; kernel kappa " +
              ", ".join(f"{s} {k:.3f}" for s, k in kappas.items()))
    assert not bad, bad


@pytest.mark.parametrize("d", [64, 256, 320])
@pytest.mark.parametrize("n_mels", [80, 83, 7])
def test_conv1_against_float64(hip, n_mels, d):
    """sc_conv1 against float64 conv2d + ReLU within 12 * 2^-24 (sum |x||w| + |b|): three jobs in one launch (T1 = 9, 3, 1,
    overlapping source rows), d beyond the block size, an odd number of mel bins, half the pre-activations negative"""
    case = fr.conv1_case(n_mels, d)
    rows, val, tol = fr.conv1_ref(case)
    c1 = fr.run_conv1(hip.conv1, case, DEV)
    err = np.abs(c1[rows] - val)
    assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())
    rest = np.ones(case.n_rows, bool)
    rest[rows] = False
    assert (c1[rest] == np.float32(fr.SENTINEL)).all()


@pytest.mark.parametrize("d", [64, 256, 320])
@pytest.mark.parametrize("name", list(fr.BLOCK_PACK_LAUNCHES))
def test_block_pack_against_float64(hip, name, d):
    """sc_block_pack against float64 (body rows 3 * 2^-24 (sqrt(d)|v| + |pe|), context row (clen + 4) * 2^-24 (...)):
    inputs 100 + N(0, 1), clen 1 / 7 / R - 2, non-zero PE offsets; slot 0 and the rows behind the chunk exactly 0 over a
    non-zero pre-fill; the short path writes clen rows and nothing else"""
    case = fr.block_pack_case(name, d)
    val, tol, written = fr.block_pack_ref(case)
    x = fr.run_block_pack(hip.block_pack, case, DEV)
    err = np.abs(x[written] - val[written])
    assert (err <= tol[written]).all(), float((err - tol[written]).max())
    zero = written & (tol.max(axis=1) == 0)
    assert (x[zero] == 0).all()
    assert (x[~written] == np.float32(fr.SENTINEL)).all()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("layer", [0, 2])
@pytest.mark.parametrize("d", [64, 256])
def test_ctx_handoff_bit_for_bit(hip, d, layer, flip):
    """sc_ctx_handoff against the spec, byte for byte on x and state: chains of 1, 2 and 5 blocks listed in non-ascending
    block order, saved state valid and invalid (flip swaps them), two blocks outside every chain, state rows of other
    streams and layers"""
    R, n_layers = 6, 3
    jobs, free, n_streams = fr.chain_table(12, n_layers, flip)
    rng = np.random.RandomState(11 + d)
    x0 = rng.randn(12 * R, d).astype(np.float32)
    st0 = rng.randn(n_streams * n_layers, d).astype(np.float32)
    xs, ss = torch.from_numpy(x0.copy()), torch.from_numpy(st0.copy())
    _spec().ctx_handoff(xs, R, torch.from_numpy(jobs), len(jobs), ss, layer)
    xg, sg = torch.from_numpy(x0.copy()).to(DEV), torch.from_numpy(st0.copy()).to(DEV)
    hip.ctx_handoff(xg, R, torch.from_numpy(jobs).to(DEV), len(jobs), sg, layer)
    torch.cuda.synchronize()
    xg, sg = xg.cpu().numpy(), sg.cpu().numpy()
    assert xg.tobytes() == xs.numpy().tobytes() and sg.tobytes() == ss.numpy().tobytes()
    for b in free:
        assert xg[b * R:(b + 1) * R].tobytes() == x0[b * R:(b + 1) * R].tobytes()
    named = {int(j[2]) + layer for j in jobs}
    for r in range(len(st0)):
        assert (r in named) or sg[r].tobytes() == st0[r].tobytes()


@functools.lru_cache(maxsize=None)
def _encoder_reference(n_layers, flip):
    """-> (float64 x, float64 state, max abs error of the fp32 spec against them) on the CPU"""
    w = fr.xl_weights(n_layers)
    case = fr.encoder_case(n_layers, flip)
    x64, s64 = fr.encoder_layers_f64(fr.enc_layers_as_numpy(w), case.x0, case.nblk, case.R, w.cfg.enc_heads, True, case.jobs,
                                     case.state0, w.cfg.ln_eps)
    x32, s32 = fr.run_encoder_layers(_spec(), w, case)
    return x64, s64, max(float(np.abs(x32 - x64).max()), float(np.abs(s32 - s64).max()))


def _check_chains(case, x, st):
    """the hand-off's invariants on one output, no reference needed"""
    R, L = case.R, case.n_layers
    xb = x.reshape(case.nblk, R, -1)
    for b0, nbk, srow, has in case.jobs.tolist():
        for i in range(1, nbk):
            assert xb[b0 + i, 0].tobytes() == xb[b0 + i - 1, R - 1].tobytes(), (b0, i)
        assert st[srow + L - 1].tobytes() == xb[b0 + nbk - 1, R - 1].tobytes(), b0
        first = case.state0[srow + L - 1] if has else xb[b0, R - 1]
        assert xb[b0, 0].tobytes() == first.tobytes(), (b0, has)
    named = {int(j[2]) + li for j in case.jobs for li in range(L)}
    for r in range(len(st)):
        assert (r in named) or st[r].tobytes() == case.state0[r].tobytes(), r


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("n_layers", [1, 3])
def test_encoder_layers_handoff_paths(hip, n_layers, flip, capsys):
    """sc_encoder_layers at the XL dims (d 256, F 2048, 8 heads; 7 blocks of 42 rows) with chains of 3, 1 and 1 blocks in
    non-ascending order and two blocks outside every chain: with the default workspace (hand-off fused into the
    feed-forward's reduce), with a workspace too small for one slab (fused feed-forward in slabs, sc_ctx_handoff launches)
    and with the default again.  The chains' invariants hold byte for byte, blocks outside the chains come out as a
    layer without any hand-off leaves them, both paths give the same bytes (sums never depend on how rows are
    batched), and the result lies within 4 x the fp32 spec's own error of the float64 layer."""
    case = fr.encoder_case(n_layers, flip)
    w = fr.xl_weights(n_layers, DEV)
    cfg = w.cfg
    M, d, F = case.nblk * case.R, cfg.d_model, cfg.ffn_dim
    small = 2 << 20
    assert (F // 128) * 80 * d * 4 <= small < (F // 128) * M * d * 4 <= hip.workspace.numel()
    graphs, hip.use_graphs = hip.use_graphs, False     # the graph key does not include the workspace
    try:
        fused = fr.run_encoder_layers(hip, w, case, DEV)
        plain = fr.run_encoder_layers(hip, w, case, DEV, jobs=case.jobs[:0])
        hip._chk(hip.lib.sc_set_workspace(hip.workspace.data_ptr(), small), "sc_set_workspace")
        separate = fr.run_encoder_layers(hip, w, case, DEV)
        plain_small = fr.run_encoder_layers(hip, w, case, DEV, jobs=case.jobs[:0])
    finally:
        hip._chk(hip.lib.sc_set_workspace(hip.workspace.data_ptr(), hip.workspace.numel()), "sc_set_workspace")
        hip.use_graphs = graphs
    again = fr.run_encoder_layers(hip, w, case, DEV)
    R = case.R
    for name, (x, st) in (("fused", fused), ("separate", separate)):
        _check_chains(case, x, st)
        for b in case.free:
            assert x[b * R:(b + 1) * R].tobytes() == plain[0][b * R:(b + 1) * R].tobytes(), (name, b)
    assert plain[1].tobytes() == case.state0.tobytes() and plain_small[1].tobytes() == case.state0.tobytes()
    assert plain[0].tobytes() == plain_small[0].tobytes(), float(np.abs(plain[0] - plain_small[0]).max())
    assert fused[0].tobytes() == separate[0].tobytes(), float(np.abs(fused[0] - separate[0]).max())
    assert fused[1].tobytes() == separate[1].tobytes()
    assert fused[0].tobytes() == again[0].tobytes() and fused[1].tobytes() == again[1].tobytes()
    x64, s64, e32 = _encoder_reference(n_layers, flip)
    ex, es = float(np.abs(fused[0] - x64).max()), float(np.abs(fused[1] - s64).max())
    with capsys.disabled():
        print(f"\nsc_encoder_layers {n_layers} layer(s), flip {flip}: max|x err| {ex:.3e}, max|state err| {es:.3e} against "
              f"float64; fp32 spec {e32:.3e}")
    assert ex <= 4 * e32 and es <= 4 * e32, (ex, es, e32)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("R", [15, 16, 17, 31, 32, 33, 47, 48, 49])
def test_enc_attention_tile_edges(hip, monkeypatch, R, masked):
    """the default encoder attention around the 16-row tiles of the matrix-core kernel (R <= 48) and across its upper
    limit, against float64: the inputs and tolerance of test_gpu_ops.test_enc_attention"""
    monkeypatch.delenv("SC_ENC_ATTN", raising=False)
    H, dk, nblk = 8, 32, 3
    d = H * dk
    g = torch.Generator().manual_seed(201)
    qkv = torch.randn(nblk * R, 3 * d, generator=g).float()
    qkv[:, :d] *= 3.0   # peaked softmax rows as well
    ref = fr.block_attention_f64(qkv.numpy(), nblk, R, H, masked)
    out = torch.full((nblk * R + 2, d), 3.0, device=DEV)
    hip.enc_attention(qkv.to(DEV), out, nblk, R, H, masked)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out[:nblk * R].cpu().numpy(), ref, atol=5e-5, rtol=5e-5)
    assert float(out[nblk * R:].min()) == 3.0 and float(out[nblk * R:].max()) == 3.0

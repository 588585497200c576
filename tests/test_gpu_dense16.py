"""The reduced-precision forms of the dense kernels of csrc/gemm.hip - sc_gemm with SC_GEMM_SPLIT16, sc_rowtile_proj_s / _h,
sc_ffn_ln_s / _h, and sc_ffn_ln_handoff with split16 / float16 weights through sc_encoder_layers - each launch on its own
against the float64 references and the error model of tests/dense16_ref.py.  It mirrors tests/test_gpu_dense.py.  Per launch:
  * every named output is finite although everything the launch must not read is NaN - rows no table entry names, the columns
    behind K, row 0 of A where a gather entry is -1, the head of the split-K workspace (0xFF bytes before each launch);
  * every output lies within 4 x kappa_ref of the float64 reference, kappa_ref = the kappa the numpy transcription of the
    form's documented arithmetic needs on the same case (measured here, on the CPU); below 2^-14 the model holds the split
    form to its 2^-36 floor (families small / mixed / edge);
  * every sentinel keeps its bits, every read-only input too (the fp16 weight buffers compared as int16).
And the bit promises of DESIGN.md "Canonical summation" for these forms, compared as integers: the forced forms of the
feed-forward and row-tile kernels (every row-tile height the dispatcher may choose for that weight form), rows alone and
through a reversed table, the GEMM's row count, tile size and workspace size.  The numbers are left in the report
dense16_parity.json (test_gpu_ops.write_report).  tests/test_dense16_ref_spec.py holds the references to the fp32 spec."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dense16_ref as d16
import frontend_ref as fr
from test_gpu_encoder_input import _check_chains, _encoder_reference
from test_gpu_ops import write_report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WS_POISON = 8 << 20          # >= 8 planes of the largest GEMM case, 16 of the largest feed-forward (81 x 256)
REPORT = {"kappa": {}, "worst_ratio": {}, "bit_identities": {}, "encoder_layers": {}}
FFN_KERNELS, ROWTILE_KERNELS = ("ffn_s", "ffn_h"), ("rowtile_s", "rowtile_h")


@pytest.fixture(scope="module")
def hip():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend(DEV)


@pytest.fixture(scope="module", autouse=True)
def _release_weights():
    yield
    fr._xl_packed.cache_clear()
    fr.xl_state_dict.cache_clear()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _launch(hip, case, t):
    hip.workspace[:WS_POISON].fill_(0xFF)                      # partial sums of an earlier launch must not leak
    d16.launch(hip, case, t)
    torch.cuda.synchronize()


def _run_case(hip, case, **over):
    t = d16.tensors(case, DEV)
    t.update(over)
    _launch(hip, case, t)
    return t


def _identity(name, bad):
    """records the outcome of a bit identity in the report and asserts it"""
    REPORT["bit_identities"][name] = "same bits" if not bad else f"DIFFERS {bad}"
    write_report("dense16_parity", REPORT)
    assert not bad, (name, bad)


def _randn(g, *shape, scale=1.0, shift=0.0):
    return (shift + scale * torch.randn(*shape, generator=g)).to(DEV)


@pytest.mark.parametrize("kernel", d16.KERNELS)
def test_kernels_against_float64(hip, capsys, kernel):
    """every launch of the kernel's case list: finite, within 4 x kappa_ref, sentinels and read-only inputs bit for bit"""
    bad, rep, worst = [], {}, 0.0
    for case in d16.cases_of(kernel):
        kref = d16.kappa_ref(case)
        t = d16.tensors(case, DEV)
        readonly = {n: t[n].clone() for n in (*case.inputs, *case.tables)}
        _launch(hip, case, t)
        bufs = d16.outputs(case, t)
        k = case.kappas_of_buffers(bufs)
        rep[case.name] = {n: {"kappa_ref": kref[n], "kappa_kernel": k[n]} for n in k}
        for n in k:
            print(f"{case.name} {n}: kappa_ref {kref[n]:.4g} kernel {k[n]:.4g}")
            if not math.isfinite(k[n]):
                bad.append((case.name, n, "non-finite output: a masked or out-of-range row entered a product"))
            elif not k[n] <= 4 * kref[n]:
                bad.append((case.name, n, f"kappa {k[n]:.3g} > 4 x kappa_ref {kref[n]:.3g}"))
            if math.isfinite(k[n]) and kref[n] > 0:
                worst = max(worst, k[n] / kref[n])
        bad.extend((case.name, m) for m in case.sentinel_problems(bufs))
        bad.extend((case.name, f"{n}: a read-only input changed") for n, v in readonly.items() if not _same(v, t[n]))
    REPORT["kappa"][kernel], REPORT["worst_ratio"][kernel] = rep, worst
    write_report("dense16_parity", REPORT)
    with capsys.disabled():
        kr = [v["kappa_ref"] for c in rep.values() for v in c.values()]
        kk = [v["kappa_kernel"] for c in rep.values() for v in c.values()]
        print(f"\n{kernel}: {len(rep)} launches, kappa_ref {min(kr):.3g} .. {max(kr):.3g}, kernel kappa {min(kk):.3g} .. "
              f"{max(kk):.3g}, worst kernel / kappa_ref {worst:.3g} (limit 4)")
        for b in bad:
            print("  FAILED", b)
    assert not bad, bad


def _rtt_max(kernel, D):
    """ffn_rtt_max of csrc/gemm.hip: the tallest row tile (16 * rtt rows) the dispatcher may choose for the weight form"""
    return 3 if kernel == "ffn_s" and D == 256 else 5


@pytest.mark.parametrize("M,D,F", [(49, 256, 2048), (81, 128, 384), (17, 256, 256), (80, 128, 128)])
@pytest.mark.parametrize("kernel", FFN_KERNELS)
def test_feed_forward_forced_forms(hip, monkeypatch, kernel, M, D, F):
    """sc_ffn_ln_s / _h under SC_FFN_FORCE = rtt,cpw: every row-tile height of the weight form and one chunk or an aligned pair
    per workgroup give the same bits for X and ln_out (the second accumulator set is folded in per chunk, whatever the shape);
    X is the same with and without the LayerNorm output"""
    case = d16.Case(kernel, 0, M=M, D=D, F=F, ln=True, table=False, family="unit")
    noln = d16.Case(kernel, 0, M=M, D=D, F=F, ln=False, table=False, family="unit")
    monkeypatch.delenv("SC_FFN_FORCE", raising=False)
    ref = _run_case(hip, case)
    assert bool(torch.isfinite(ref["X"][:M]).all())
    bad = [] if _same(_run_case(hip, noln)["X"], ref["X"]) else ["default form without the LayerNorm output"]
    forms = [(r, c) for r in range(1, _rtt_max(kernel, D) + 1) for c in (1, 2) if (F // 128) % c == 0]
    for rtt, cpw in forms:
        monkeypatch.setenv("SC_FFN_FORCE", f"{rtt},{cpw}")
        t = _run_case(hip, case)
        if not (_same(t["X"], ref["X"]) and _same(t["ln_out"], ref["ln_out"])):
            bad.append((rtt, cpw))
        if not _same(_run_case(hip, noln)["X"], ref["X"]):
            bad.append((rtt, cpw, "without the LayerNorm output"))
    _identity(f"{kernel} M={M} D={D} F={F}: forced forms {forms} and the default, with and without ln_out", bad)


@pytest.mark.parametrize("M,D", [(49, 256), (65, 128)])
@pytest.mark.parametrize("kernel", ROWTILE_KERNELS)
def test_row_tile_forced_forms(hip, monkeypatch, kernel, M, D):
    """sc_rowtile_proj_s / _h under SC_ROWTILE_FORCE: every tile height of the weight form (1..4; 1..3 for the fp16 form with
    residual at D = 256: its fp16 tile copy puts 64 rows beyond the LDS, rowtile_run) and every cpw that divides N / 128"""
    bad, all_forms = [], []
    for form, N in (("qkv", 3 * D), ("qkv", D), ("out", D)):
        case = d16.Case(kernel, 0, M=M, D=D, N=N, form=form, ld=True, family="unit")
        monkeypatch.delenv("SC_ROWTILE_FORCE", raising=False)
        ref = _run_case(hip, case)
        nch = N // 128
        rtt_max = 3 if (kernel, form, D) == ("rowtile_h", "out", 256) else 4
        forms = [(r, c) for r in range(1, rtt_max + 1) for c in (range(1, nch + 1) if form == "qkv" else (nch,)) if nch % c == 0]
        all_forms.append((form, N, forms))
        for rtt, cpw in forms:
            monkeypatch.setenv("SC_ROWTILE_FORCE", f"{rtt},{cpw}")
            t = _run_case(hip, case)
            if not all(_same(t[n], ref[n]) for n in case.ref):
                bad.append((form, N, rtt, cpw))
    _identity(f"{kernel} M={M} D={D}: forced forms {all_forms} and the default", bad)


def test_rows_do_not_depend_on_their_neighbours(hip):
    """rows of an M = 49 launch of every feed-forward and row-tile form == the same rows launched alone (M = 1) and, for the
    feed-forward, through a row table in reversed order"""
    bad = []
    for kernel in FFN_KERNELS:
        for p in (dict(D=256, F=2048, ln=True), dict(D=128, F=384, ln=True)):
            case = d16.Case(kernel, 0, M=49, table=False, family="unit", **p)
            full = _run_case(hip, case)
            rev = torch.arange(48, -1, -1, dtype=torch.int32, device=DEV)
            t = _run_case(hip, case, rows=rev)
            if not all(_same(t[n], full[n]) for n in case.ref):
                bad.append((case.name, "row table in reversed order"))
            one = d16.Case(kernel, 0, **{**case.p, "M": 1})       # (the launch reads M from the case; the buffers stay this case's)
            for r in (0, 15, 16, 47, 48):
                t = d16.tensors(case, DEV)
                t["rows"] = torch.tensor([r], dtype=torch.int32, device=DEV)
                _launch(hip, one, t)
                if not all(_same(t[n][r], full[n][r]) for n in case.ref):
                    bad.append((case.name, f"row {r} alone"))
    for kernel in ROWTILE_KERNELS:                             # no row table here: the rows alone, through the base pointers
        for form, N in (("qkv", 768), ("out", 256)):
            case = d16.Case(kernel, 0, M=49, D=256, N=N, form=form, ld=False, family="unit")
            full = _run_case(hip, case)
            one = d16.Case(kernel, 0, M=1, D=256, N=N, form=form, ld=False, family="unit")
            for r in (0, 15, 16, 47, 48):
                t = d16.tensors(case, DEV)
                t1 = {**t, "A": t["A"][r:], "C": t["C"][r:]}
                if "LN2" in t:
                    t1["LN2"] = t["LN2"][r:]
                _launch(hip, one, t1)
                if not all(_same(t[n][r], full[n][r]) for n in case.ref):
                    bad.append((case.name, f"row {r} alone"))
    _identity("ffn_s / ffn_h / rowtile_s / rowtile_h M=49: rows == the rows alone (M=1) and through a reversed row table", bad)


def _gemm_rows(hip, A, W, b, M, N, K):
    Cm = torch.full((M, N), d16.SENTINEL, device=DEV)
    hip.workspace[:WS_POISON].fill_(0xFF)
    hip.gemm(A, None, K, W, b, Cm, None, N, M, N, K, split16=True)
    torch.cuda.synchronize()
    return Cm


def _kinds(hip):
    NK = 13
    ms, fl, by, nn = (C.c_double * NK)(), (C.c_double * NK)(), (C.c_double * NK)(), (C.c_longlong * NK)()
    assert hip.lib.sc_prof_collect_kinds(ms, fl, by, nn, NK) == 0
    return [int(v) for v in nn]


@pytest.mark.parametrize("N,K", [(68, 64), (256, 2560), (64, 4864)])
def test_gemm_rows_do_not_depend_on_the_row_count(hip, N, K):
    """split16: the rows of an M = 129 launch == the same rows computed in launches of M = 1, 33 and 65"""
    g = torch.Generator().manual_seed(K + N)
    A, W, b = _randn(g, 129, K), _randn(g, N, K, scale=K ** -0.5), _randn(g, N)
    full = _gemm_rows(hip, A, W, b, 129, N, K)
    assert bool(torch.isfinite(full).all())
    bad = [m for m in (1, 33, 65) if not _same(_gemm_rows(hip, A[:m].contiguous(), W, b, m, N, K), full[:m])]
    bad += [f"rows {a}.." for a in (64, 128) if not _same(_gemm_rows(hip, A[a:].contiguous(), W, b, 129 - a, N, K), full[a:])]
    _identity(f"gemm_s N={N} K={K}: rows of M=129 == launches of M=1, 33, 65 and of the rows from 64 / 128 on", bad)


def test_gemm_tile_size_does_not_change_the_bits(hip):
    """split16, 8192 x 1024 at K = 64: the cost model of gemm_dispatch takes the 128-row tile (confirmed through the per-kind
    launch counts); its rows == the same rows in an M = 129 launch, which takes the 64-row tile"""
    M, N, K = 8192, 1024, 64
    g = torch.Generator().manual_seed(5)
    A, W, b = _randn(g, M, K), _randn(g, N, K, scale=K ** -0.5), _randn(g, N)
    _kinds(hip)                                                # (drops what an earlier test may have left)
    try:
        hip.lib.sc_prof_enable(1)
        big = _gemm_rows(hip, A, W, b, M, N, K)
        kinds_big = _kinds(hip)
        head = _gemm_rows(hip, A[:129].contiguous(), W, b, 129, N, K)
        tail = _gemm_rows(hip, A[-65:].contiguous(), W, b, 65, N, K)
        kinds_small = _kinds(hip)
    finally:
        hip.lib.sc_prof_enable(0)
        _kinds(hip)
    REPORT["tile_kinds"] = {"M=8192": kinds_big[:4], "M=129 and 65": kinds_small[:4]}
    assert kinds_big[2] == 1 and kinds_big[3] == 0 and kinds_small[2] == 0 and kinds_small[3] == 2, (kinds_big, kinds_small)
    bad = [n for n, ok in (("first 129 rows", _same(big[:129], head)), ("last 65 rows", _same(big[-65:], tail))) if not ok]
    _identity("gemm_s 8192x1024x64 (128-row tile) == the same rows in M=129 / M=65 launches (64-row tile)", bad)


def test_workspace_size_does_not_change_the_k_cut(hip):
    """split16 sc_gemm at (200, 256, 2560) with the full workspace and with 1 MiB (8 partial planes of 200 rows do not fit: row
    slabs of 128): one set of bits"""
    M, N, K = 200, 256, 2560
    g = torch.Generator().manual_seed(9)
    A, W, b, C0 = _randn(g, M, K), _randn(g, N, K, scale=K ** -0.5), _randn(g, N), _randn(g, M, N)
    small = 1 << 20
    assert 8 * 128 * N * 4 <= small < 8 * M * N * 4

    def run():
        hip.workspace[:WS_POISON].fill_(0xFF)
        Cg = C0.clone()
        hip.gemm(A, None, K, W, b, Cg, None, N, M, N, K, residual=True, split16=True)
        torch.cuda.synchronize()
        return Cg

    try:
        full = run()
        hip._chk(hip.lib.sc_set_workspace(hip.workspace.data_ptr(), small), "sc_set_workspace")
        slabs = run()
    finally:
        hip._chk(hip.lib.sc_set_workspace(hip.workspace.data_ptr(), hip.workspace.numel()), "sc_set_workspace")
    assert bool(torch.isfinite(full).all()) and bool(torch.isfinite(slabs).all())
    _identity("gemm_s (200, 256, 2560): full workspace == 1 MiB workspace (row slabs)",
              [] if _same(slabs, full) else [int((_bits(slabs) != _bits(full)).sum())])


@pytest.mark.parametrize("n_layers", [1, 3])
@pytest.mark.parametrize("dtype", ["split16", "float16"])
def test_encoder_layers_handoff_paths(hip, dtype, n_layers, capsys):
    """sc_encoder_layers with split16 and with float16 weights on the case of
    test_gpu_encoder_input.test_encoder_layers_handoff_paths (sc_ffn_ln_handoff with wf = 2 / 1): the chains' invariants,
    blocks outside every chain equal to the run without hand-off jobs, the fused hand-off equal to separate sc_ctx_handoff
    launches (small workspace), repeatability - byte for byte; split16 also within 4 x the fp32 spec's own error of float64
    (the form promises fp32 grade)"""
    flip = False
    case = fr.encoder_case(n_layers, flip)
    w = fr.xl_weights(n_layers, DEV, dtype)
    assert all(("w1_s" in lw and "wqkv_s" in lw) if dtype == "split16" else ("w1_h" in lw and "wqkv_h" in lw) for lw in w.enc)
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
    assert np.isfinite(fused[0]).all() and np.isfinite(fused[1]).all()
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
    REPORT["encoder_layers"][f"{dtype}, {n_layers} layer(s)"] = {"max_abs_err_x": ex, "max_abs_err_state": es, "fp32_spec": e32,
                                                                "bytes": "chains, free blocks, fused == separate, repeatable"}
    write_report("dense16_parity", REPORT)
    with capsys.disabled():
        print(f"\nsc_encoder_layers {dtype}, {n_layers} layer(s): max|x err| {ex:.3e}, max|state err| {es:.3e} against float64; "
              f"fp32 spec {e32:.3e}")
    if dtype == "split16":
        assert ex <= 4 * e32 and es <= 4 * e32, (ex, es, e32)

"""The dense fp32 kernels of csrc/gemm.hip and csrc/decoder_panel.hip, each launch on its own against the float64 references of
tests/dense_ref.py: sc_gemm (tile edges of the 64- and 128-row tiles, the K edges of the split, scalar fallbacks, leading
dimensions, gather / scatter tables with -1 entries, the implicit conv), sc_gemm_ln (the LayerNorm fused into the reduce and as
a launch of its own; N > 1024 refused with nothing written), sc_rowtile_proj (both forms), sc_ffn_ln, sc_proj_ln_proj and
sc_ffn_ln_proj.  Where tests/test_gpu_ops.py compares N(0,1) operands with the fp32 torch
spec at 2e-4 .. 6e-4, here per launch:
  * every named output is finite although everything the operation must not read is NaN - the rows no table entry names, the
    columns behind K, row 0 of A where a gather entry is -1, and the head of the split-K workspace (0xFF bytes before each launch);
  * every output lies within the error model at 4 x kappa_ref, kappa_ref = the larger of the kappas the fp32 torch spec and the
    fp32 transcription of the documented summation order need on the same case, measured here on the CPU;
  * every sentinel keeps its bits (rows nobody names, columns behind N, rows of c_rows = -1), every read-only input too.
And the bit promises of DESIGN.md section 4 "Canonical summation" for these kernels, compared as integers: tiled == scalar chain,
no dependence on the row count, the tile size, the forced forms of the feed-forward and row-tile kernels, or the workspace size.
The numbers are left in the report dense_parity.json (test_gpu_ops.write_report).  tests/test_dense_ref_spec.py holds the references themselves to the spec."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dense_ref as dr
from speechcatcher_amd._abi import ScasrError
from test_gpu_ops import write_report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WS_POISON = 8 << 20          # >= 8 planes of the largest GEMM case (129 x 1028), 16 of the largest feed-forward (81 x 256)
REPORT = {"kappa": {}, "worst_ratio": {}, "bit_identities": {}}


@pytest.fixture(scope="module")
def hip():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _launch(hip, case, t, naive=False):
    hip.workspace[:WS_POISON].fill_(0xFF)                      # partial sums of an earlier launch must not leak
    dr.launch(hip, case, t, naive=naive)
    torch.cuda.synchronize()


def _identity(name, bad):
    """records the outcome of a bit identity in the report and asserts it"""
    REPORT["bit_identities"][name] = "same bits" if not bad else f"DIFFERS {bad}"
    write_report("dense_parity", REPORT)
    assert not bad, (name, bad)


def _randn(g, *shape, scale=1.0, shift=0.0):
    return (shift + scale * torch.randn(*shape, generator=g)).to(DEV)


@pytest.mark.parametrize("kernel", dr.KERNELS)
def test_kernels_against_float64(hip, capsys, kernel):
    """every launch of the kernel's case list: finite, within 4 x kappa_ref, sentinels and read-only inputs bit for bit"""
    bad, rep, worst = [], {}, 0.0
    for case in dr.cases_of(kernel):
        kref = dr.kappa_ref(case)
        t = dr.tensors(case, DEV)
        readonly = {n: t[n].clone() for n in (*case.inputs, *case.tables)}
        if case.refused:         # beyond what the kernels cover: an error, and nothing written (not a partial result)
            with pytest.raises(ScasrError):
                _launch(hip, case, t)
            torch.cuda.synchronize()
            rep[case.name] = "refused"
            bad.extend((case.name, f"{n}: written by a refused call") for n in case.ref
                       if not np.array_equal(t[n].cpu().numpy().view(np.int32), case.init[n].view(np.int32)))
            continue
        _launch(hip, case, t)
        bufs = dr.outputs(case, t)
        k = case.kappas_of_buffers(bufs)
        keys = ("kappa_spec", "kappa_transcription", "kappa_ref", "kappa_kernel")
        rep[case.name] = {n: dict(zip(keys, (*kref[n], k[n]))) for n in k}
        for n in k:
            if not math.isfinite(k[n]):
                bad.append((case.name, n, "non-finite output: a masked or out-of-range row entered a product"))
            elif not k[n] <= 4 * kref[n][2]:
                bad.append((case.name, n, f"kappa {k[n]:.3g} > 4 x kappa_ref {kref[n][2]:.3g}"))
            if math.isfinite(k[n]) and kref[n][2] > 0:
                worst = max(worst, k[n] / kref[n][2])
        bad.extend((case.name, m) for m in case.sentinel_problems(bufs))
        bad.extend((case.name, f"{n}: a read-only input changed") for n, v in readonly.items() if not _same(v, t[n]))
    REPORT["kappa"][kernel], REPORT["worst_ratio"][kernel] = rep, worst
    write_report("dense_parity", REPORT)
    with capsys.disabled():
        kr = [v["kappa_ref"] for c in rep.values() if c != "refused" for v in c.values()]
        kk = [v["kappa_kernel"] for c in rep.values() if c != "refused" for v in c.values()]
        print(f"\n{kernel}: {len(rep)} launches, kappa_ref {min(kr):.3g} .. {max(kr):.3g}, kernel kappa {min(kk):.3g} .. "
              f"{max(kk):.3g}, worst kernel / kappa_ref {worst:.3g} (limit 4)")
        for b in bad:
            print("  FAILED", b)
    assert not bad, bad


def _aligned(p):
    lda = p.get("lda", p["K"])
    return p["K"] % 32 == 0 and lda % 4 == 0 and (not p.get("conv") or lda % 32 == 0)


def test_tiled_gemm_is_the_scalar_chain(hip):
    """sc_gemm tiled == sc_gemm(naive) bit for bit on every aligned case below the K split, in all three modes"""
    bad, n = [], 0
    for i, (kernel, p) in enumerate(dr.case_params()):
        if kernel != "gemm" or not _aligned(p) or p["K"] >= 2560:
            continue
        for mode in dr.MODES:
            case = dr.Case("gemm", i, **{**p, "mode": mode})
            outs = []
            for naive in (False, True):
                t = dr.tensors(case, DEV)
                _launch(hip, case, t, naive=naive)
                outs.append(t["C"])
            n += 1
            if not _same(*outs):
                bad.append((case.name, int((_bits(outs[0]) != _bits(outs[1])).sum())))
    assert n >= 60
    _identity("gemm: tiled == scalar k-ordered chain (aligned cases, K < 2560, three modes, tables, conv offsets)", bad)


def _gemm_rows(hip, A, W, b, M, N, K):
    Cm = torch.full((M, N), dr.SENTINEL, device=DEV)
    hip.workspace[:WS_POISON].fill_(0xFF)
    hip.gemm(A, None, K, W, b, Cm, None, N, M, N, K)
    torch.cuda.synchronize()
    return Cm


def _kinds(hip):
    NK = 13
    ms, fl, by, nn = (C.c_double * NK)(), (C.c_double * NK)(), (C.c_double * NK)(), (C.c_longlong * NK)()
    assert hip.lib.sc_prof_collect_kinds(ms, fl, by, nn, NK) == 0
    return [int(v) for v in nn]


@pytest.mark.parametrize("N,K", [(68, 64), (256, 2560), (64, 4864)])
def test_gemm_rows_do_not_depend_on_the_row_count(hip, N, K):
    """the rows of an M = 129 launch == the same rows computed in launches of M = 1, 33 and 65"""
    g = torch.Generator().manual_seed(K + N)
    A, W, b = _randn(g, 129, K), _randn(g, N, K, scale=K ** -0.5), _randn(g, N)
    full = _gemm_rows(hip, A, W, b, 129, N, K)
    assert bool(torch.isfinite(full).all())
    bad = [m for m in (1, 33, 65) if not _same(_gemm_rows(hip, A[:m].contiguous(), W, b, m, N, K), full[:m])]
    bad += [f"rows {a}.." for a in (64, 128) if not _same(_gemm_rows(hip, A[a:].contiguous(), W, b, 129 - a, N, K), full[a:])]
    _identity(f"gemm N={N} K={K}: rows of M=129 == launches of M=1, 33, 65 and of the rows from 64 / 128 on", bad)


def test_gemm_tile_size_does_not_change_the_bits(hip):
    """8192 x 1024 at K = 64: the cost model of gemm_dispatch takes the 128-row tile (confirmed through the per-kind launch
    counts); its rows == the same rows in an M = 129 launch, which takes the 64-row tile"""
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
    _identity("gemm 8192x1024x64 (128-row tile) == the same rows in M=129 / M=65 launches (64-row tile)", bad)


def _run_case(hip, case, **over):
    t = dr.tensors(case, DEV)
    t.update(over)
    _launch(hip, case, t)
    return t


@pytest.mark.parametrize("M,D,F", [(49, 256, 2048), (81, 128, 384), (17, 256, 256), (80, 128, 128)])
def test_feed_forward_forced_forms(hip, monkeypatch, M, D, F):
    """sc_ffn_ln under SC_FFN_FORCE = rtt,cpw: every row-tile height and one chunk or an aligned pair per workgroup give the
    same bits for X and ln_out; X is the same with and without the LayerNorm output"""
    case = dr.Case("ffn", 0, M=M, D=D, F=F, ln=True, table=False, family="unit")
    noln = dr.Case("ffn", 0, M=M, D=D, F=F, ln=False, table=False, family="unit")
    monkeypatch.delenv("SC_FFN_FORCE", raising=False)
    ref = _run_case(hip, case)
    assert bool(torch.isfinite(ref["X"][:M]).all())
    bad = [] if _same(_run_case(hip, noln)["X"], ref["X"]) else ["default form without the LayerNorm output"]
    forms = [(r, c) for r in range(1, 6) for c in (1, 2) if (F // 128) % c == 0]
    for rtt, cpw in forms:
        monkeypatch.setenv("SC_FFN_FORCE", f"{rtt},{cpw}")
        t = _run_case(hip, case)
        if not (_same(t["X"], ref["X"]) and _same(t["ln_out"], ref["ln_out"])):
            bad.append((rtt, cpw))
        if not _same(_run_case(hip, noln)["X"], ref["X"]):
            bad.append((rtt, cpw, "without the LayerNorm output"))
    _identity(f"ffn M={M} D={D} F={F}: forced forms {forms} and the default, with and without ln_out", bad)


@pytest.mark.parametrize("M,D", [(49, 256), (65, 128)])
def test_row_tile_forced_forms(hip, monkeypatch, M, D):
    """sc_rowtile_proj under SC_ROWTILE_FORCE: tile heights 1..4 and every cpw that divides N / 128 (form without residual)"""
    bad, all_forms = [], []
    for form, N in (("qkv", 3 * D), ("qkv", D), ("out", D)):
        case = dr.Case("rowtile", 0, M=M, D=D, N=N, form=form, ld=True, family="unit")
        monkeypatch.delenv("SC_ROWTILE_FORCE", raising=False)
        ref = _run_case(hip, case)
        nch = N // 128
        forms = [(r, c) for r in range(1, 5) for c in (range(1, nch + 1) if form == "qkv" else (nch,)) if nch % c == 0]
        all_forms.append((form, N, forms))
        for rtt, cpw in forms:
            monkeypatch.setenv("SC_ROWTILE_FORCE", f"{rtt},{cpw}")
            t = _run_case(hip, case)
            if not all(_same(t[n], ref[n]) for n in case.ref):
                bad.append((form, N, rtt, cpw))
    _identity(f"rowtile M={M} D={D}: forced forms {all_forms} and the default", bad)


def _table_launches(hip, case, full, names):
    """the launch again through a row table in reversed order, and single rows alone: the named outputs' rows keep their bits"""
    M, bad = case.p["M"], []
    rev = torch.arange(M - 1, -1, -1, dtype=torch.int32, device=DEV)
    t = _run_case(hip, case, rows=rev)
    if not all(_same(t[n], full[n]) for n in names):
        bad.append("row table in reversed order")
    for r in (0, 15, 16, 48):
        one = dr.Case(case.kernel, 0, **{**case.p, "M": 1})    # (the launch reads M from the case; the buffers stay this case's)
        t = dr.tensors(case, DEV)
        t["rows"] = torch.tensor([r], dtype=torch.int32, device=DEV)
        _launch(hip, one, t)
        if not all(_same(t[n][r], full[n][r]) for n in names):
            bad.append(f"row {r} alone")
    return bad


def test_rows_do_not_depend_on_their_neighbours(hip):
    """rows of an M = 49 feed-forward, row-tile and panel launch == the same rows launched alone (M = 1) and through a row table
    in another order"""
    bad = []
    for kernel, p in (("ffn", dict(D=256, F=2048, ln=True)), ("ffn", dict(D=128, F=384, ln=True)),
                      ("panel", dict(D=256, second=True)), ("panel", dict(D=64, second=False)),
                      ("ffn_proj", dict(D=256, F=2048, N=768))):
        case = dr.Case(kernel, 0, M=49, table=False, family="unit", **p)
        full = _run_case(hip, case)
        bad += [(case.name, m) for m in _table_launches(hip, case, full, tuple(case.ref))]
    for form, N in (("qkv", 768), ("out", 256)):               # no row table here: the rows alone, through the base pointers
        case = dr.Case("rowtile", 0, M=49, D=256, N=N, form=form, ld=False, family="unit")
        full = _run_case(hip, case)
        one = dr.Case("rowtile", 0, M=1, D=256, N=N, form=form, ld=False, family="unit")
        for r in (0, 15, 16, 48):
            t = dr.tensors(case, DEV)
            t1 = {**t, "A": t["A"][r:], "C": t["C"][r:]}
            if "LN2" in t:
                t1["LN2"] = t["LN2"][r:]
            _launch(hip, one, t1)
            if not all(_same(t[n][r], full[n][r]) for n in case.ref):
                bad.append((case.name, f"row {r} alone"))
    _identity("ffn / ffn_proj / panel / rowtile M=49: rows == the rows alone (M=1) and through a reversed row table", bad)


def test_workspace_size_does_not_change_the_k_cut(hip):
    """sc_gemm and sc_gemm_ln at (200, 256, 2560) with the full workspace and with 1 MiB (8 partial planes of 200 rows do not
    fit: row slabs of 128): one set of bits for C, ln_out the same at both sizes"""
    M, N, K = 200, 256, 2560
    g = torch.Generator().manual_seed(9)
    A, W, b = _randn(g, M, K), _randn(g, N, K, scale=K ** -0.5), _randn(g, N)
    C0, lg, lb = _randn(g, M, N), _randn(g, N, scale=0.1, shift=1.0), _randn(g, N)
    small = 1 << 20
    assert 8 * 128 * N * 4 <= small < 8 * M * N * 4

    def run():
        hip.workspace[:WS_POISON].fill_(0xFF)
        Cg, Cl, L = C0.clone(), C0.clone(), torch.full((M, N), dr.SENTINEL, device=DEV)
        hip.gemm(A, None, K, W, b, Cg, None, N, M, N, K, residual=True)
        hip.gemm_ln(A, None, K, W, b, Cl, None, N, M, N, K, lg, lb, L, residual=True)
        torch.cuda.synchronize()
        return Cg, Cl, L

    graphs, hip.use_graphs = hip.use_graphs, False
    try:
        full = run()
        hip._chk(hip.lib.sc_set_workspace(hip.workspace.data_ptr(), small), "sc_set_workspace")
        slabs = run()
    finally:
        hip._chk(hip.lib.sc_set_workspace(hip.workspace.data_ptr(), hip.workspace.numel()), "sc_set_workspace")
        hip.use_graphs = graphs
    assert all(bool(torch.isfinite(x).all()) for x in (*full, *slabs))
    bad = []
    if not _same(full[0], full[1]):
        bad.append("full workspace: C of sc_gemm_ln != C of sc_gemm")
    if not _same(slabs[0], full[0]):
        bad.append("sc_gemm: 1 MiB workspace != full workspace")
    if not _same(slabs[1], full[0]):
        bad.append("sc_gemm_ln: C at the 1 MiB workspace != sc_gemm (the K cut gave way to the row count)")
    if not _same(slabs[2], full[2]):
        bad.append("sc_gemm_ln: ln_out at the 1 MiB workspace != full workspace")
    _identity("gemm / gemm_ln (200, 256, 2560): full workspace == 1 MiB workspace (row slabs), C of both entry points", bad)

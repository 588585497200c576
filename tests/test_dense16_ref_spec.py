"""tests/dense16_ref.py on the CPU: the float64 references of the split16 / float16 dense forms against the fp32 torch spec
(oracle/kernel_spec.py on the unsplit weights, the fp32 error model), the coverage of the case list, the transcriptions of the
forms (finite everywhere; this run measures kappa_ref for tests/test_gpu_dense16.py, which measures it again on the machine the
kernels run on), the planted mistakes - each must rise above the 4 x kappa_ref the GPU test allows, on every kernel it applies
to - split_panel_weight against the representation bound of the error model, and the `small` family reaching the 2^-36 floor."""
import math

import numpy as np
import pytest
import torch

import dense16_ref as d16
import dense_ref as dr


@pytest.mark.parametrize("kernel", d16.KERNELS)
def test_references_against_the_spec(kernel, capsys):
    """fp32 model: spec kappa <= 4 x the kappa of dense_ref's fp32 transcription on every output of every case, and the spec
    is finite on every poisoned case.  (`_h` cases: the spec computes with the fp16 weight VALUES in fp32.)"""
    rows, bad = [], []
    for case in d16.cases_of(kernel):
        ks, kt = d16.spec_kappas(case), case.kappas_of_rows(case.transcription32(), fp32=True)
        for name in ks:
            rows.append((case.name, name, ks[name], kt[name]))
            if not math.isfinite(ks[name]):
                bad.append((case.name, name, "the spec reads a poisoned element (or the reference is not finite)"))
            elif not (math.isfinite(kt[name]) and ks[name] <= 4 * kt[name]):
                bad.append((case.name, name, f"spec kappa {ks[name]:.3g} > 4 x fp32 transcription kappa {kt[name]:.3g}"))
    with capsys.disabled():
        print(f"\nfp32 model, {kernel}: {len(rows)} outputs of {len(d16.cases_of(kernel))} launches")
        for cn, n, ks, kt in rows:
            print(f"  {cn} {n}: spec {ks:.3g} fp32 transcription {kt:.3g}")
    assert not bad, bad


def test_cases_cover_kernels_families_edges_and_poison():
    assert {c.kernel16 for c in d16.all_cases()} == set(d16.KERNELS)
    for kernel in d16.KERNELS:                                   # every kernel x every family at least twice
        fams = [c.family for c in d16.cases_of(kernel)]
        for f in d16.FAMILIES:
            assert fams.count(f) >= 2, (kernel, f, fams.count(f))
    gemm = d16.cases_of("gemm_s")
    mnk = {(c.p["M"], c.p["N"], c.p["K"]) for c in gemm}
    assert set(dr.GEMM_TILE_EDGES) <= mnk and {(65, 68, K) for K in dr.GEMM_K_EDGES} <= mnk
    assert {c.p["mode"] for c in gemm} == set(dr.MODES) and {c.p["mode"] for c in gemm if c.p["K"] >= 2528} == set(dr.MODES)
    assert {c.p.get("tables", "") for c in gemm} == {"", "gather", "scatter", "both"}
    assert any(c.p.get("conv") == (7, 5) and (c.p["M"], c.p["N"], c.p["K"]) == (6, 36, 288) for c in gemm)
    assert any(c.p.get("lda") == c.p["K"] + 4 and c.p.get("ldc") == c.p["N"] + 4 for c in gemm)
    assert {c.p["K"] for c in gemm if c.fp32_only} == {40} and all(c.p["K"] % 32 == 0 for c in gemm if not c.fp32_only)
    assert any(c.poisoned and c.p["K"] >= 2560 for c in gemm) and sum(c.poisoned and c.p["K"] < 2560 for c in gemm) >= 4
    assert any((c.tables["c_rows"] == -1).sum() == 1 for c in gemm if "c_rows" in c.tables)
    for c in gemm:
        if c.poisoned:
            t = c.tables["a_rows"]
            assert (t == -1).sum() == 2 and not (t == 0).any() and np.isnan(c.inputs["A"][0]).all(), c.name
    for kernel in ("rowtile_s", "rowtile_h"):
        rt = d16.cases_of(kernel)
        assert {c.p["M"] for c in rt} == set(dr.ROWTILE_M)
        assert {(c.p["D"], c.p["N"]) for c in rt} == {(128, 128), (128, 384), (256, 256), (256, 768)}
        assert {(c.p["form"], c.p["D"]) for c in rt} == {("qkv", 128), ("qkv", 256), ("out", 128), ("out", 256)}
        assert any(c.p["ld"] for c in rt if c.p["form"] == "qkv") and any(c.p["ld"] for c in rt if c.p["form"] == "out")
    for kernel in ("ffn_s", "ffn_h"):
        ffn = d16.cases_of(kernel)
        assert {c.p["M"] for c in ffn} == set(d16.FFN_M) == {1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 79, 80, 81}
        assert {c.p["F"] for c in ffn} == set(d16.FFN_F)
        for M in d16.FFN_M:                                      # every M edge at both widths (49: the split form's tallest tile)
            assert {c.p["D"] for c in ffn if c.p["M"] == M} == {128, 256}, M
        assert {(c.p["ln"], c.p["table"]) for c in ffn} == {(a, b) for a in (True, False) for b in (True, False)}
    assert max(c.inputs[n].size for c in d16.all_cases() for n in c.inputs) <= max(c.inputs[n].size for c in dr.all_cases()
                                                                                    for n in c.inputs)
    for c in d16.all_cases():
        assert (c.family == "nobias" or c.family in ("small", "mixed", "edge")) == ("bias" not in c.inputs and "b1" not in c.inputs)
        for name, buf in c.inputs.items():                       # every input buffer is larger than what the launch names
            if buf.ndim == 2 and name in ("A", "XN"):
                assert np.isnan(buf).any(), (c.name, name)
        for name in c.ref:                                       # ... and so is every output buffer
            keep, named = ~c.named[name], c.named[name]
            assert keep.any() and (c.init[name][keep] == dr.SENTINEL).all(), (c.name, name)
            assert np.isfinite(c.ref[name][named]).all(), (c.name, name)
            assert (c.A[name][named] >= c.A32[name][named]).all() and (c.A32[name][named] >= 0).all(), (c.name, name)
        ops = [np.abs(v[np.isfinite(v)]) for n, v in c.inputs.items() if n in ("A", "XN", "W", "W1", "W2")]
        assert max(float(v.max()) for v in ops) < 65520.0, c.name                # no operand leaves fp16's range
        if c.family == "small" and not (c.kernel == "rowtile" and c.p["form"] == "qkv"):
            width = c.p["lda"] if c.p.get("conv") else c.p.get("K", c.p.get("D"))       # (the columns behind it are NaN)
            a = np.abs(c.inputs["A" if "A" in c.inputs else "XN"])[:, :width]
            tiny = np.isfinite(a).all(1) & (a <= 2.0 ** -14).all(1) & (a >= 2.0 ** -30).all(1)
            assert tiny.any(), c.name                            # rows whose hi halves are fp16 subnormals or zero
        if c.family == "edge" and not (c.kernel == "rowtile" and c.p["form"] == "qkv"):
            a = c.inputs["A" if "A" in c.inputs else "XN"]
            if c.p["M"] >= 4 and not c.p.get("tables"):
                assert all((np.abs(a) == v).any() for v in (2.0 ** -14, 2.0 ** -24, 2.0 ** -25, d16.FP16_BIG)), c.name
    assert np.float32(d16.FP16_BIG).astype(np.float16) == np.float16(65504.0)
    hi, lo = d16.split16(np.float32([2.0 ** -13 + 2.0 ** -25, 2.0 ** -25]))
    assert hi.tolist() == [2.0 ** -13, 0.0] and lo.tolist() == [2.0 ** -14, 2.0 ** -14]


@pytest.mark.parametrize("kernel", d16.KERNELS)
def test_transcriptions_are_finite_and_give_kappa_ref(kernel, capsys):
    """the transcription of every form on every case: finite (no poisoned element, no operand beyond fp16's range), and the
    kappa it needs - kappa_ref - per case and output"""
    bad, lines = [], []
    for case in d16.cases_of(kernel):
        for name, k in d16.kappa_ref(case).items():
            lines.append(f"  {case.name} {name}: kappa_ref {k:.3g}")
            if not math.isfinite(k):
                bad.append((case.name, name))
    with capsys.disabled():
        print(f"\nkappa_ref, {kernel}:")
        print("\n".join(lines))
    assert not bad, bad


def _fam(*names):
    return lambda c: c.family in names


LIVE = ("unit", "rows", "offset", "nobias")
SPLIT = ("gemm_s", "rowtile_s", "ffn_s")
# mistake -> the cases it is planted into: (kernel, condition on the case)
PLANTED = {
    "drop_cross_term": [(k, _fam(*LIVE)) for k in SPLIT],
    "cross_unscaled": [(k, _fam(*LIVE)) for k in SPLIT],
    "lo_unscaled_before_rounding": [(k, _fam("small")) for k in SPLIT],
    "hi_only": [(k, _fam(*LIVE)) for k in SPLIT],
    "flush_subnormal": [(k, _fam("small")) for k in d16.KERNELS],
    "fold_after_relu": [("gemm_s", lambda c: c.p["mode"] == "relu" and c.family in LIVE), ("ffn_s", _fam(*LIVE))],
    "clamped_row": [("gemm_s", lambda c: c.poisoned)],
    "hidden_fp32_in_h": [("ffn_h", _fam(*LIVE))],
}


@pytest.mark.parametrize("mistake", d16.MISTAKES)
def test_planted_mistakes_rise_above_the_tolerance(mistake, capsys):
    """each mistake, applied to the transcription, exceeds 4 x kappa_ref on some output of every case it is planted into
    (hidden_fp32_in_h: on the measure against the form itself - against the exact reference it is too good)"""
    assert set(PLANTED) == set(d16.MISTAKES)
    lines, bad = [], []
    for kernel, cond in PLANTED[mistake]:
        hit = [c for c in d16.cases_of(kernel) if not c.fp32_only and cond(c)]
        assert hit, (mistake, kernel)
        for case in hit[:3]:
            kref = d16.kappa_ref(case)
            km = case.kappas_of_rows(case.transcription(mistake))
            margin = max(km[n] / (4 * kref[n]) if kref[n] > 0 else (math.inf if km[n] > 0 else 0.0) for n in km)
            lines.append(f"  {case.name}: worst kappa / (4 x kappa_ref) {margin:.3g}")
            if not margin > 1.0:
                bad.append((case.name, margin))
            if mistake == "hidden_fp32_in_h":
                assert km["X"] <= kref["X"] and km["X@form"] > 4 * kref["X@form"], (case.name, km, kref)
    with capsys.disabled():
        print(f"\nplanted mistake {mistake}:")
        print("\n".join(lines))
    assert not bad, bad


def _unsplit(Ws):
    """the float64 weights a split_panel_weight copy stands for, back in [N][K] order"""
    from speechcatcher_amd.weights import unpack_panel_weight
    N, K = Ws.shape[0], Ws.shape[1] // 2
    v = Ws.reshape(-1, 2, 64, 8).double()
    v = v[:, 0] + v[:, 1] / 2048.0                               # [n][lane][8 k values]
    return unpack_panel_weight(torch.stack([v[..., :4], v[..., 4:]], dim=1).reshape(N, K)).numpy()


def test_split_panel_weight_reproduces_every_weight_to_rho():
    """hi + lo / 2^11 of the offline split against the weight itself: within rho(w) = max(2^-22 |w|, 2^-36), zero exactly - on
    the weights of every row-tile and feed-forward case of the split form (tiny columns and fp16 boundary values included)"""
    n = 0
    for case in d16.cases_of("rowtile_s") + d16.cases_of("ffn_s"):
        t = d16.tensors(case)
        for name in ("W", "W1", "W2"):
            if name in t:
                W = case.inputs[name].astype(np.float64)
                err = np.abs(_unsplit(t[name]) - W)
                assert (err <= d16._rho(W)).all(), (case.name, name, float((err / np.maximum(d16._rho(W), 1e-300)).max()))
                n += 1
    assert n >= 60
    W = np.float64(np.float32(1e-6))                             # the floor is real: 2^-23 |w| does not hold below 2^-14
    hi, lo = d16.split16(np.float32([1e-6]))
    assert abs(float(hi[0]) + float(lo[0]) / 2048.0 - W) > 2.0 ** -23 * W


def test_the_small_family_reaches_the_floor(capsys):
    """at the worst element of a `small` case's direct output the 2^-36 term is at least half of E(y): the family measures the
    floor, not the bias or the residual"""
    lines, reach = [], {k: 0 for k in SPLIT}
    for kernel in SPLIT:
        for case in d16.cases_of(kernel):
            if case.family != "small" or case.fp32_only:
                continue
            share, k = case.floor_share(case.transcription())
            lines.append(f"  {case.name}: floor / E at the worst element {share:.3f}, kappa there {k:.3g}")
            reach[kernel] += share >= 0.5
    with capsys.disabled():
        print("\nthe 2^-36 floor in the small family:")
        print("\n".join(lines))
    assert all(v >= 1 for v in reach.values()), reach

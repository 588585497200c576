"""The float64 references of tests/dense_ref.py against the fp32 torch spec (oracle/kernel_spec.py) on the CPU, every case of the
list.  A wrong reference shows as a kappa of 1e3 and more; a right one leaves the spec within 4 x the kappa that the fp32
transcription of the kernels' documented summation order needs.  The same run measures kappa_ref for the GPU module
(tests/test_gpu_dense.py runs it again on the machine the kernels run on).  Also here: the case list covers every edge it was
written for, the poison is where the kernels could read it but the spec does not, and mistakes planted into the transcription
show far above the tolerance the GPU test will apply."""
import math

import numpy as np
import pytest

import dense_ref as dr

# a planted mistake must exceed the GPU test's limit (4 x kappa_ref) by this factor: as far above the limit as the limit is
# above what a correct fp32 evaluation needs.  Most mistakes are of the order of an operand (margins of 1e4 and more) or of
# 2^-11 of it (~100); the one-pass variance at the offset family's 100 + N(0,1) is the faintest - its error is a few roundings
# of E[x^2] ~ 1e4 against a variance of ~1, i.e. ~1e-3 of the output, some 5 - 15 times the limit
MISTAKE_MARGIN = 4.0


@pytest.mark.parametrize("kernel", dr.KERNELS)
def test_references_against_the_spec(kernel, capsys):
    """spec kappa <= 4 x transcription kappa on every output of every case; the spec is finite on every poisoned case"""
    rows, bad = [], []
    for case in dr.cases_of(kernel):
        for name, (ks, kt, kr) in dr.kappa_ref(case).items():
            rows.append((case.name, name, ks, kt))
            if not math.isfinite(ks):
                bad.append((case.name, name, "the spec reads a poisoned element (or the reference is not finite)"))
            elif not (math.isfinite(kt) and ks <= 4 * kt):
                bad.append((case.name, name, f"spec kappa {ks:.3g} > 4 x transcription kappa {kt:.3g}"))
            if kt == 0 and ks == 0 and case.family not in ("dead", "constant"):
                bad.append((case.name, name, "nothing is measured: both evaluations are exact"))
    with capsys.disabled():
        kr = [max(ks, kt) for _, _, ks, kt in rows]
        print(f"\nkappa_ref, {kernel}: {len(rows)} outputs of {len(dr.cases_of(kernel))} launches, {min(kr):.3g} .. {max(kr):.3g}")
        for cn, n, ks, kt in rows:
            print(f"  {cn} {n}: spec {ks:.3g} transcription {kt:.3g}")
    assert not bad, bad


def _shapes(kernel, *keys):
    return {tuple(c.p.get(k) for k in keys) for c in dr.cases_of(kernel)}


def test_cases_cover_the_edges_families_and_poison():
    gemm = dr.cases_of("gemm")
    mnk = _shapes("gemm", "M", "N", "K")
    assert set(dr.GEMM_TILE_EDGES) <= mnk and {(65, 68, K) for K in dr.GEMM_K_EDGES} <= mnk
    assert 35 <= len(gemm) <= 45 and 55 <= len(dr.all_cases()) - len(gemm) <= 80
    for shape in set(dr.GEMM_TILE_EDGES) | {(65, 68, K) for K in dr.GEMM_K_EDGES}:      # every shape meets two families
        assert len({c.family for c in gemm if (c.p["M"], c.p["N"], c.p["K"]) == shape}) >= 2, shape
    assert {c.p["mode"] for c in gemm if c.p["K"] >= 2528} == set(dr.MODES)
    assert any(c.p["K"] % 32 for c in gemm) and any(c.p.get("lda", 0) == c.p["K"] + 2 for c in gemm)          # scalar fallbacks
    assert any(c.p.get("lda") == c.p["K"] + 4 and c.p.get("ldc") == c.p["N"] + 4 for c in gemm)
    assert any(c.p.get("conv") == (7, 5) and c.p["lda"] == 32 for c in gemm)
    gathers = [c.tables["a_rows"] for c in gemm if "a_rows" in c.tables and not c.p.get("conv")]
    assert any((t == -1).sum() == 2 and len(set(t.tolist())) < len(t) - 1 for t in gathers)          # two -1 and duplicates
    assert any((c.tables["c_rows"] == -1).sum() == 1 for c in gemm if "c_rows" in c.tables)
    assert any(c.poisoned and c.p["K"] >= 2560 for c in gemm) and any(c.poisoned and c.p["K"] < 2560 for c in gemm)
    ln = dr.cases_of("gemm_ln")
    assert {c.p["N"] for c in ln} == {64, 256, 1024, 1028} and {c.p["K"] for c in ln} == {40, 64, 2560}
    assert {c.p["M"] for c in ln} == {1, 3, 4, 5, 33, 65} and {c.p["N"] for c in ln if c.refused} == {1028}
    assert {c.p["at_crows"] for c in ln if c.p["tables"]} == {True, False}
    rt = dr.cases_of("rowtile")
    assert {c.p["M"] for c in rt} == set(dr.ROWTILE_M)
    assert _shapes("rowtile", "D", "N") == {(128, 128), (128, 384), (256, 256), (256, 768)}
    assert {(c.p["form"], c.p["D"]) for c in rt} == {("qkv", 128), ("qkv", 256), ("out", 128), ("out", 256)}
    assert any(c.p["ld"] for c in rt if c.p["form"] == "qkv") and any(c.p["ld"] for c in rt if c.p["form"] == "out")
    ffn = dr.cases_of("ffn")
    assert {c.p["M"] for c in ffn} == set(dr.FFN_M) and {c.p["F"] for c in ffn} == set(dr.FFN_F)
    assert {c.p["D"] for c in ffn} == {128, 256}
    assert {(c.p["ln"], c.p["table"]) for c in ffn} == {(a, b) for a in (True, False) for b in (True, False)}
    pn = dr.cases_of("panel")
    assert {c.p["M"] for c in pn} == set(dr.PANEL_M) and {c.p["D"] for c in pn} == {64, 128, 256}
    assert {(c.p["second"], c.p["table"]) for c in pn} == {(a, b) for a in (True, False) for b in (True, False)}
    assert _shapes("ffn_proj", "M", "D", "F", "N") == set(dr.FFN_PROJ_SHAPES)
    for kernel in dr.KERNELS:
        assert {c.family for c in dr.cases_of(kernel)} == set(dr.FAMILIES), kernel
    n_poisoned = 0
    for c in dr.all_cases():
        A = c.inputs.get("A")
        if c.poisoned:
            t = c.tables["a_rows"]
            assert (t == -1).any() and not (t == 0).any() and np.isnan(A[0]).all(), c.name
            n_poisoned += 1
        for name, buf in c.inputs.items():                     # every input buffer is larger than what the launch names
            if buf.ndim == 2 and name in ("A", "XN", "Xin"):
                assert np.isnan(buf).any(), (c.name, name)
        for name in c.ref:                                     # ... and so is every output buffer
            assert (~c.named[name]).any() and (c.init[name][~c.named[name]] == dr.SENTINEL).all(), (c.name, name)
            assert np.isfinite(c.ref[name][c.named[name]]).all() and (c.A[name][c.named[name]] >= 0).all(), (c.name, name)
    assert n_poisoned >= 8


LIVE = ("unit", "rows", "offset", "nobias")     # families without zero rows (a zero row hides what is done to its products)
# mistake -> the cases it is planted into: (kernel, condition on the case)
def _fam(*names):
    return lambda c: c.family in names


PLANTED = {
    "drop_k_tile": [("gemm", lambda c: c.p["K"] == 64 and c.p["N"] == 68), ("gemm", lambda c: c.p["K"] == 2560),
                    ("rowtile", _fam(*LIVE)), ("panel", _fam(*LIVE))],
    "clamped_row": [("gemm", lambda c: c.poisoned), ("gemm_ln", lambda c: c.poisoned)],
    "bias_tile": [("gemm", lambda c: c.p["N"] == 132 and c.family != "nobias"),
                  ("gemm_ln", lambda c: c.p["N"] == 1028 and c.family != "nobias")],
    "relu_first": [("gemm", lambda c: c.p["mode"] == "relu" and c.family == "rows"), ("ffn", _fam("unit"))],
    # (M > 1: the error of a one-pass variance is ONE rounding of E[x^2] ~ 1e4 per row - anything from half an ulp down to
    # nothing; a launch of a single row is one draw of it)
    "one_pass_var": [("gemm_ln", lambda c: c.family == "offset" and c.p["M"] > 1), ("rowtile", _fam("offset")),
                     ("ffn", lambda c: c.family == "offset" and c.p["ln"]), ("panel", _fam("offset"))],
    "fp16_operand": [("gemm", lambda c: c.p["K"] == 64 and c.family == "unit"), ("gemm", lambda c: c.p["K"] == 4864),
                     ("rowtile", _fam("unit")), ("ffn", _fam("unit")), ("panel", _fam("unit"))],
    "drop_chunk": [("ffn", lambda c: c.p["F"] == 384), ("ffn", lambda c: c.p["F"] == 2048 and c.family == "nobias"),
                   ("ffn_proj", lambda c: c.p["F"] == 2048)],
    "residual_twice": [("gemm", lambda c: c.p["mode"] == "residual"), ("rowtile", lambda c: c.p["form"] == "out"), ("ffn", None),
                       ("panel", None)],
}


@pytest.mark.parametrize("mistake", dr.MISTAKES)
def test_planted_mistakes_show_far_above_the_tolerance(mistake, capsys):
    """each mistake, applied to the transcription, exceeds 4 x kappa_ref on some output of every case it is planted into"""
    assert set(PLANTED) == set(dr.MISTAKES)
    lines, bad = [], []
    for kernel, cond in PLANTED[mistake]:
        hit = [c for c in dr.cases_of(kernel) if cond is None or cond(c)]
        assert hit, (mistake, kernel)
        for case in hit[:3]:
            kref = dr.kappa_ref(case)
            km = case.kappas_of_rows(case.transcription(mistake))
            margin = max(km[n] / (4 * kref[n][2]) if kref[n][2] > 0 else (math.inf if km[n] > 0 else 0.0) for n in km)
            lines.append(f"  {case.name}: margin {margin:.3g}")
            if not margin >= MISTAKE_MARGIN:
                bad.append((case.name, margin))
    with capsys.disabled():
        print(f"\nplanted mistake {mistake}: worst kappa / (4 x kappa_ref)")
        print("\n".join(lines))
    assert not bad, bad

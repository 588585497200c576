"""The float64 references of tests/dec_dense_ref.py against the fp32 torch spec (oracle/kernel_spec.py) on the CPU, for every
fp32 case of the decoder's dense launches - sc_dec_embed, sc_dec_layer_ffn, sc_dec_layer_ffn_xn, sc_dec_output_logits - with the
row tables and row counts the GPU test uses.  A wrong reference shows as a kappa of 1e4 and more; a right one leaves the spec a
kappa of at most KAPPA_MAX.  The same run measures kappa_ref (the spec's kappa on the fp32 cases, the transcription's on the
fp16 and split16 ones), prints the table and leaves it as dec_dense_kappa_ref.json beside the GPU numbers (test_gpu_ops.write_report).  Also
here: every planted mistake in the transcriptions is rejected - it exceeds 4 x kappa_ref (or is not finite: a poisoned element
was read) on at least one case - and the case lists cover what they are meant to."""
import math

import numpy as np
import pytest

import dec_dense_ref as dd

# A charges every term ONE unit 2^-24; an fp32 evaluation rounds a term about a dozen times on its way through the partial
# sums, the residual, the LayerNorm (mean, deviation, variance, scale, shift) and a product sum: 16 (test_dec_attn_ref_spec.py)
KAPPA_MAX = 16.0
FP32_FFN = [c for c in dd.FFN_CONFIGS if dd.fp32_case(c[3], c[4])]
FP32_LOGITS = [c for c in dd.LOGITS_CONFIGS if not c[2]]
LAUNCHES = ((None, "descending"), (None, "shuffled"), (33, "shuffled"), (17, "descending"))


def _held(k, where):
    for name, v in k.items():
        assert math.isfinite(v) and v <= KAPPA_MAX, (where, name, v)


@pytest.mark.parametrize("geom,W,hpw,wform,act_half", FP32_FFN)
def test_feed_forward_references_against_the_spec(geom, W, hpw, wform, act_half, capsys):
    """dec_layer_ffn (residual + head partials + bo2, norm3, feed-forward as ONE partial sum by row id) and dec_layer_ffn_xn as
    SpecBackend states them, over the whole table and over a part of it: rows the table does not list keep the sentinel"""
    rep = {}
    for fam in dd.FAMILIES:
        case = dd.ffn_case(geom, W, fam, hpw, wform, act_half)
        for M, perm in LAUNCHES:
            k, bad = dd.spec_ffn(case, M, perm)
            assert not bad, (case.name, M, perm, bad)
            _held(k, (case.name, M, perm))
            assert k["xout"] > 0 and k["ffn"] > 0 and k["ffn_xn"] > 0      # (a case whose every sum is exact measures nothing)
        rep[fam] = dd.ffn_kappa_ref(geom, W, fam, hpw, wform, act_half)
    with capsys.disabled():
        print(f"\nspec kappa, dec_layer_ffn {geom} beam {W} hpw {hpw}: " +
              "; ".join(f"{f} " + " ".join(f"{n} {v:.3g}" for n, v in k.items()) for f, k in rep.items()))


@pytest.mark.parametrize("geom,W,act_half", FP32_LOGITS)
def test_output_layer_references_against_the_spec(geom, W, act_half, capsys):
    rep = {}
    for f, fam in enumerate(dd.FAMILIES):
        for npart in dd.nparts_of(geom):
            case = dd.logits_case(geom, W, fam, npart, act_half)
            for M, perm in LAUNCHES[(f + npart) % 2::2]:
                k, bad = dd.spec_logits(case, M, perm)
                assert not bad, (case.name, M, perm, bad)
                _held(k, (case.name, M, perm))
                assert k["xout"] > 0 and k["logits"] > 0
            rep[(fam, npart)] = dd.logits_kappa_ref(geom, W, fam, npart, act_half)
    with capsys.disabled():
        print(f"\nspec kappa, dec_output_logits {geom} beam {W}: " +
              "; ".join(f"{f} npart {p} " + " ".join(f"{n} {v:.3g}" for n, v in k.items()) for (f, p), k in rep.items()))


@pytest.mark.parametrize("geom,W", [("D8", 10), ("D4", 10), ("D8", 5), ("D128", 10)])
def test_embed_reference_against_the_spec(geom, W):
    """the spec's rows are the reference's BITS (d = 256: the product with sqrt(d) = 16 is exact; d = 128: within KAPPA_MAX),
    rows >= nh and the inactive stream keep the sentinel; the positional row L instead of L - 1 is another row"""
    from oracle.kernel_spec import SpecBackend
    case = dd.EmbedCase(geom, W)
    sb = dd.spec_batch(geom, W, case.S)
    dd.apply_embed(sb, case)
    SpecBackend().dec_embed(sb)
    kref = dd.embed_kappa_ref(geom, W)
    assert not case.problems(sb.dx.numpy(), kref) and (case.exact or 0 < kref <= KAPPA_MAX)
    assert {case.L[s] - 1 for s in case.L} == {0, 1, dd.LCAP - 2}
    assert any(case.nh[s] < W for s in case.nh) and dd.INACTIVE not in case.nh
    toks = np.concatenate(list(case.tok.values()))
    assert 0 in toks and case.V - 1 in toks and len(set(toks.tolist())) < len(toks)
    # planted mistake: pe[L] instead of pe[L - 1]
    wrong = np.full((case.n, case.d), dd.SENTINEL, np.float32)
    for s, r in case.ref_wrong_row.items():
        wrong[s * W:s * W + case.nh[s]] = r
    assert case.problems(wrong, kref)


def test_kappa_ref_table(capsys):
    """kappa_ref of every case of the GPU test, per output; fp16 / split16 cases: the transcription's"""
    from test_gpu_ops import write_report
    rep = {"ffn": {}, "logits": {}}
    for geom, W, hpw, wform, act_half in dd.FFN_CONFIGS:
        for fam in dd.FAMILIES:
            k = dd.ffn_kappa_ref(geom, W, fam, hpw, wform, act_half)
            assert all(math.isfinite(v) and (0 < v or n == "ffn@form") and v <= KAPPA_MAX for n, v in k.items()), (geom, W, hpw, wform, act_half, fam, k)
            rep["ffn"][dd.ffn_case(geom, W, fam, hpw, wform, act_half).name] = k
    for geom, W, act_half in dd.LOGITS_CONFIGS:
        for fam in dd.FAMILIES:
            for npart in dd.nparts_of(geom):
                k = dd.logits_kappa_ref(geom, W, fam, npart, act_half)
                assert all(math.isfinite(v) and 0 < v <= KAPPA_MAX for v in k.values()), (geom, W, act_half, fam, npart, k)
                rep["logits"][dd.logits_case(geom, W, fam, npart, act_half).name] = k
    write_report("dec_dense_kappa_ref", rep)
    with capsys.disabled():
        print("\nkappa_ref (largest over the families and partial counts):")
        for kind in rep:
            groups = {}
            for name, k in rep[kind].items():
                key = name.rsplit(",", 1)[0] if kind == "ffn" else ",".join(p for p in name.split(",")[:-1] if not p.startswith("npart"))
                g = groups.setdefault(key, {})
                for n, v in k.items():
                    g[n] = max(v, g.get(n, 0.0))
            for key, g in groups.items():
                print(f"  {key:50s} " + " ".join(f"{n} {v:.3g}" for n, v in g.items()))


def _rejected(k, kref):
    """a planted mistake shows: some output is not finite or beyond 4 x kappa_ref"""
    return any(not math.isfinite(v) or v > 4 * kref[n] for n, v in k.items())


@pytest.mark.parametrize("mistake", dd.FFN_MISTAKES)
def test_planted_feed_forward_mistakes_are_rejected(mistake):
    """bo2 added twice; LayerNorm before the residual; the head partials read with the one-head layout (H per row, groups of
    four) where the four-head launch wrote H / 4 per row; the slots of a row read at twice their index; fp32 partials kept in fp16 mode (closer to exact: only "ffn@form" sees it)"""
    geom, W, hpw, wform, act_half = {"head_layout": ("D8", 10, 4, "float32", 3), "parts_fp32_in_half": ("D8", 10, 1, "float32", 2)
                                     }.get(mistake, ("D8", 10, 1, "float32", 1))
    hits = []
    for fam in dd.FAMILIES:
        case = dd.ffn_case(geom, W, fam, hpw, wform, act_half)
        kref = dd.ffn_kappa_ref(geom, W, fam, hpw, wform, act_half)
        for n_part in dd.n_part_rule(case.F, case.F // 128, case.part_half):
            good = case.kappas_of(*case.transcription(33, "shuffled", n_part))
            assert not _rejected(good, kref), (case.name, n_part, good, kref)    # (the transcription itself passes the same check)
            k = case.kappas_of(*case.transcription(33, "shuffled", n_part, mistake))
            hits.append(_rejected(k, kref))
            if mistake == "parts_fp32_in_half":                  # the measure against the reference cannot see it
                assert k["ffn"] <= 4 * kref["ffn"], (case.name, k, kref)
    assert any(hits), mistake
    if mistake != "parts_fp32_in_half":
        assert all(hits), (mistake, hits)


@pytest.mark.parametrize("mistake", dd.LOGITS_MISTAKES)
def test_planted_output_layer_mistakes_are_rejected(mistake):
    """the ninth partial dropped; b2 added twice; LayerNorm before the residual; partial sums indexed by position instead of
    row id; fp16 partial sums read as fp32"""
    act_half = 2 if mistake == "half_as_fp32" else 0
    hits = []
    for fam in dd.FAMILIES:
        case = dd.logits_case("D8", 10, fam, 9, act_half)
        kref = dd.logits_kappa_ref("D8", 10, fam, 9, act_half)
        rows, x, xn, lg = case.transcription(33, "shuffled")
        assert not _rejected(case.kappas_of(rows, x, xn, lg), kref), case.name
        rows, x, xn, lg = case.transcription(33, "shuffled", mistake)
        hits.append(_rejected(case.kappas_of(rows, x, xn, lg), kref))
    assert any(hits), mistake
    if mistake != "drop_last_partial":       # (zero rows carry partials of zero: a dropped one is no mistake there)
        assert all(hits), (mistake, hits)


def test_cases_cover_the_rows_tables_and_forms():
    assert dd.M_EDGES == (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 79, 80, 81, 90)
    for W in (10, 5):
        S = 90 // W
        maps = dd.rowmaps(S, W)
        for name, m in maps.items():
            assert sorted(m.tolist()) == list(range(90)) and (m != np.arange(90)).any(), name
        streams = (maps["descending"][::W] // W).tolist()
        assert streams[-2:] == [dd.GAP, dd.INACTIVE] and streams[:-2] == sorted(streams[:-2], reverse=True)
    # the documented group counts: 16 or 8 at F = 2048, pairs only beyond, an odd chunk count never pairs, never more than max_part
    assert dd.n_part_rule(2048, 16) == [16, 8] and dd.n_part_rule(2048, 8) == [8] and dd.n_part_rule(2304, 18) == [9]
    assert dd.n_part_rule(640, 5) == [5] and dd.n_part_rule(2048, 7) == []
    # fp16 partial sums: a function of F alone
    assert dd.n_part_rule(2048, 16, True) == [8] == dd.n_part_rule(2048, 8, True) and dd.n_part_rule(640, 5, True) == [5]
    assert {c[0] for c in dd.FFN_CONFIGS} == set(dd.GEOMS) and {c[4] for c in dd.FFN_CONFIGS} == {0, 1, 2, 3}
    assert {c[3] for c in dd.FFN_CONFIGS} == {"float32", "float16", "split16"} and {c[2] for c in dd.FFN_CONFIGS} == {1, 4}
    assert {c[1] for c in dd.FFN_CONFIGS} == {10, 5}
    assert set(dd.nparts_of("D8")) == {1, 2, 8, 9, 16} and {dd.GEOMS[c[0]]["vocab_size"] for c in dd.LOGITS_CONFIGS} == {1024, 1280}
    for geom, cfg in dd.GEOMS.items():       # every geometry is one the fused decoder layers accept (D128: accepted, not refused)
        from speechcatcher_amd.weights import dec_layer_fused_supported
        assert dec_layer_fused_supported(dd.config_of(geom), 10), geom
    case = dd.ffn_case("D8", 10, "zero", 1, "float32", 0)
    assert case.zero_rows.sum() == 30 and (case.ref["xout"][case.zero_rows] == 0).all()
    nh = dd.short_nh(10)
    assert (case.ph[dd.SHORT * 10 + nh:(dd.SHORT + 1) * 10] == 0).all()
    case = dd.ffn_case("D8", 10, "cancel", 1, "float32", 0)
    assert (np.abs(case.ph.sum(1)) <= 0.1 * np.abs(case.ph).sum(1)).all()

"""The float64 references of tests/dec_attn_ref.py against the fp32 torch spec (oracle/kernel_spec.py) on the CPU: every
case family of every geometry and launch kind.  A wrong reference shows as a kappa of 1e4 and more; a right one leaves the
spec a kappa of at most KAPPA_MAX, the rounding of fp32 sums.  The same run is what measures kappa_ref for the GPU module
(tests/test_gpu_decoder_attention.py runs it again on the machine the kernels run on).  Also here: the tables of every case
are valid (the GPU test must never launch an invalid one)."""
import math

import numpy as np
import pytest

import dec_attn_ref as dr

# (geometry, beam): head dims 16 / 32 / 64; the 5- / 10- / 16-row instantiations.  Head dim 64 at beam 16 is not a shape of the
# product: HipBackend.check_supported refuses it when the batch is made (64: beam <= 10), so no batch can be built for it
ATTN_GEOMS = [("TINY", 10), ("TINY", 5), ("TINY", 16), ("XL", 10), ("XL", 5), ("XL", 16), ("L_LIKE", 10), ("L_LIKE", 5)]
FUSED_GEOMS = [("XL", 10), ("XL", 5), ("XL", 16), ("L_LIKE", 10)]
# A charges every term ONE unit 2^-24; an fp32 evaluation rounds a term at most about a dozen times on its way (product, sum,
# scale, maximum subtracted, exponential - 2 ulp = 4 units -, normalisation, P.V product and sum, output projection): 16.  A
# reference that is off by 1e-5 of a value already needs more.
KAPPA_MAX = 16.0
# The dominant-key contexts: A = (1 + M) sum p|v| with M = max sum|q k| / sqrt(dk) >= 45 on every peaked row (the margin is
# part of some key's score).  Of the 16 roundings only those of the score terms are multiplied by M - product and accumulation,
# 2 units per term; the exponential's error is relative to p, not to the score - so kappa <= (16 + 2 M) / (1 + M) <= 2.5.
KAPPA_MAX_DOMINANT_CTX = 2.5


def _check(case, which=None):
    bad = dr.validity_problems(case)
    assert not bad, bad
    k = dr.spec_kappas(case, which)
    for name, v in k.items():
        top = KAPPA_MAX_DOMINANT_CTX if case.family == "dominant" and name.endswith("_ctx") else KAPPA_MAX
        assert math.isfinite(v) and v <= top, (case.geom, case.W, case.kind, case.family, name, v)
    return k


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("geom,W", ATTN_GEOMS)
def test_context_reference_against_the_spec(geom, W, half, capsys):
    """dec_self_attn / dec_cross_attn: the float64 context of every (stream, hypothesis, head), fp32 and fp16-rounded caches"""
    rep = {}
    for fam in dr.FAMILIES:
        case = dr.Case(geom, W, "attn", fam, half=half)
        rep[fam] = {**_check(case, "self"), **_check(case, "cross")}
        assert rep[fam]["self_ctx"] > 0 and rep[fam]["cross_ctx"] > 0      # (a family whose every softmax is exact measures nothing)
    with capsys.disabled():
        print(f"\nspec kappa, attention {geom} beam {W} {'fp16' if half else 'fp32'} K|V: " +
              "; ".join(f"{f} self {k['self_ctx']:.3g} cross {k['cross_ctx']:.3g}" for f, k in rep.items()))


@pytest.mark.parametrize("kind", ["self", "cross"])
@pytest.mark.parametrize("geom,W", FUSED_GEOMS)
def test_fused_layer_references_against_the_spec(geom, W, kind, capsys):
    """dec_layer_self / dec_layer_cross as SpecBackend states them: residual + partial sums + bias, LayerNorm, projection, K|V
    append, attention, per-head output projection - layer 0 and a later layer with 1 and 11 partial sums, one and (XL, beams
    <= 10) four heads per partial product"""
    rep = {}
    gi = FUSED_GEOMS.index((geom, W))
    for hpw in (1, 4) if geom == "XL" and W <= 10 else (1,):
        for f, fam in enumerate(dr.FAMILIES):
            li, npart = dr.layer_variant(f + gi)
            case = dr.Case(geom, W, kind, fam, half=bool((f + hpw) % 2), li=li if kind == "self" else 1, npart=npart, hpw=hpw)
            rep[(hpw, fam)] = _check(case)
    with capsys.disabled():
        print(f"\nspec kappa, dec_layer_{kind} {geom} beam {W}: " +
              "; ".join(f"hpw{h} {f} " + " ".join(f"{n} {v:.3g}" for n, v in k.items()) for (h, f), k in rep.items()))


def test_stream_resident_reference_against_the_spec(capsys):
    """dec_layer_stream (XL, beam 10): both attention blocks of a layer, xout and xn_out"""
    rep = {}
    for f, fam in enumerate(dr.FAMILIES):
        li, npart = dr.layer_variant(f)
        rep[fam] = _check(dr.Case("XL", 10, "stream", fam, li=li, npart=npart))
    with capsys.disabled():
        print("\nspec kappa, dec_layer_stream XL beam 10: " +
              "; ".join(f"{f} " + " ".join(f"{n} {v:.3g}" for n, v in k.items()) for f, k in rep.items()))


# fp16 decoder mode: (geometry, beam, act_half) - all three settings at XL beam 10, the whole mode at head dim 64 and at beam 5
HALF_GEOMS = [("XL", 10, 1), ("XL", 10, 2), ("XL", 10, 3), ("L_LIKE", 10, 3), ("XL", 5, 3)]


def half_cases(geom, W, kind, dec_half):
    """the reduced case set of the fp16 decoder mode: families flat and dominant, one and (XL, beams <= 10) four heads per
    workgroup; the layer / partial-sum variant rotates"""
    for f, fam in enumerate(dr.HALF_FAMILIES):
        for hpw in (1, 4) if geom == "XL" and W <= 10 else (1,):
            li, npart = dr.layer_variant(f + hpw + dec_half)
            yield dr.Case(geom, W, kind, fam, half=True, li=li if kind == "self" else 1, npart=npart, hpw=hpw, dec_half=dec_half)


@pytest.mark.parametrize("kind", ["self", "cross"])
@pytest.mark.parametrize("geom,W,dec_half", HALF_GEOMS)
def test_fp16_decoder_mode_references_against_their_transcription(geom, W, dec_half, kind, capsys):
    """SpecBackend has no fp16 mode: kappa_ref of these cases is the kappa the fp32 transcription of the documented arithmetic
    needs (dec_attn_ref.transcription).  The transcription itself is held to the spec where both exist: on the same cases with
    the mode off it needs what the spec needs, within the cap.  Then the planted mistake: fp16 partial products read as fp32"""
    rep = {}
    for case in half_cases(geom, W, kind, dec_half):
        assert not dr.validity_problems(case)
        k = dr.transcription_kappas(case)
        for name, v in k.items():
            assert math.isfinite(v) and 0 < v <= KAPPA_MAX, (case.family, case.hpw, name, v)
        rep[(case.family, case.hpw)] = k
        off = dr.Case(geom, W, kind, case.family, half=True, li=case.li, npart=case.npart, hpw=case.hpw)
        k0, ks = dr.transcription_kappas(off), dr.spec_kappas(off)
        for name, v in k0.items():
            assert math.isfinite(v) and v <= KAPPA_MAX and ks[name] <= KAPPA_MAX, (case.family, case.hpw, name, v, ks[name])
    with capsys.disabled():
        print(f"\ntranscription kappa, dec_layer_{kind} {geom} beam {W} act_half {dec_half}: " +
              "; ".join(f"{f} hpw{h} " + " ".join(f"{n} {v:.3g}" for n, v in k.items()) for (f, h), k in rep.items()))


def test_fp16_decoder_mode_cases_cover_the_reduced_set():
    Lc, T = set(), set()
    for fam in dr.HALF_FAMILIES:
        plan = dr.half_stream_plan(fam, 10)
        assert not plan[dr.INACTIVE].active and {st.nh for st in plan if st.active} >= {1, 3, 10}
        for st in plan:
            if st.active:
                Lc.add(st.L - 1), T.add(st.T)
                assert dr.PLACE.get(st.variant, 0) < min(st.L - 1, st.T)
    assert Lc == set(dr.HALF_LC) == {16, 17, 128, 129} and T == set(dr.HALF_T) == {16, 17, 129}
    # the mode changes what is written, not only what is allowed: fp16 weights, fp16 partial inputs
    case = next(half_cases("XL", 10, "cross", 3))
    assert (case.inputs["ph1"][np.isfinite(case.inputs["ph1"])] == dr.f16(case.inputs["ph1"][np.isfinite(case.inputs["ph1"])])).all()
    wq = case.w["dec"][1]["wq"]
    assert (wq == dr.f16(wq)).all() and not (dr._weights(dr.spec_batch("XL", 10))["dec"][1]["wq"] == wq).all()
    # a planted mistake: the head partials of a four-head launch rounded per head instead of once per workgroup is a
    # reordering of roundings that kappa cannot see; one that drops the rounding of the context is closer to exact; what kappa
    # does see is a partial product read in the wrong precision
    t = dr.transcription(case)
    s = next(iter(t["ph2"]))
    wrong = t["ph2"][s].astype(np.float16).view(np.uint16).astype(np.float32)          # the fp16 bits taken for numbers
    assert dr.kappa(wrong, case.ref["ph2"][s], case.A["ph2"][s]) > 4 * dr.transcription_kappas(case)["ph2"]


def test_cases_cover_the_lengths_forms_and_patterns():
    """every length of the issue's lists, an inactive stream, nh = 1 and 1 < nh < W in every launch, the three ancestries, a fork
    on the 512 edge / a tile edge / inside a tile, and the dominant key at every place"""
    Lc, T, kinds, forks = set(), set(), set(), set()
    for fam in dr.FAMILIES:
        plan = dr.stream_plan(fam, 10)
        assert [st.active for st in plan].count(0) == 1 and not plan[dr.INACTIVE].active
        nhs = {st.nh for st in plan if st.active}
        assert 1 in nhs and any(1 < n < 10 for n in nhs) and 10 in nhs
        for st in plan:
            if st.active:
                Lc.add(st.L - 1), T.add(st.T), kinds.add(st.anc_kind)
                if st.anc_kind == "fork":
                    forks.add("512" if st.fork == 512 else "edge" if st.fork % 16 == 0 else "inside")
    assert Lc == set(dr.SELF_LC) and T == set(dr.CROSS_T)
    assert kinds == {"shared", "fork", "divergent"} and forks == {"512", "edge", "inside"}
    assert [v for v, _, _ in dr.DOMINANT] == ["first", "last", "wave1", "wave2", "wave3", "batch2", "own"]
    for v, lc, t in dr.DOMINANT:       # the place exists at the lengths it is used with
        assert dr.PLACE.get(v, 0) < min(lc, t)
    # the patterns are what they are called: a dominant key leads by >= 40 in the reference's own scores
    case = dr.Case("XL", 10, "attn", "dominant")
    for st in case.streams:
        if st.active and st.variant != "own":
            d, dk = case.d, case.dk
            q = case.inputs["dq"][st.s * 10:st.s * 10 + st.nh].astype(np.float64).reshape(st.nh, case.H, dk)
            k = case.ckv[st.s, case.li, :st.T, :d].astype(np.float64).reshape(st.T, case.H, dk)
            sc = np.einsum("hgd,tgd->hgt", q, k) / math.sqrt(dk)
            peaked = sc[:st.nh - 1] if st.nh > 2 else sc
            top2 = np.sort(peaked, -1)[..., -2:]
            assert (top2[..., 1] - top2[..., 0] >= 40).all(), (st.s, float((top2[..., 1] - top2[..., 0]).min()))

"""The decoder attention kernels, each launch on its own against the float64 references of tests/dec_attn_ref.py:
sc_dec_self_attn / sc_dec_cross_attn (head dims 16 / 32 / 64, the 5- / 10- / 16-row instantiations - head dim 64 at beams 5 and
10: HipBackend.check_supported refuses a batch of head dim 64 with a wider beam -, both batch depths, fp32 and fp16 K|V),
sc_dec_layer_self / sc_dec_layer_cross (one head per workgroup at both depths, four heads per workgroup, layer 0 and a later
layer with 1 and 11 partial sums, fp32 and fp16 K|V) and sc_dec_layer_stream.  Where the lock-step runs of test_gpu_ops.py see
flat softmaxes at whatever lengths a fixture walks through, the cases here put L and T on the tile, batch and row-list edges,
control the beam's ancestry and impose peaked, ascending, descending, shifted and per-hypothesis score patterns through the
cache contents.  Per launch:
  * every output is finite although everything the operation must not read is NaN;
  * every output lies within the error model at 4 x kappa_ref, kappa_ref = the kappa the fp32 torch spec needs on the same case,
    measured here on the CPU (4: the kernels' k-ordered MFMA chains and per-batch rescales against torch's blocked sums);
  * the K|V rows of the new tokens are appended (fp16-rounded for the half cache), every other element of the pool keeps its bits;
  * rows of the inactive stream keep the sentinel, rows >= nh are what the spec says, exactly H / HPW partial slots are written;
  * SC_ATTN_DEEP = 0 and 1 give the same bits.
tests/test_dec_attn_ref_spec.py holds the references themselves to the spec on the CPU."""
import numpy as np
import pytest
import torch

import dec_attn_ref as dr
from test_dec_attn_ref_spec import ATTN_GEOMS, FUSED_GEOMS, HALF_GEOMS, half_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend(DEV)


def _gpu_batch(hip, geom, W, half, dec_half=False):
    from test_engine_spec import make_batch
    return make_batch(dr.cfg_name(geom), 1234, "meanstd", W, False, backend=hip, device=DEV,
                      kv_dtype="float16" if half else "float32", dec_dtype="float16" if dec_half else "float32",
                      **dr.batch_kwargs(W))


def _bits(sb, case):
    """the launch's output buffers as integers (NaN-proof comparison of two forms)"""
    return [getattr(sb, n).clone().view(torch.int32) for n in case.outputs()] + \
           [sb.skv.clone().view(torch.int32 if sb.skv.dtype == torch.float32 else torch.int16)]


def _kv_new_problems(case, sg, kref):
    """the appended rows: the reference k|v within the projection's own bound - exactly the inputs for the stand-alone
    kernel, which copies them - and rounded to fp16 for the half cache"""
    bad = []
    got = case.collect(sg, "kv_new")
    for s, g in got.items():
        ref, A = case.ref["kv_new"][s], case.A["kv_new"][s]
        if not np.isfinite(g).all():
            bad.append(f"kv_new: stream {s}: not finite")
        elif case.kind == "attn":
            if not np.array_equal(g, dr.f16(ref) if case.half else ref):
                bad.append(f"kv_new: stream {s}: the appended rows are not the new token's k|v")
        else:
            tol = 4 * kref * dr.EPS * A
            if case.half:            # round to nearest: half an ulp of 11 bits, or half the subnormal spacing
                tol = tol + 2.0 ** -11 * (np.abs(ref) + tol) + 2.0 ** -25
            if not (np.abs(g - ref) <= tol).all():
                bad.append(f"kv_new: stream {s}: worst error / tolerance {float((np.abs(g - ref) / tol).max()):.3g}")
    return bad


def _run(hip, sg, case, kref, which, tag, bad):
    """one launch and its checks; returns (kappas, bits)"""
    case.apply(sg)
    before = sg.skv.clone()
    dr.launch(hip, sg, case, which)
    torch.cuda.synchronize()
    names = [n for n in case.result_names(which) if n != "kv_new"]
    k = case.kappas(sg, names)
    for n in names:
        if not np.isfinite(k[n]):
            bad.append((tag, n, "non-finite output: a masked or out-of-range row entered a product"))
        elif not k[n] <= 4 * kref[n]:
            bad.append((tag, n, f"kappa {k[n]:.3g} > 4 x kappa_ref {kref[n]:.3g}"))
    appended = case.kind != "cross" and which != "cross"
    if appended:
        bad.extend((tag, m) for m in _kv_new_problems(case, sg, kref.get("kv_new", 0.0)))
    bad.extend((tag, m) for m in case.untouched_problems(sg, before, appended))
    return k, _bits(sg, case)


def _report(capsys, title, rows, bad=()):
    with capsys.disabled():
        print(f"\n{title}")
        for b in bad:
            print("  FAILED", b)
        for fam, kref, ks in rows:
            print(f"  {fam:10s} " + "; ".join(f"{n}: kappa_ref {kref[n]:.3g} kernel " + " / ".join(f"{k[n]:.3g}" for k in ks)
                                             for n in ks[0]))


@pytest.mark.parametrize("half", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("geom,W", ATTN_GEOMS)
def test_attention_kernels_against_float64(hip, monkeypatch, capsys, geom, W, half):
    """sc_dec_self_attn / sc_dec_cross_attn, SC_ATTN_DEEP = 0 / 1 (kernel kappas are printed in that order)"""
    sg = _gpu_batch(hip, geom, W, half)
    bad, rows = [], []
    for fam in dr.FAMILIES:
        case = dr.Case(geom, W, "attn", fam, half=half)
        kref, ks = {}, [{}, {}]
        for which in ("self", "cross"):
            kref.update(dr.spec_kappas(case, which))
            bits = []
            for i, deep in enumerate(("0", "1")):
                monkeypatch.setenv("SC_ATTN_DEEP", deep)
                k, b = _run(hip, sg, case, kref, which, (fam, which, "deep" + deep), bad)
                ks[i].update(k)
                bits.append(b)
            if not all(torch.equal(x, y) for x, y in zip(*bits)):
                bad.append((fam, which, "SC_ATTN_DEEP = 0 and 1 differ in bits"))
        rows.append((fam, kref, ks))
    _report(capsys, f"attention {geom} beam {W} {'fp16' if half else 'fp32'} K|V (kernel: deep 0 / deep 1)", rows, bad)
    assert not bad, bad


@pytest.mark.parametrize("half", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("kind", ["self", "cross"])
@pytest.mark.parametrize("geom,W", FUSED_GEOMS)
def test_fused_layer_kernels_against_float64(hip, monkeypatch, capsys, geom, W, kind, half):
    """sc_dec_layer_self / sc_dec_layer_cross: SC_DEC_HPW = 1 with SC_ATTN_DEEP = 0 / 1, SC_DEC_HPW = 4 (XL, beams <= 10); the
    layer / partial-sum variant rotates over the families and geometries (dr.layer_variant)"""
    sg = _gpu_batch(hip, geom, W, half)
    gi = FUSED_GEOMS.index((geom, W))
    bad, rows = [], []
    for f, fam in enumerate(dr.FAMILIES):
        li, npart = dr.layer_variant(f + gi)
        for hpw in (1, 4) if geom == "XL" and W <= 10 else (1,):
            case = dr.Case(geom, W, kind, fam, half=half, li=li if kind == "self" else 1, npart=npart, hpw=hpw)
            kref = dr.spec_kappas(case)
            monkeypatch.setenv("SC_DEC_HPW", str(hpw))
            ks, bits = [], []
            for deep in ("0", "1") if hpw == 1 else ("0",):
                monkeypatch.setenv("SC_ATTN_DEEP", deep)
                k, b = _run(hip, sg, case, kref, None, (fam, f"hpw{hpw}", "deep" + deep, f"layer {case.li} npart {npart}"), bad)
                ks.append(k)
                bits.append(b)
            if len(bits) == 2 and not all(torch.equal(x, y) for x, y in zip(*bits)):
                bad.append((fam, f"hpw{hpw}", "SC_ATTN_DEEP = 0 and 1 differ in bits"))
            rows.append((f"{fam} hpw{hpw}", kref, ks))
    _report(capsys, f"dec_layer_{kind} {geom} beam {W} {'fp16' if half else 'fp32'} K|V (kernel: deep 0 / deep 1)", rows, bad)
    assert not bad, bad


@pytest.mark.parametrize("kind", ["self", "cross"])
@pytest.mark.parametrize("geom,W,dec_half", HALF_GEOMS)
def test_fused_layer_kernels_in_fp16_decoder_mode(hip, monkeypatch, capsys, geom, W, dec_half, kind):
    """sc_dec_layer_self / sc_dec_layer_cross with the *_pph weights and fp16 partial products (SC_ACT_HALF = 1, 2, 3; fp16 K|V):
    the reduced case set of dec_attn_ref against float64 at 4 x the kappa the transcription of the mode's arithmetic needs;
    the same checks of what must stay untouched, on the fp16 elements of ph1 / ph2"""
    sg = _gpu_batch(hip, geom, W, True, dec_half=True)
    monkeypatch.setenv("SC_ACT_HALF", str(dec_half))
    sg._sc_search_struct = None                      # (the search struct carries act_half)
    assert hip.search_struct(sg).act_half == dec_half
    monkeypatch.setenv("SC_ATTN_DEEP", "0")
    bad, rows = [], []
    for case in half_cases(geom, W, kind, dec_half):
        kref = dr.transcription_kappas(case)
        monkeypatch.setenv("SC_DEC_HPW", str(case.hpw))
        k, _ = _run(hip, sg, case, kref, None, (case.family, f"hpw{case.hpw}", f"layer {case.li} npart {case.npart}"), bad)
        rows.append((f"{case.family} hpw{case.hpw}", kref, [k]))
    _report(capsys, f"dec_layer_{kind} {geom} beam {W} act_half {dec_half} (fp16 decoder mode)", rows, bad)
    assert not bad, bad


def test_stream_resident_layer_against_float64(hip, capsys):
    """sc_dec_layer_stream (XL, beam 10, fp32): xout, xn_out and the K|V append of both attention blocks in one launch"""
    sg = _gpu_batch(hip, "XL", 10, False)
    bad, rows = [], []
    for f, fam in enumerate(dr.FAMILIES):
        li, npart = dr.layer_variant(f)
        case = dr.Case("XL", 10, "stream", fam, li=li, npart=npart)
        kref = dr.spec_kappas(case)
        k, _ = _run(hip, sg, case, kref, None, (fam, f"layer {li} npart {npart}"), bad)
        rows.append((fam, kref, [k]))
    _report(capsys, "dec_layer_stream XL beam 10 fp32 K|V", rows, bad)
    assert not bad, bad

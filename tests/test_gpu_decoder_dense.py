"""The decoder's dense launches, each on its own against the float64 references of tests/dec_dense_ref.py: sc_dec_embed,
sc_dec_layer_ffn, sc_dec_layer_ffn_xn, sc_dec_layer_reduce_ln and sc_dec_output_logits (reduce_ln_rows_kernel + sc_gemm and the
reduce_ln_proj_kernel row panels), where the lock-step runs of test_gpu_ops.py see one stream of beam 10 - one 16-row tile, an
identity row table - against the fp32 spec at 5e-4.  Here a launch names M = 1 .. 90 rows (the 16-row tile edges up to five
tiles per workgroup) through a row table that is no identity, in four geometries (16, 18 and 5 hidden chunks; 8 and 4 heads;
d = 256 and 128 - sc_dec_layer_fused_supported(128, 4, W, 640) = 1: d = 128 is accepted, not refused), with one and four heads
per partial product, fp32 / fp16 / split16 feed-forward weights and the fp16 decoder mode (SC_ACT_HALF = 1, 2, 3, and 7 for the
row-panel output layer).  Per launch:
  1. every output is finite although every row the table does not list, the other buffers' slots and the partial slots >= n_part
     are NaN;
  2. kappa <= 4 x kappa_ref per output (dec_dense_ref: the spec's kappa on fp32 cases, the transcription's on fp16 / split16
     ones; 4: the kernels' k-ordered MFMA chains against blocked sums); sc_dec_embed: the reference's bits;
  3. rows the table does not list keep the sentinel bit for bit in xout, ffn_part, logits and dq, and so do the slots >= n_part;
     n_part is what the documented rule allows (F/128 or F/256, never more than max_part, pairs only - and always - beyond 2048);
  4. a row's xout and logits bits (the logits of sc_dec_output_logits fed with the launch's own partial sums) are the same at
     every M, at every place in the table and at both group counts.  The cost model never leaves one chunk per workgroup at
     these row counts (it does from 257 rows on), so the other count is forced with max_part = F/256, and the test asserts that
     both occurred.  With fp16 partial sums the two counts are different numbers by construction (rounded at the store): there
     n_part is F/256 at every row count and every max_part - a 1040-row batch holds the library to it.  sc_dec_layer_reduce_ln
     + sc_dec_layer_ffn_xn, called directly (the two launches the library's split hook runs), give the bits of sc_dec_layer_ffn;
  5. nothing is skipped: what the library refuses is asserted as SC_ERR_ARG with every output untouched.
The worst kappa per kernel and output, its kappa_ref and case are left as dec_dense_<kernel>.json in the reports
folder of the GPU tests (test_gpu_ops.write_report).  tests/test_dec_dense_ref_spec.py holds the references themselves to the spec on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import dec_dense_ref as dd
from test_gpu_ops import write_report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LI = dd.LI
SHUFFLED_M = (17, 49, 90)            # the row counts that are launched through the shuffled table too
REPORT = {}                          # kernel -> output -> dd.Worst


@pytest.fixture(scope="module")
def hip():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend(DEV)


def _gpu_batch(hip, geom, W, S, wform="float32", act_half=0):
    half = "float16" if act_half else "float32"
    return dd.make_batch(geom, W, S, backend=hip, device=DEV, ffn_dtype=wform, dec_dtype=half, kv_dtype=half)


def _mode(monkeypatch, hip, sg, hpw, act_half):
    """the switches of a launch, read as the library and the backend read them: SC_DEC_HPW, SC_ACT_HALF (the search struct is
    built anew: it carries act_half)"""
    monkeypatch.setenv("SC_DEC_HPW", str(hpw))
    monkeypatch.setenv("SC_ACT_HALF", str(act_half))
    sg._sc_search_struct = None
    assert hip.search_struct(sg).act_half == act_half


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _ffn(hip, sg, max_part=None):
    """sc_dec_layer_ffn with a max_part of the test's choosing (HipBackend.dec_layer_ffn passes the buffer's slot count)"""
    n = C.c_int(-1)
    mp = int(sg.ffn_part.shape[0] if max_part is None else max_part)
    hip._sb_call("sc_dec_layer_ffn", sg, LI, _ptr(sg.dx), _ptr(sg.dxn), _ptr(sg.ffn_part), mp, C.byref(n))
    torch.cuda.synchronize()
    return int(n.value)


def _see(kernel, k, kref, name, bad, tag, own=None):
    """holds a launch's kappas to 4 x kappa_ref; keeps the worst per kernel and output (own: of the calling test alone)"""
    for out, v in k.items():
        ref = kref[out]
        REPORT.setdefault(kernel, {}).setdefault(out, dd.Worst()).see(v, ref, name + " " + tag)
        if own is not None:
            own.setdefault(out, dd.Worst()).see(v, ref, name + " " + tag)
        if not np.isfinite(v):
            bad.append((name, tag, out, "not finite: a row the table does not list, or an unwritten slot, entered the result"))
        elif not v <= 4 * ref:
            bad.append((name, tag, out, f"kappa {v:.3g} > 4 x kappa_ref {ref:.3g}"))


def _leave_report(kernel):
    write_report("dec_dense_" + kernel, {out: {"kappa": w.kappa, "kappa_ref": w.kappa_ref, "worst_case": w.case}
                                         for out, w in REPORT.get(kernel, {}).items()})


def _same_bits(store, rows, arr, what, bad, tag):
    """a row's bits are what they were at its first launch"""
    for r in rows:
        b = arr[r].tobytes()
        if store.setdefault((what, int(r)), b) != b:
            bad.append((tag, f"{what}: row {int(r)} differs in bits from its first launch"))
            return


def _launches():
    return [(M, "descending") for M in dd.M_EDGES] + [(M, "shuffled") for M in SHUFFLED_M]


@pytest.mark.parametrize("geom,W,hpw,wform,act_half", dd.FFN_CONFIGS)
def test_feed_forward_launch_against_float64(hip, monkeypatch, capsys, geom, W, hpw, wform, act_half):
    """sc_dec_layer_ffn over the row edges and both tables, at the group count the cost model takes and at F/256 forced through
    max_part; each launch's partial sums are fed into sc_dec_output_logits: xout and logits bits per row"""
    sg = _gpu_batch(hip, geom, W, 90 // W, wform, act_half)
    _mode(monkeypatch, hip, sg, hpw, act_half)
    F = dd.GEOMS[geom]["ffn_dim"]
    allowed = dd.n_part_rule(F, F // 128, bool(act_half & 2))
    bad, seen, own = [], set(), {}
    for fam in dd.FAMILIES:
        case = dd.ffn_case(geom, W, fam, hpw, wform, act_half)
        kref = dd.ffn_kappa_ref(geom, W, fam, hpw, wform, act_half)
        bits = {}
        for M, perm in _launches():
            for max_part in (None, F // 256) if F <= 2048 and F % 256 == 0 and M in (1, 17, 33, 81, 90) else (None,):
                tag = f"M={M} {perm} max_part={max_part}"
                dd.apply_ffn(sg, case, M, perm)
                n_part = _ffn(hip, sg, max_part)
                seen.add(n_part)
                if n_part not in dd.n_part_rule(F, max_part or F // 128, case.part_half):
                    bad.append((case.name, tag, f"n_part {n_part} is not what the rule allows"))
                    continue
                rows = case.maps[perm][:M]
                xout = sg.dxn.cpu().numpy()
                parts, _ = dd.read_parts(sg, case.part_half)
                _see("dec_layer_ffn", case.kappas_of(rows, xout[rows], None, parts[:n_part, rows]), kref, case.name, bad, tag, own)
                bad.extend((case.name, tag, m) for m in dd.ffn_sentinel_problems(case, sg, M, perm, n_part))
                if not bool(torch.isnan(sg.ph1).all()):
                    bad.append((case.name, tag, "ph1 written"))
                _same_bits(bits, rows, xout, "xout", bad, (case.name, tag))
                # the consumer: residual + tree of the partial sums + b2, after_norm, output layer
                sg.logits.fill_(dd.SENTINEL)
                hip.dec_output_logits(sg, sg.dxn, sg.dx, n_part)
                torch.cuda.synchronize()
                lg = sg.logits.cpu().numpy()
                if not np.isfinite(lg[rows]).all() or not (lg[~case.listed(M, perm)] == np.float32(dd.SENTINEL)).all():
                    bad.append((case.name, tag, "logits of the launch's partial sums: not finite, or an unlisted row written"))
                _same_bits(bits, rows, lg, "logits", bad, (case.name, tag))
                _same_bits(bits, rows, sg.dx.cpu().numpy(), "x + feed-forward", bad, (case.name, tag))
    _leave_report("dec_layer_ffn")
    with capsys.disabled():
        print(f"\ndec_layer_ffn {geom} beam {W} hpw {hpw} {wform} act_half {act_half}: n_part seen {sorted(seen)}; " +
              "; ".join(f"{o}: kappa {w.kappa:.3g} (kappa_ref {w.kappa_ref:.3g})" for o, w in own.items()))
        for b in bad[:20]:
            print("  FAILED", b)
    assert not bad, bad[:20]
    assert seen == set(allowed), (seen, allowed)           # both group counts occurred (F = 2304 and 640, and fp16 partial sums, have one)


@pytest.mark.parametrize("geom,W,act_half", dd.LOGITS_CONFIGS)
def test_output_layer_launch_against_float64(hip, monkeypatch, capsys, geom, W, act_half):
    """sc_dec_output_logits with 1, 2, 8, 9 and 16 partial sums: reduce_ln_rows_kernel + sc_gemm (act_half 0, 2, 3; V = 1024 and
    1280) and the row panels (SC_ACT_HALF = 7: fp16 output weights), over the row edges and both tables"""
    sg = _gpu_batch(hip, geom, W, 90 // W, "float32", act_half)
    _mode(monkeypatch, hip, sg, 1, act_half)
    rows_form = not act_half & 4
    bad, own = [], {}
    for f, fam in enumerate(dd.FAMILIES):
        for npart in dd.nparts_of(geom):
            case = dd.logits_case(geom, W, fam, npart, act_half)
            kref = dd.logits_kappa_ref(geom, W, fam, npart, act_half)
            bits = {}
            for M, perm in _launches():
                tag = f"M={M} {perm}"
                dd.apply_logits(sg, case, M, perm)
                hip.dec_output_logits(sg, sg.dx, sg.dxn, npart)
                torch.cuda.synchronize()
                rows = case.maps[perm][:M]
                xout, lg = sg.dxn.cpu().numpy(), sg.logits.cpu().numpy()
                xn = sg.dq.cpu().numpy() if rows_form else None
                _see("dec_output_logits", case.kappas_of(rows, xout[rows], None if xn is None else xn[rows], lg[rows]), kref,
                     case.name, bad, tag, own)
                bad.extend((case.name, tag, m) for m in dd.logits_sentinel_problems(case, sg, M, perm, rows_form))
                _same_bits(bits, rows, xout, "xout", bad, (case.name, tag))
                _same_bits(bits, rows, lg, "logits", bad, (case.name, tag))
    _leave_report("dec_output_logits")
    with capsys.disabled():
        print(f"\ndec_output_logits {geom} beam {W} act_half {act_half}: " +
              "; ".join(f"{o}: kappa {w.kappa:.3g} (kappa_ref {w.kappa_ref:.3g})" for o, w in own.items()))
        for b in bad[:20]:
            print("  FAILED", b)
    assert not bad, bad[:20]


def test_output_layer_row_panels_two_column_blocks(hip, monkeypatch, capsys):
    """the row-panel form (SC_ACT_HALF = 7) at 1040 rows: cdiv(M, 16) * (V / d) = 65 * 4 > 256, so a workgroup takes two column
    blocks (cb = 2); at M = 17 it takes one - the same rows, the same bits"""
    geom, W, S, npart = "D8", 10, 104, 8
    sg = _gpu_batch(hip, geom, W, S, "float32", 7)
    _mode(monkeypatch, hip, sg, 1, 7)
    case = dd.logits_case(geom, W, "normal", npart, 7, S)
    kref = dd.logits_kappa_ref(geom, W, "normal", npart, 7, S)
    assert -(-case.n // 16) * (case.V // case.d) > 256 and case.n == 1040
    bad, bits = [], {}
    for M, perm in ((case.n, "shuffled"), (17, "shuffled"), (case.n, "descending")):
        tag = f"M={M} {perm}"
        dd.apply_logits(sg, case, M, perm)
        hip.dec_output_logits(sg, sg.dx, sg.dxn, npart)
        torch.cuda.synchronize()
        rows = case.maps[perm][:M]
        xout, lg = sg.dxn.cpu().numpy(), sg.logits.cpu().numpy()
        _see("dec_output_logits", case.kappas_of(rows, xout[rows], None, lg[rows]), kref, case.name, bad, tag)
        bad.extend((case.name, tag, m) for m in dd.logits_sentinel_problems(case, sg, M, perm, False))
        _same_bits(bits, rows, xout, "xout", bad, (case.name, tag))
        _same_bits(bits, rows, lg, "logits", bad, (case.name, tag))
    _leave_report("dec_output_logits")
    with capsys.disabled():
        print("\ndec_output_logits 1040 rows, row panels: " +
              "; ".join(f"{o}: kappa {w.kappa:.3g} (kappa_ref {w.kappa_ref:.3g})" for o, w in REPORT["dec_output_logits"].items()))
    assert not bad, bad[:20]


def test_fp16_partial_sums_do_not_depend_on_the_row_count(hip, monkeypatch):
    """REGRESSION: with fp16 partial sums (act_half & 2) sc_dec_layer_ffn took its group count from the
    cost model like the fp32 form - F/128 up to 256 rows, F/256 at 1040 - but a pair that is summed and then rounded is another
    number than the sum of its two rounded halves: a row's feed-forward depended on how many rows were in the launch.  The
    count is F/256 at every row count now; the same rows at M = 17 and M = 1040 give the same xout, partial sums and logits."""
    geom, W, S = "D8", 10, 104
    sg = _gpu_batch(hip, geom, W, S, "float32", 3)
    _mode(monkeypatch, hip, sg, 1, 3)
    case = dd.ffn_case(geom, W, "normal", 1, "float32", 3, S)
    bad, bits, counts = [], {}, {}
    for M, perm in ((case.n, "shuffled"), (17, "shuffled"), (257, "shuffled"), (case.n, "descending")):
        tag = f"M={M} {perm}"
        dd.apply_ffn(sg, case, M, perm)
        counts[M] = n_part = _ffn(hip, sg)
        rows = case.maps[perm][:M]
        bad.extend((tag, m) for m in dd.ffn_sentinel_problems(case, sg, M, perm, n_part))
        _same_bits(bits, rows, sg.dxn.cpu().numpy(), "xout", bad, tag)
        parts, _ = dd.read_parts(sg, True)
        if n_part == case.nch // 2:
            _same_bits(bits, rows, np.ascontiguousarray(parts[:n_part].transpose(1, 0, 2)), "ffn_part", bad, tag)
        sg.logits.fill_(dd.SENTINEL)
        hip.dec_output_logits(sg, sg.dxn, sg.dx, n_part)
        torch.cuda.synchronize()
        _same_bits(bits, rows, sg.logits.cpu().numpy(), "logits", bad, tag)
    assert set(counts.values()) == {case.nch // 2}, counts
    assert not bad, bad[:20]


def test_split_feed_forward_gives_the_same_bits(hip, monkeypatch, capsys):
    """sc_dec_layer_reduce_ln + sc_dec_layer_ffn_xn, called directly - the two launches the split hook puts in the place of sc_dec_layer_ffn
    (d = 256, four heads per workgroup, fp32 partial products) - give its xout bits and, through the consumer's reduce, its
    feed-forward bits; xn and the prologue-less feed-forward on its own rows lie within the error model"""
    geom, W, hpw = "D8", 10, 4
    sg = _gpu_batch(hip, geom, W, 9)
    _mode(monkeypatch, hip, sg, hpw, 0)
    bad = []
    for fam in dd.FAMILIES:
        case = dd.ffn_case(geom, W, fam, hpw, "float32", 0)
        kref = dd.ffn_kappa_ref(geom, W, fam, hpw, "float32", 0)
        for M, perm in _launches():
            tag = f"M={M} {perm}"
            rows = case.maps[perm][:M]
            off = ~case.listed(M, perm)
            # one launch
            dd.apply_ffn(sg, case, M, perm)
            n_part = _ffn(hip, sg)
            x_one = sg.dxn.cpu().numpy()
            hip.dec_output_logits(sg, sg.dxn, sg.dx, n_part)
            torch.cuda.synchronize()
            y_one = sg.dx.cpu().numpy()
            # two launches: the rows xn go through dq, as in sc_decode_step
            dd.apply_ffn(sg, case, M, perm)
            sg.dq.fill_(dd.SENTINEL)
            hip._sb_call("sc_dec_layer_reduce_ln", sg, LI, _ptr(sg.dx), _ptr(sg.dxn), _ptr(sg.dq))
            torch.cuda.synchronize()
            x_two, xn = sg.dxn.cpu().numpy(), sg.dq.cpu().numpy()
            if not (xn[off] == np.float32(dd.SENTINEL)).all() or not (x_two[off] == np.float32(dd.SENTINEL)).all():
                bad.append((case.name, tag, "reduce_ln: a row the table does not list was written"))
            _see("dec_layer_reduce_ln", {"xout": dd.kappa(x_two[rows], case.ref["xout"][rows], case.A["xout"][rows]),
                                         "xn": dd.kappa(xn[rows], case.ref["xn"][rows], case.A["xn"][rows])}, kref, case.name, bad, tag)
            n_two = hip.dec_layer_ffn_xn(sg, LI, sg.dq)
            torch.cuda.synchronize()
            if n_two not in dd.n_part_rule(case.F, case.F // 128):
                bad.append((case.name, tag, f"ffn_xn: n_part {n_two}"))
            bad.extend((case.name, tag, "ffn_xn: " + m) for m in dd.ffn_sentinel_problems(case, sg, M, perm, n_two, xout=False))
            hip.dec_output_logits(sg, sg.dxn, sg.dx, n_two)
            torch.cuda.synchronize()
            y_two = sg.dx.cpu().numpy()
            if x_one[rows].tobytes() != x_two[rows].tobytes():
                bad.append((case.name, tag, "xout: the split form differs in bits"))
            if y_one[rows].tobytes() != y_two[rows].tobytes():
                bad.append((case.name, tag, f"x + feed-forward: the split form (n_part {n_two}) differs in bits from the one launch ({n_part})"))
            # the prologue-less form on rows of its own
            dd.apply_ffn(sg, case, M, perm)
            n_xn = hip.dec_layer_ffn_xn(sg, LI, sg.dq)
            torch.cuda.synchronize()
            parts, _ = dd.read_parts(sg, False)
            k = case.kappas_of(rows, None, None, parts[:n_xn, rows], xn_form=True)
            _see("dec_layer_ffn_xn", {"ffn_xn": k["ffn"]}, kref, case.name, bad, tag)
            bad.extend((case.name, tag, "ffn_xn: " + m) for m in dd.ffn_sentinel_problems(case, sg, M, perm, n_xn, xout=False))
    _leave_report("dec_layer_reduce_ln")
    _leave_report("dec_layer_ffn_xn")
    with capsys.disabled():
        for kern in ("dec_layer_reduce_ln", "dec_layer_ffn_xn"):
            print(f"\n{kern}: " + "; ".join(f"{o}: kappa {w.kappa:.3g} (kappa_ref {w.kappa_ref:.3g})" for o, w in REPORT[kern].items()))
    assert not bad, bad[:20]


@pytest.mark.parametrize("geom,W", [("D8", 10), ("D4", 10), ("D8", 5), ("D128", 10)])
def test_embed_launch_gives_the_reference_bits(hip, geom, W):
    """sc_dec_embed: L - 1 in 0, 1, LCAP - 2; tokens 0, V - 1 and a repeated id; nh < W; an inactive stream.  E = 0 at d = 256:
    the reference's bits; d = 128 (the product with sqrt(d) rounds): 4 x the spec's kappa"""
    case = dd.EmbedCase(geom, W)
    sg = _gpu_batch(hip, geom, W, case.S)
    dd.apply_embed(sg, case)
    hip.dec_embed(sg)
    torch.cuda.synchronize()
    kref = dd.embed_kappa_ref(geom, W)
    dx = sg.dx.cpu().numpy()
    bad = case.problems(dx, kref)
    if case.exact:
        REPORT.setdefault("dec_embed", {})["dx"] = dd.Worst(0.0, 0.0, case.name + (": the reference's bits" if not bad else ": " + bad[0]))
    else:
        REPORT.setdefault("dec_embed", {})["dx (d = 128)"] = dd.Worst(case.kappa_of(dx), kref, case.name)
    _leave_report("dec_embed")
    assert not bad, bad


def test_refused_forms_leave_everything_untouched(hip, monkeypatch):
    """SC_ERR_ARG and not one element written: sc_dec_output_logits at a V that is no multiple of d (scasr.h: "needs the
    lane-packed output layer (V a multiple of d)"), sc_dec_layer_ffn with max_part below F/256, sc_dec_layer_reduce_ln with fp16
    partial products; and d = 128 is a geometry the fused layers accept"""
    from speechcatcher_amd._abi import ScasrError, load
    assert load().sc_dec_layer_fused_supported(128, 4, 10, 640) == 1 and load().sc_dec_layer_fused_supported(128, 4, 10, 600) == 0
    sg = _gpu_batch(hip, "D8", 10, 9)
    _mode(monkeypatch, hip, sg, 1, 0)
    case = dd.logits_case("D8", 10, "normal", 8, 0)
    outs = ("dxn", "dq", "logits")

    def untouched():
        torch.cuda.synchronize()
        return all(bool((getattr(sg, n) == dd.SENTINEL).all()) for n in outs)

    dd.apply_logits(sg, case, 33, "shuffled")
    s = hip.search_struct(sg)
    s.V = 1000
    with pytest.raises(ScasrError, match=r"\(-1\).*multiple of d"):
        hip.dec_output_logits(sg, sg.dx, sg.dxn, 8)
    s.V = 1024
    assert untouched()
    fcase = dd.ffn_case("D8", 10, "normal", 1, "float32", 0)
    dd.apply_ffn(sg, fcase, 33, "shuffled")
    with pytest.raises(ScasrError, match=r"\(-1\).*max_part"):
        _ffn(hip, sg, 7)
    torch.cuda.synchronize()
    assert bool((sg.dxn == dd.SENTINEL).all()) and bool((sg.ffn_part == dd.SENTINEL).all())
    # fp16 partial products: the launch of its own refuses them (the feed-forward keeps its prologue in that mode)
    sh = _gpu_batch(hip, "D8", 10, 9, "float32", 2)
    _mode(monkeypatch, hip, sh, 4, 2)
    hcase = dd.ffn_case("D8", 10, "normal", 4, "float32", 2)
    dd.apply_ffn(sh, hcase, 33, "shuffled")
    sh.dq.fill_(dd.SENTINEL)
    with pytest.raises(ScasrError, match=r"\(-1\).*fp32 partial products"):
        hip._sb_call("sc_dec_layer_reduce_ln", sh, LI, _ptr(sh.dx), _ptr(sh.dxn), _ptr(sh.dq))
    torch.cuda.synchronize()
    assert bool((sh.dxn == dd.SENTINEL).all()) and bool((sh.dq == dd.SENTINEL).all())

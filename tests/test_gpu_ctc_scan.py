"""The CTC prefix scan and the rebuild of the winners' forward variables (sc_ctc_prefix_scan_split + sc_ctc_gather_state_split:
ctc_prefix_scan_colmajor_kernel, ctc_prefix_scan_tpar_kernel, ctc_gather_state_kernel), one scan launch and one rebuild launch per
case, against the float64 reference of tests/ctc_scan_ref.py.  Where test_gpu_ops.py::test_ctc_prefix_scan_long_table gives every
stream of a batch the same T, L and state and compares with the fp32 spec, the cases here mix streams of different T, L, nh, has
and cur - one of them inactive - in one launch, put T and L on the places where the frame walk branches (checkpoint frames, chunk
and segment edges, nothing to walk, T = TCAP, the threshold between the two scan kernels, empty segments, the stale-table length),
and let the two scan kernels share a batch.  Per case:
  * psi, the eos score, every rebuilt r[t] and r^n (+) r^b of the winners and the rows the scan parks in ctc_rnew lie within the error
    model at 4 x kappa_ref, and the same entries are logzero; kappa_ref = the larger kappa of the fp32 torch spec and of a float32
    transcription of the segment-affine form, both measured here on the CPU (4: the hardware exp2 / log are good to about one ulp
    where libm is good to half, and the combine adds three log-add-exps per segment);
  * everything is finite although everything the launches must not read is NaN;
  * ctc_rnew holds 16-frame checkpoints for the streams the sequential kernel walks - equal, bit for bit, to the winners' rebuilt
    rows at those frames: the rebuild is the scan's recurrence - and 32 segment start states for the streams that are split;
  * dead hypothesis rows, the inactive stream, rows >= T and the whole `cur` side keep their bits, as do all inputs;
  * every active stream, run again alone in a batch of one, gives the same bits; a stream the sequential kernel walks gives the
    same bits whether the launch is allowed to split others (split_min 16) or not (0) - and the streams that change kernels in
    that second launch of the batch pass all of the above in their other form too.
kappa_ref and the kernel kappas of every case are printed and go to ctc_scan_parity.json beside the other reports of the GPU tests
(test_gpu_ops.write_report)."""
import numpy as np
import pytest
import torch

import ctc_scan_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INPUTS = ("ctrl", "ctcx", "ctcxT", "pre_ids", "yseq", "sel")
_batches = {}
_report_all = {}


@pytest.fixture(scope="module")
def hip():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend(DEV)


def _gpu_batch(hip, V, W, S, max_frames):
    from test_engine_spec import make_batch
    key = (V, W, S, max_frames)
    if key not in _batches:
        _batches[key] = make_batch(cr.cfg_name(V), 1234, "meanstd", W, False, backend=hip, device=DEV,
                                   **cr.batch_kwargs(S, max_frames))
    return _batches[key]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _is_sentinel(a):
    return bool((np.asarray(a) == cr.SENTINEL).all())


def _launch(hip, sb, c, slots, split_min):
    """the case's streams `slots` in the batch, one scan and one rebuild; returns the outputs per stream and the bits of the
    inputs before and after"""
    c.apply(sb, slots)
    before = {n: getattr(sb, n).clone() for n in INPUTS}
    hip.ctc_prefix_scan(sb, split_min=split_min)
    hip.ctc_gather_state(sb, split_min=split_min)
    torch.cuda.synchronize()
    changed = [n for n in INPUTS if not torch.equal(getattr(sb, n).view(torch.int32), before[n].view(torch.int32))]
    return {s: c.collect(sb, slot, s) for slot, s in slots}, changed


def _check_stream(c, s, o, split, kref, bad):
    """one stream of the mixed launch; returns its kappas"""
    st, d, W, K = c.streams[s], c.data[s], c.W, c.K
    T, nh = st.Te, st.nh
    tag = (c.name, f"stream {s} ({'split' if split else 'sequential'})")
    rows = cr.NSEG if split else T // cr.CK
    if not _same_bits(o["r_cur"], d["r"][st.cur]) or not _same_bits(o["rs_cur"], d["rs"][st.cur]):
        bad.append((*tag, "the cur side of ctc_r / ctc_rs changed"))
    if not st.active:
        for n in ("psi", "psi_eos", "rnew"):
            if not _is_sentinel(o[n]):
                bad.append((*tag, f"{n} of the inactive stream written"))
        if not _same_bits(o["r"], d["r"][1 - st.cur]) or not _same_bits(o["rs"], d["rs"][1 - st.cur]):
            bad.append((*tag, "ctc_r / ctc_rs of the inactive stream written"))
        return None
    # what must keep the sentinel
    for n, part in (("psi rows >= nh", o["psi"][nh:]), ("psi_eos rows >= nh", o["psi_eos"][nh:]),
                    ("ctc_rnew columns >= nh K", o["rnew"][:, :, nh * K:]), (f"ctc_rnew rows >= {rows}", o["rnew"][rows:]),
                    ("ctc_r rows >= T", o["r"][T:]), ("ctc_rs rows >= T", o["rs"][T:])):
        if not _is_sentinel(part):
            bad.append((*tag, f"{n} written"))
    # which kernel took the stream: 32 segment states, or T // 16 checkpoints (what lies behind them is the sentinel: above)
    written = o["rnew"][:rows, :, :nh * K]
    if (written == cr.SENTINEL).any():
        bad.append((*tag, f"ctc_rnew: not every one of the {rows} rows written"))
    for n, part in (("psi", o["psi"][:nh]), ("psi_eos", o["psi_eos"][:nh]), ("ctc_rnew", written), ("ctc_r", o["r"][:T]),
                    ("ctc_rs", o["rs"][:T])):
        if not np.isfinite(part).all():
            bad.append((*tag, f"{n}: not finite - something the launch must not read entered"))
    ks = c.kappas(o, s, split)
    for n, (k, masks) in ks.items():
        if not masks:
            bad.append((*tag, n, "not the same entries logzero as in the reference"))
        if not k <= 4 * kref[n]:
            bad.append((*tag, n, f"kappa {k:.3g} > 4 x kappa_ref {kref[n]:.3g}"))
    if not split:        # the rebuild walks the scan's recurrence: the winners' rows at the checkpoint frames ARE the checkpoints
        e = d["sel"][:, 0] * K + d["sel"][:, 1]
        if not _same_bits(o["rnew"][:rows][:, :, e], o["r"][cr.CK - 1:cr.CK * rows:cr.CK]):
            bad.append((*tag, "rebuilt r[16 j + 15] of the winners differs in bits from the scan's checkpoints"))
    return {n: k for n, (k, _) in ks.items()}


def _report(capsys, c, kref, kspec, kaff, per_stream, other_form, other, bad):
    kernel = {n: max((k[n] for k in per_stream.values()), default=0.0) for n in cr.OUTPUTS}
    with capsys.disabled():
        print(f"\nctc scan {c.name} (V {c.V}, beam {c.W}, TCAP {c.TCAP}, split_min {c.split_min})")
        for b in bad:
            print("  FAILED", b)
        for n in cr.OUTPUTS:
            print(f"  {n:8s} kappa_ref {kref[n]:.3g} (spec {kspec[n]:.3g}, affine-f32 {kaff[n]:.3g})  kernel {kernel[n]:.3g}  [" +
                  ", ".join(f"s{s} {'par' if c.split(s) else 'seq'} {k[n]:.3g}" for s, k in per_stream.items()) + "]" +
                  (f"  at split_min {other}: [" + ", ".join(f"s{s} {'par' if c.split(s, other) else 'seq'} {k[n]:.3g}"
                                                             for s, k in other_form.items()) + "]" if other_form else ""))
    from test_gpu_ops import write_report
    rep = _report_all
    rep[c.name] = dict(kappa_ref=kref, kappa_spec=kspec, kappa_affine_f32=kaff, kernel=kernel,
                       streams={str(s): dict(form="split" if c.split(s) else "sequential", T=c.streams[s].Te, L=c.streams[s].L,
                                             nh=c.streams[s].nh, has=c.streams[s].has, kappa=k) for s, k in per_stream.items()},
                       other_split_min={"split_min": other, "streams": {
                           str(s): dict(form="split" if c.split(s, other) else "sequential", kappa=k) for s, k in other_form.items()}},
                       failed=[" / ".join(str(x) for x in b) for b in bad])
    write_report("ctc_scan_parity", rep)        # (all cases of this run so far)


@pytest.mark.parametrize("name", list(cr.CASES))
def test_scan_and_rebuild_against_float64(hip, capsys, name):
    c = cr.case(name)
    kref, kspec, kaff = cr.kappa_ref(name)
    sb = _gpu_batch(hip, c.V, c.W, c.S, c.TCAP)
    one = _gpu_batch(hip, c.V, c.W, 1, c.TCAP)
    bad, per_stream = [], {}
    outs, changed = _launch(hip, sb, c, [(s, s) for s in range(c.S)], c.split_min)
    if changed:
        bad.append((name, f"inputs changed: {changed}"))
    for s in range(c.S):
        k = _check_stream(c, s, outs[s], c.split(s), kref, bad)
        if k is not None:
            per_stream[s] = k
    if c.split_min > 0:      # (the case's own table says which streams split: both kernels have work in these launches)
        assert any(c.split(s) for s in c.live) and any(not c.split(s) for s in c.live)
    names = ("psi", "psi_eos", "rnew", "r", "rs")
    # composition independence: the stream alone in a batch of one
    for s in c.live:
        alone, _ = _launch(hip, one, c, [(0, s)], c.split_min)
        diff = [n for n in names if not _same_bits(alone[s][n], outs[s][n])]
        if diff:
            bad.append((name, f"stream {s}", f"alone in a batch of one: other bits in {diff}"))
    # a stream the sequential kernel walks either way: the same bits at split_min 0 and 16
    other = 16 if c.split_min == 0 else 0
    again, _ = _launch(hip, sb, c, [(s, s) for s in range(c.S)], other)
    other_form = {}
    for s in range(c.S):
        if s in c.live and not c.split(s, 0) and not c.split(s, 16):
            diff = [n for n in names if not _same_bits(again[s][n], outs[s][n])]
            if diff:
                bad.append((name, f"stream {s}", f"split_min {other} against {c.split_min}: other bits in {diff}"))
        else:            # the inactive stream, and the streams that take the other kernel in this launch: all checks again
            k = _check_stream(c, s, again[s], c.split(s, other), kref, bad)
            if k is not None:
                other_form[s] = k
    _report(capsys, c, kref, kspec, kaff, per_stream, other_form, other, bad)
    assert not bad, bad

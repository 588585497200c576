"""Cases, a float64 reference and an error model for the CTC prefix scan and the rebuild of the winners' forward variables
(sc_ctc_prefix_scan_split / sc_ctc_gather_state_split: ctc_prefix_scan_colmajor_kernel, ctc_prefix_scan_tpar_kernel and
ctc_gather_state_kernel of csrc/search.hip).  numpy throughout, no GPU.  tests/test_ctc_scan_ref_spec.py holds the reference
to the torch spec on the CPU, tests/test_gpu_ctc_scan.py holds the HIP kernels to it.

REFERENCE.  reference_stream(): Watanabe's Algorithm 2 as SpecBackend.ctc_prefix_scan / ctc_gather_state define it, in float64,
one loop over the frames with the (hypothesis, candidate) pairs of a stream side by side: logzero = -1e10,
start = min(max(L - 1, 1), T), r[start-1][n] = x[0, c] only when L == 1, a prefix without state has r_prev^b = the running
blank sum (and r_prev^n = logzero), the eos candidate scores r_sum[T-1], the blank candidate logzero, ctrl[SC_C_TCTC] > 0
overrides T.

A CASE is one launch over 4 or 5 streams that differ in (active, T, L, nh, has, tctc, cur).  It is written identically into a CPU
batch (SpecBackend) and a GPU batch (HipBackend).  The table is a log-softmax with raw-logit rows behind frame 24; the state
of the previous prefix is what the reference leaves one step earlier (rows in front of the prefix are exactly logzero, ctc_rs
is the sum of ctc_r); the candidates of every live hypothesis hold its last token, eos and blank.  Everything the launch must
not read is NaN (an id past the vocabulary in integer buffers), everything it must not write carries SENTINEL.

ERROR MODEL.  Every frame of the walk rounds a handful of times relative to the magnitudes it handles, and the recurrence
hands an error on with a gain of at most one (a log-add-exp is a convex combination of its arguments' errors).  So a value
after the frames start .. t has
    A[t] = A0 + sum over tau = start .. t of (1 + max(|r^n[tau]|, |r^b[tau]|, |phi[tau-1] + x[tau, c]|))
with the terms at or below -1e9 left out and A0 = 1 + |r[start-1][n]|; r^n (+) r^b has A[t] + 1 + |rs[t]|.  psi is a
log-sum-exp over the whole walk, but a term moves it only by its softmax weight w (behind a peak of phi + x the frames of a
long table do not reach it at all, and the walk's running sum would leave them a kappa of 1e-5 where anything could hide):
    A_psi = 1 + |psi| + sum over the terms of w (1 + |phi + x| + A_phi),
A_phi = |phi| for a stored state (its one rounding), the running sum of 1 + |blank sum| without one; the eos score 1 + |r_sum[T-1]| (the sum of 1 + |blank sum| over the frames without state).  A result has
kappa = max |result - ref| / (2^-24 A) over the entries whose reference is above -1e9; the others are logzero, and which ones
are is compared as a mask.  The constant is NOT chosen here: kappa_ref is measured on the CPU, per case and output, as the
larger of the kappa of the fp32 torch spec and of segment_affine_f32() - a numpy float32 transcription of the segment-affine
form of the T-parallel scan with every intermediate rounded - and a kernel is allowed 4 x kappa_ref."""
import dataclasses
import functools

import numpy as np
import torch

LOGZERO = -1.0e10
LIVE = -1.0e9                        # a value above it is a number, at or below it logzero
EPS = 2.0 ** -24
SENTINEL = -77.25                    # in every buffer the launch must not write
NSEG, CK = 32, 16                    # segments of the T-parallel scan; checkpoint distance of the sequential one
F32 = np.float32
OUTPUTS = ("psi", "psi_eos", "r", "rs", "rnew")


# ---------------------------------------------------------------------------------------------------------------------
# streams and cases
@dataclasses.dataclass
class Stream:
    active: int
    T: int
    L: int
    nh: int
    has: int
    tctc: int = 0
    cur: int = 0

    @property
    def Te(self):
        """the rows of the table the step sees (scasr.h: SC_C_TCTC)"""
        return self.tctc if self.tctc > 0 else self.T

    @property
    def start(self):
        return min(max(self.L - 1, 1), self.Te)

    @property
    def ctrl(self):
        return [self.active, self.cur, 0, self.T, self.L, self.nh, self.has, self.tctc]

    def segments(self):
        """[t_lo, t_hi) of the 32 segments of the T-parallel form"""
        T, start = self.Te, self.start
        base = start & ~15
        seg = 16 * -(-(T - base) // (16 * NSEG))
        return [(max(start, base + p * seg), min(T, base + (p + 1) * seg)) for p in range(NSEG)]


@dataclasses.dataclass(frozen=True)
class CaseSpec:
    name: str
    V: int
    W: int
    max_frames: int
    split_min: int
    streams: tuple                   # of (active, T, L, nh, has, tctc)


def effective_split(max_frames, split_min):
    """the T-parallel form parks 32 segment states per pair where the checkpoints live: off for shorter tables"""
    return split_min if (max_frames + CK - 1) // CK >= NSEG else 0


def is_split(st, max_frames, split_min):
    eff = effective_split(max_frames, split_min)
    return eff > 0 and st.Te - st.start >= eff


def _nh(W, i):
    return (W, W - 3, 1)[i % 3]


def _with_inactive(rows, at, W):
    rows = list(rows)
    rows.insert(at, (0, 29, 4, W, 1, 0))
    return tuple(rows)


def _case_table():
    out = []
    # sequential form: T in {1, 2, 15, 16, 17, 31, 32, 33} x L in {1, 2, 3}, three of the 24 to a batch
    combos = [(T, L) for T in (1, 2, 15, 16, 17, 31, 32, 33) for L in (1, 2, 3)]
    for b in range(8):
        W = 10 if b % 2 == 0 else 5
        rows = []
        for j, i in enumerate((b, b + 8, b + 16)):
            T, L = combos[i]
            rows.append((1, T, L, _nh(W, b + j), (i // 3 + i % 3) % 2, 0))
        out.append(CaseSpec(f"seq_T{'_'.join(str(combos[i][0]) for i in (b, b + 8, b + 16))}", 1024, W, 500, 0,
                            _with_inactive(rows, b % 4, W)))
    # start - 1 in front of, on and behind a checkpoint frame
    out.append(CaseSpec("seq_T40_start15_16_17", 1024, 10, 500, 0,
                        _with_inactive([(1, 40, 16, 7, 1, 0), (1, 40, 17, 10, 0, 0), (1, 40, 18, 1, 1, 0)], 1, 10)))
    # nothing walked: L - 1 in {T, T + 4}
    out.append(CaseSpec("seq_nothing_walked", 1024, 5, 500, 0,
                        _with_inactive([(1, 20, 21, 5, 1, 0), (1, 20, 25, 2, 0, 0), (1, 33, 38, 1, 1, 0)], 3, 5)))
    # the stale-table length: 24 rows seen of T = 40
    out.append(CaseSpec("seq_tctc24", 1024, 10, 500, 0,
                        _with_inactive([(1, 40, 3, 10, 1, 24), (1, 40, 9, 7, 0, 0), (1, 24, 1, 1, 0, 0)], 0, 10)))
    # T = TCAP, TCAP no multiple of 16 (nor of 4: the column-major copy has three padding columns)
    out.append(CaseSpec("seq_T_is_TCAP45", 1024, 5, 45, 0,
                        _with_inactive([(1, 45, 1, 5, 0, 0), (1, 45, 20, 2, 1, 0), (1, 44, 2, 1, 1, 0)], 2, 5)))
    out.append(CaseSpec("seq_V1182", 1182, 10, 500, 0,
                        _with_inactive([(1, 33, 2, 10, 1, 0), (1, 17, 1, 7, 0, 0), (1, 40, 18, 1, 1, 0)], 1, 10)))
    out.append(CaseSpec("seq_V37", 37, 10, 500, 0,
                        _with_inactive([(1, 31, 3, 7, 1, 0), (1, 16, 1, 1, 0, 0), (1, 40, 17, 10, 0, 0)], 2, 10)))
    # T-parallel form, split_min = 16.  T - start = 15 stays sequential, 16 splits
    out.append(CaseSpec("par_threshold_15_16", 1024, 10, 520, 16,
                        _with_inactive([(1, 19, 5, 10, 1, 0), (1, 20, 5, 7, 1, 0), (1, 36, 21, 1, 0, 0)], 2, 10)))
    # start % 16 in {0, 1, 15} against T % 16 in {0, 1, 15}; start = 1 as L = 1 (the only state that is not logzero) and L = 2
    starts, Ts = (16, 1, 31), (48, 49, 63)
    for i in range(3):
        W = 10 if i != 1 else 5
        rows = []
        for j, start in enumerate(starts):
            has = (i + j) % 2
            L = start + 1 if start > 1 else (2 if has else 1)
            rows.append((1, Ts[(i + j) % 3], L, _nh(W, i + j), has, 0))
        rows.append((1, 12 + i, 3, _nh(W, i), i % 2, 0))         # ... and one the sequential kernel walks: 10 + i frames
        out.append(CaseSpec(f"par_edges{i}", 1024, W, 520, 16, _with_inactive(rows, (i + 3) % 4, W)))
    # T - base = 17 (thirty empty segments), 512 (16-frame segments, all full), 513 (32-frame segments)
    out.append(CaseSpec("par_base17_512_513", 1024, 10, 600, 16,
                        _with_inactive([(1, 17, 2, 10, 1, 0), (1, 544, 41, 7, 1, 0), (1, 513, 1, 1, 0, 0), (1, 30, 20, 7, 0, 0)], 1, 10)))
    # nh K no multiple of the 8 pairs of a workgroup: K = V = 37
    out.append(CaseSpec("par_V37_beam10", 37, 10, 520, 16,
                        _with_inactive([(1, 60, 3, 7, 1, 0), (1, 50, 1, 1, 0, 0), (1, 19, 5, 10, 1, 0)], 0, 10)))
    out.append(CaseSpec("par_V37_beam5", 37, 5, 520, 16,
                        _with_inactive([(1, 49, 17, 5, 0, 0), (1, 48, 2, 2, 1, 0), (1, 18, 4, 1, 1, 0)], 3, 5)))
    return out


CASES = {c.name: c for c in _case_table()}


def max_tokens(max_frames):
    return max_frames + 16           # L - 1 = T + 4 at any T fits


def cfg_name(V):
    """registers the tiny model at vocabulary V in test_engine_spec.CFGS"""
    import test_engine_spec
    from speechcatcher_amd.config import TINY
    if V == 1024:
        return "TINY"
    test_engine_spec.CFGS.setdefault(f"TINY_V{V}", dataclasses.replace(TINY, vocab_size=V))
    return f"TINY_V{V}"


def batch_kwargs(S, max_frames):
    return dict(n_streams=S, max_frames=max_frames, max_tokens=max_tokens(max_frames), pcm_capacity=1 << 12)


@functools.lru_cache(maxsize=None)
def spec_batch(V, W, S, max_frames):
    from oracle.kernel_spec import SpecBackend
    from test_engine_spec import make_batch
    return make_batch(cfg_name(V), 1234, "meanstd", W, False, backend=SpecBackend(), **batch_kwargs(S, max_frames))


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference
def lse64(a, b):
    return np.maximum(a, b) + np.log1p(np.exp(-np.abs(a - b)))


def _live_abs(v):
    """|v| where v is a number, 0 where it is logzero"""
    return np.where(v > LIVE, np.abs(v), 0.0)


def reference_stream(x, ids, last, L, has, r_prev, blank, eos):
    """x [T][V] float64; ids [nh][K]; last [nh]; r_prev [T][2][nh] (has).  Returns psi [nh][K], psi_eos [nh], r [T][2][nh][K],
    rs [T][nh][K] and the magnitudes A of the module docstring: A_psi, A_eos, A_r [T][nh][K], A_rs."""
    T = x.shape[0]
    nh, K = ids.shape
    xb = x[:, blank]
    if has:
        pn, pb = r_prev[:, 0], r_prev[:, 1]
        r_sum = lse64(pn, pb)                                    # [T][nh]
        A_eos = 1.0 + _live_abs(r_sum[T - 1])
    else:
        cum = np.zeros(T)
        acc = 0.0
        for t in range(T):
            acc += xb[t]
            cum[t] = acc
        pb = np.repeat(cum[:, None], nh, 1)
        r_sum = pb
        A_eos = np.full(nh, float((1.0 + np.abs(cum)).sum()))
    same = ids == last[:, None]
    out_len = L - 1
    start = min(max(out_len, 1), T)
    r = np.full((T, 2, nh, K), LOGZERO)
    if out_len == 0:
        r[0, 0] = x[0][ids]
    A_r = np.ones((T, nh, K))
    acc = 1.0 + _live_abs(r[start - 1, 0])
    A_r[start - 1] = acc
    terms, A_terms = [r[start - 1, 0]], [_live_abs(r[start - 1, 0])]
    # what phi[t] itself carries: one rounding of the stored sum, or the fp32 blank sum over the frames <= t
    A_phi = _live_abs(r_sum) if has else np.repeat(np.cumsum(1.0 + np.abs(cum))[:, None], nh, 1)
    for t in range(start, T):
        phi = np.where(same, pb[t - 1][:, None], r_sum[t - 1][:, None])
        xc = x[t][ids]
        r[t, 0] = lse64(r[t - 1, 0], phi) + xc
        r[t, 1] = lse64(r[t - 1, 0], r[t - 1, 1]) + xb[t]
        terms.append(phi + xc)
        A_terms.append(1.0 + _live_abs(phi + xc) + A_phi[t - 1][:, None])
        acc = acc + 1.0 + np.maximum(np.maximum(_live_abs(r[t, 0]), _live_abs(r[t, 1])), _live_abs(phi + xc))
        A_r[t] = acc
    terms = np.stack(terms)
    m = terms.max(0)
    w = np.exp(terms - m)
    psi = m + np.log(w.sum(0))
    A_psi = 1.0 + _live_abs(psi) + (w * np.stack(A_terms)).sum(0) / w.sum(0)
    is_eos, is_blank = ids == eos, ids == blank
    psi = np.where(is_eos, r_sum[T - 1][:, None], psi)
    A_psi = np.where(is_eos, A_eos[:, None], A_psi)
    psi = np.where(is_blank, LOGZERO, psi)
    rs = lse64(r[:, 0], r[:, 1])
    return dict(psi=psi, psi_eos=r_sum[T - 1].copy(), r=r, rs=rs, A_psi=A_psi, A_eos=A_eos, A_r=A_r,
                A_rs=A_r + 1.0 + _live_abs(rs), same=same)


def expected_live(st, same, ids, blank, eos):
    """Which outputs are numbers and which logzero, from the lengths alone.  A prefix of n tokens cannot end before frame
    n - 1, and not in a blank before frame n; a candidate that repeats the last token needs a blank in between, one frame
    more, when the previous prefix has a state (without one, phi is the blank sum whatever the candidate).  With
    fn = the first frame at which r^n of the extended prefix is a number (0 for L = 1, else L - 1, + 1 for a repeat):
    r^n[t] is a number from fn on, r^b[t] from fn + 1 on, psi if fn < T; the eos score is r_sum[T-1] of the previous prefix,
    a number if T >= L - 1 (always without a state)."""
    T, L, has = st.Te, st.L, bool(st.has)
    fn = np.zeros(same.shape, np.int64) if L == 1 else (L - 1) + (same & has).astype(np.int64)
    t = np.arange(T)[:, None, None]
    r = np.stack([np.broadcast_to(t >= fn, (T,) + same.shape), np.broadcast_to(t >= fn + 1, (T,) + same.shape)], 1)
    eos_live = (not has) or L == 1 or T >= L - 1
    psi = np.where(ids == eos, eos_live, fn < T) & (ids != blank)
    return dict(psi=psi, psi_eos=np.full(same.shape[0], eos_live), r=r, rs=r[:, 0] | r[:, 1])


# ---------------------------------------------------------------------------------------------------------------------
# numpy float32 transcriptions: every intermediate is rounded to float32
def lse2_f32(a, b):
    """max + log(1 + exp(-|a - b|)), the kernels' lse2"""
    return np.maximum(a, b) + np.log(F32(1.0) + np.exp(-np.abs(a - b)))


def _psi_add_f32(pm, ps, v):
    """the kernels' running log-sum-exp: maximum so far and the sum scaled by it, plus one term"""
    d = v - pm
    e = np.exp(-np.abs(d))
    return np.maximum(pm, v), np.where(d > 0, ps * e + F32(1.0), ps + e)


def _frame_f32(rn, rb, prs, pb, same, xc, xb):
    phi = np.where(same, pb, prs)
    return lse2_f32(rn, phi) + xc, lse2_f32(rn, rb) + xb, phi


PLANTS = ("phi_frame", "skip_first", "prs_for_same", "cum_short", "walk_from_base")


def segment_affine_f32(x, ids, last, L, has, r_prev, rs_prev, blank, eos, plant=None):
    """The segment-affine form in float32: per segment the coefficients A, C, D, Un, Ub of
    n_end = A n0 + Un, b_end = C n0 + D b0 + Ub (log domain) and the segment's share of psi, a 32-step combine that gives every
    segment its start state, and the walk of every segment from its start state with the sequential recurrence (the rebuild).
    x [T][V], r_prev [T][2][nh], rs_prev [T][nh]: float32.  Returns psi, psi_eos, r [T][2][nh][K], rs, seg_state [32][2][nh][K].
    plant: one of PLANTS - a deliberate mistake, for the sensitivity test:
      phi_frame       phi of frame t instead of t - 1 at the first frame of a segment
      skip_first      the first frame of a non-empty segment left out
      prs_for_same    r^n (+) r^b of the prefix where its r^b belongs (a candidate that repeats the last token)
      cum_short       the blank sum in front of a segment one frame short (no state)
      walk_from_base  the frames [base, start) walked as well"""
    T = x.shape[0]
    nh, K = ids.shape
    LZ = F32(LOGZERO)
    st = Stream(1, T, L, nh, int(has))
    start, segs = st.start, st.segments()
    same = ids == last[:, None]
    xb = x[:, blank]
    cumseq = np.concatenate([[F32(0.0)], np.cumsum(xb, dtype=F32)])      # cumseq[t] = sum of the frames < t, in order
    where = next((p for p in range(1, NSEG) if segs[p][0] < segs[p][1]), 0)    # the segment a plant goes to

    def prefix(t):                   # (r^n (+) r^b, r^b) of the previous prefix at frame t, [nh][1]
        if has:
            t = min(max(t, 0), T - 1)
            return rs_prev[t][:, None], r_prev[t, 1][:, None]
        return None

    # blank sums in front of the segments (no state)
    bs = np.zeros(NSEG, F32)
    if not has:
        for p, (lo, hi) in enumerate(segs):
            acc = cumseq[start] if p == 0 else F32(0.0)
            if plant == "cum_short" and p == where - 1:
                hi -= 1
            for t in range(lo, hi):
                acc = F32(acc + xb[t])
            bs[p] = acc
    cum0 = np.zeros(NSEG, F32)
    for p in range(1, NSEG):
        cum0[p] = F32(cum0[p - 1] + bs[p - 1])
    cum0[0] = cumseq[start]
    # pass 1: coefficients and psi shares
    shape = (nh, K)
    co = []
    for p, (lo, hi) in enumerate(segs):
        if plant == "walk_from_base" and p == 0:
            lo = start & ~15
        if plant == "skip_first" and p == where:
            lo += 1
        A, D = np.zeros(shape, F32), np.zeros(shape, F32)
        C, Un, Ub, pm = (np.full(shape, LZ) for _ in range(4))
        ps = np.zeros(shape, F32)
        cu = cum0[p]
        for t in range(lo, hi):
            xc, xbt = x[t][ids], xb[t]
            late = plant == "phi_frame" and p == where and t == lo
            if has:
                prs, pb = prefix(t if late else t - 1)
            else:
                prs = pb = np.full(shape, F32(cu + xbt) if late else cu)
            if plant == "prs_for_same":
                pb = prs
            phi = np.where(same, pb, prs)
            nUb = lse2_f32(Un, Ub) + xbt
            nC = lse2_f32(A, C) + xbt
            Un = lse2_f32(Un, phi) + xc
            Ub, C = nUb, nC
            A = A + xc
            D = D + xbt
            pm, ps = _psi_add_f32(pm, ps, phi + xc)
            if not has:
                cu = F32(cu + xbt)
        co.append((A, C, D, Un, Ub, pm, ps))
    # combine
    n = x[0][ids].astype(F32) if L == 1 else np.full(shape, LZ)
    b = np.full(shape, LZ)
    gm, gs = n.copy(), np.ones(shape, F32)
    seg_state = np.empty((NSEG, 2) + shape, F32)
    for q, (A, C, D, Un, Ub, pm, ps) in enumerate(co):
        seg_state[q, 0], seg_state[q, 1] = n, b
        n, b = lse2_f32(A + n, Un), lse2_f32(lse2_f32(C + n, D + b), Ub)
        m = np.maximum(gm, pm)
        gs = gs * np.exp(gm - m) + ps * np.exp(pm - m)
        gm = m
    psi = gm + np.log(gs)
    total = F32(0.0)
    for p in range(NSEG):
        total = F32(total + bs[p])
    rsum_last = rs_prev[T - 1] if has else np.full(nh, total)
    psi = np.where(ids == eos, rsum_last[:, None], psi)
    psi = np.where(ids == blank, LZ, psi).astype(F32)
    # the rebuild: every segment from its start state
    r = np.full((T, 2) + shape, LZ)
    r[start - 1, 0] = seg_state[0, 0]
    for p, (lo, hi) in enumerate(segs):
        rn, rb = seg_state[p, 0], seg_state[p, 1]
        for t in range(lo, hi):
            prs, pb = prefix(t - 1) if has else (np.full(shape, cumseq[t]),) * 2
            rn, rb, _ = _frame_f32(rn, rb, prs, pb, same, x[t][ids], xb[t])
            r[t, 0], r[t, 1] = rn, rb
    assert psi.dtype == F32 and r.dtype == F32 and seg_state.dtype == F32
    return dict(psi=psi, psi_eos=np.asarray(rsum_last, F32), r=r, rs=lse2_f32(r[:, 0], r[:, 1]), seg_state=seg_state)


# ---------------------------------------------------------------------------------------------------------------------
def kappa(got, ref, A):
    """(kappa, masks equal): kappa over the entries whose reference is a number; inf if a result there is not finite"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    live = ref > LIVE
    same_mask = bool(np.array_equal(live, got > LIVE))        # (NaN > LIVE is False: a NaN where a number belongs shows here)
    if not live.any():
        return 0.0, same_mask
    g = got[live]
    if not np.isfinite(g).all():
        return float("inf"), same_mask
    return float((np.abs(g - ref[live]) / (EPS * np.broadcast_to(A, ref.shape)[live])).max()), same_mask


class Case:
    """One launch: the buffers of every stream, the float64 reference of every output with its A, and the winners."""

    def __init__(self, spec, seed=0):
        self.spec, self.name = spec, spec.name
        self.V, self.W, self.TCAP, self.split_min = spec.V, spec.W, spec.max_frames, spec.split_min
        self.K, self.LCAP = min(40, self.V), max_tokens(spec.max_frames)
        self.blank, self.eos = 0, self.V - 1
        self.tct = (self.TCAP + 3) // 4 * 4
        self.tck = (self.TCAP + CK - 1) // CK
        self.streams = [Stream(*row, cur=i % 2) for i, row in enumerate(spec.streams)]
        self.S = len(self.streams)
        names = sorted(CASES)
        self.rng = np.random.default_rng([seed, names.index(spec.name) if spec.name in CASES else len(names)])
        self.data = [self._build(st) for st in self.streams]
        self.live = [s for s, st in enumerate(self.streams) if st.active]

    def split(self, s, split_min=None):
        return is_split(self.streams[s], self.TCAP, self.split_min if split_min is None else split_min)

    # -- the buffers of one stream
    def _build(self, st):
        rng, V, W, K, TCAP, LCAP = self.rng, self.V, self.W, self.K, self.TCAP, self.LCAP
        nan = lambda *shape: np.full(shape, np.nan, F32)   # noqa: E731
        d = dict(x=nan(TCAP, V), ids=np.full((W, K), V, np.int32), yseq=np.full((2, W, LCAP), V + 5, np.int32),
                 r=nan(2, TCAP, 2, W), rs=nan(2, TCAP, W), sel=np.zeros((W, 2), np.int32))
        d["r"][1 - st.cur], d["rs"][1 - st.cur] = SENTINEL, SENTINEL
        if not st.active:
            return d
        T, L, nh, cur = st.Te, st.L, st.nh, st.cur
        z = 2.0 * rng.standard_normal((TCAP, V))
        z = z - z.max(1, keepdims=True)
        x = (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(F32)
        x[24:] = (2.0 * rng.standard_normal((TCAP - 24, V)) - 4.0).astype(F32)      # later rows are raw logits
        d["x"][:T] = x[:T]
        x64 = x[:T].astype(np.float64)
        last = np.zeros(nh, np.int64)
        for h in range(nh):
            mid = rng.permutation(np.arange(1, V - 1))
            ids = np.concatenate([mid[:K - 2], [self.eos, self.blank]])
            rng.shuffle(ids)
            d["ids"][h] = ids
            y = rng.integers(1, V - 1, L)
            y[0] = self.eos                                      # sos
            if L > 1:
                y[L - 1] = mid[int(rng.integers(0, K - 2))]      # the last token is one of the candidates
            d["yseq"][cur, h, :L] = y
            last[h] = y[L - 1]
        r_prev = None
        if st.has:
            # the state the previous step left: the prefix without its last token, extended by that token, from the state of a
            # prefix that has none (L = 1: that state itself)
            xb_cum = np.cumsum(x64[:, self.blank])
            r_prev = np.full((T, 2, nh), LOGZERO)
            r_prev[:, 1] = xb_cum[:, None]
            if L > 1:
                prev_last = d["yseq"][cur, :nh, L - 2].astype(np.int64)
                r_prev = reference_stream(x64, last[:, None], prev_last, L - 1, False, None, self.blank, self.eos)["r"][..., 0]
            r32 = r_prev.astype(F32)
            d["r"][cur, :T, :, :nh] = r32
            r_prev = r32.astype(np.float64)
            d["rs"][cur, :T, :nh] = lse64(r_prev[:, 0], r_prev[:, 1]).astype(F32)
        ref = reference_stream(x64, d["ids"][:nh].astype(np.int64), last, L, bool(st.has), r_prev, self.blank, self.eos)
        d.update(ref=ref, last=last)
        # the winners: any pair of a live hypothesis; two that share a parent, two that are the same pair
        sel = np.stack([rng.integers(0, nh, W), rng.integers(0, K, W)], 1)
        sel[1] = (sel[0, 0], (sel[0, 1] + 1 + rng.integers(0, K - 1)) % K)
        sel[3] = sel[2]
        d["sel"] = sel.astype(np.int32)
        return d

    # -- writing streams into a batch: slots = [(slot of the batch, stream of the case)]
    def apply(self, sb, slots=None):
        slots = [(s, s) for s in range(self.S)] if slots is None else slots
        assert sb.S == len(slots) and sb.TCAP == self.TCAP and sb.W == self.W and sb.K == self.K and sb.LCAP == self.LCAP
        assert sb.ctcxT.shape[-1] == self.tct and sb.ctc_rnew.shape[1] == self.tck
        dev = sb.ctrl.device
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        W, V = self.W, self.V
        sb.ctrl.copy_(t(np.array([self.streams[s].ctrl for _, s in slots], np.int32)))
        xT = sb.ctcxT.view(sb.S, V, self.tct)
        xT.fill_(float("nan"))
        for slot, s in slots:
            d = self.data[s]
            x = t(d["x"])
            sb.ctcx.view(sb.S, self.TCAP, V)[slot].copy_(x)
            xT[slot, :, :self.TCAP].copy_(x.t())
            sb.pre_ids[slot * W:(slot + 1) * W].copy_(t(d["ids"]))
            sb.yseq[:, slot].copy_(t(d["yseq"]))
            sb.ctc_r[:, slot].copy_(t(d["r"]))
            sb.ctc_rs[:, slot].copy_(t(d["rs"]))
            sb.sel[slot].copy_(t(d["sel"]))
        for name in ("psi", "psi_eos", "ctc_rnew"):
            getattr(sb, name).fill_(SENTINEL)
        sb._rnew_full = None

    # -- reading the outputs of one stream
    def collect(self, sb, slot, s):
        st, W, K = self.streams[s], self.W, self.K
        o = 1 - st.cur
        n = lambda a: a.detach().cpu().numpy()   # noqa: E731
        return dict(psi=n(sb.psi[slot * W:(slot + 1) * W]), psi_eos=n(sb.psi_eos[slot * W:(slot + 1) * W]),
                    rnew=n(sb.ctc_rnew[slot]), r=n(sb.ctc_r[o, slot]), rs=n(sb.ctc_rs[o, slot]),
                    r_cur=n(sb.ctc_r[st.cur, slot]), rs_cur=n(sb.ctc_rs[st.cur, slot]))

    def rnew_frames(self, s, split):
        """the frame whose state row j of the stream's ctc_rnew holds, for the rows the scan writes"""
        st = self.streams[s]
        if split:
            return [min(lo, st.Te) - 1 for lo, _ in st.segments()]
        return [CK * j + CK - 1 for j in range(st.Te // CK)]

    def kappas(self, out, s, split, winners_only=True):
        """kappa and mask agreement per output of stream s.  out: psi [nh..][K], psi_eos, and either the rebuilt r [T..][2][W],
        rs [T..][W] of the winners (winners_only) or r [T][2][nh][K], rs [T][nh][K] of all pairs; rnew [rows][2][nh K ..]"""
        st, d = self.streams[s], self.data[s]
        ref, T, nh, K = d["ref"], st.Te, st.nh, self.K
        res = {}
        # (the eos candidate's psi is the eos score: it goes with psi_eos, whose A is that of one stored sum - in one group with
        # the walked candidates it would set their kappa_ref)
        is_eos = d["ids"][:nh] == self.eos
        res["psi"] = kappa(np.where(is_eos, LOGZERO, out["psi"][:nh]), np.where(is_eos, LOGZERO, ref["psi"]), ref["A_psi"])
        res["psi_eos"] = kappa(np.concatenate([out["psi_eos"][:nh], out["psi"][:nh][is_eos]]),
                               np.concatenate([ref["psi_eos"], ref["psi"][is_eos]]),
                               np.concatenate([ref["A_eos"], ref["A_psi"][is_eos]]))
        if winners_only:
            h, k = d["sel"][:, 0], d["sel"][:, 1]
            r_ref, rs_ref, A_r, A_rs = ref["r"][:, :, h, k], ref["rs"][:, h, k], ref["A_r"][:, h, k], ref["A_rs"][:, h, k]
        else:
            r_ref, rs_ref, A_r, A_rs = ref["r"], ref["rs"], ref["A_r"], ref["A_rs"]
        res["r"] = kappa(out["r"][:T], r_ref, A_r[:, None])
        res["rs"] = kappa(out["rs"][:T], rs_ref, A_rs)
        if "rnew" in out:
            fr = self.rnew_frames(s, split)
            got = out["rnew"][:len(fr), :, :nh * K].reshape(len(fr), 2, nh, K)
            res["rnew"] = kappa(got, ref["r"][fr], ref["A_r"][fr][:, None]) if fr else (0.0, True)
        return res


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(CASES[name])


def _merge(into, res):
    for n, (k, ok) in res.items():
        k0, ok0 = into.get(n, (0.0, True))
        into[n] = (max(k0, k), ok0 and ok)


def spec_results(c):
    """the fp32 torch spec on the case: per live stream psi, psi_eos, r and rs of ALL pairs, the checkpoints it stores and what
    its rebuild hands the winners"""
    from oracle.kernel_spec import SpecBackend
    sc = spec_batch(c.V, c.W, c.S, c.TCAP)
    c.apply(sc)
    be = SpecBackend()
    be.ctc_prefix_scan(sc)
    be.ctc_gather_state(sc)
    out = {}
    for s in c.live:
        st = c.streams[s]
        o = c.collect(sc, s, s)
        full = sc._rnew_full[s].numpy().reshape(st.Te, 2, st.nh, c.K)
        o["r_full"], o["rs_full"] = full, torch.logsumexp(sc._rnew_full[s], 1).numpy().reshape(st.Te, st.nh, c.K)
        out[s] = o
    return out


def affine_results(c, s, plant=None):
    st, d = c.streams[s], c.data[s]
    T, nh, cur = st.Te, st.nh, st.cur
    return segment_affine_f32(d["x"][:T], d["ids"][:nh].astype(np.int64), d["last"], st.L, bool(st.has),
                              d["r"][cur, :T, :, :nh], d["rs"][cur, :T, :nh], c.blank, c.eos, plant)


def affine_kappas(c, plant=None):
    """kappa per output of the float32 segment-affine transcription over the live streams of the case (max, masks and-ed)"""
    res = {}
    for s in c.live:
        a = affine_results(c, s, plant)
        out = dict(psi=a["psi"], psi_eos=a["psi_eos"], r=a["r"], rs=a["rs"], rnew=a["seg_state"].reshape(NSEG, 2, -1))
        _merge(res, c.kappas(out, s, True, winners_only=False))
    return res


def spec_kappas(c):
    """kappa per output of the fp32 torch spec: all pairs, the checkpoints, and the winners' rebuilt rows"""
    res = {}
    for s, o in spec_results(c).items():
        _merge(res, c.kappas(dict(psi=o["psi"], psi_eos=o["psi_eos"], r=o["r_full"], rs=o["rs_full"], rnew=o["rnew"]), s, False,
                             winners_only=False))
        _merge(res, {n: v for n, v in c.kappas(dict(psi=o["psi"], psi_eos=o["psi_eos"], r=o["r"], rs=o["rs"]), s, False).items()
                     if n in ("r", "rs")})
    return res


@functools.lru_cache(maxsize=None)
def kappa_ref(name):
    """per output: the larger of the spec's kappa and the float32 transcription's; both on the CPU"""
    c = case(name)
    ks, ka = spec_kappas(c), affine_kappas(c)
    assert all(ok for _, ok in ks.values()) and all(ok for _, ok in ka.values()), (name, ks, ka)
    return {n: max(ks[n][0], ka[n][0]) for n in OUTPUTS}, {n: ks[n][0] for n in OUTPUTS}, {n: ka[n][0] for n in OUTPUTS}

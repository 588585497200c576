"""Float64 references of what every frame passes before the first matrix kernel - the log-mel front-end (sc_logmel),
conv1 (sc_conv1), block assembly (sc_block_pack) - and of the contextual encoder layer with its context hand-off
(sc_encoder_layers), in plain numpy and written independently of csrc/encoder.hip, together with the error models the
tests hold fp32 implementations to.  No GPU and no oracle import in here: the test inputs (signals, job tables) and the
thin drivers at the end take the backend under test as an argument.

Log-mel error model.  For one frame with windowed samples x_w, float64 spectrum X and float64 mel power M64 = sum_k
fb[k, m] |X_k|^2, an fp32 transform returns X_k + e_k with |e_k| <= delta = kappa * 2^-24 * ||x_w||_2 (every butterfly
stage is an orthogonal map times sqrt 2: rounding errors are carried at the scale of the frame's energy, not of the bin),
so the mel power is off by at most

    bound[m] = sum_k fb[k, m] (2 |X_k| delta + delta^2)  +  4 * 2^-24 * M64[m]

(the second term: squaring, the fma chain of the mel product), and carried through log and the MVN

    tol = (bound / max(M64, 1e-10) + 4 * 2^-24 |log|) / std  +  2 * 2^-24 |v|.

kappa is the one free number: `kappa_needed` returns the smallest kappa at which a given output holds the bound.
"""
import copy
import functools
import math
import types

import numpy as np

U = 2.0 ** -24          # unit roundoff of float32
CLAMP = 1e-10
SAMPLE_RATE = 16000
SIG_LEN = 4000

# (n_fft, win, hop, n_mels): the model's; the smallest n_fft (no window offset); the largest (more mel bins than threads)
GEOMS = {"model": (512, 400, 160, 80), "small": (64, 64, 16, 8), "large": (2048, 1200, 480, 300)}


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def signals():
    """name -> float32 [SIG_LEN]; fixed seeds, the same on every machine"""
    n = SIG_LEN
    t = np.arange(n, dtype=np.float64) / SAMPLE_RATE

    def noise(seed, sigma, m=n):
        return sigma * np.random.RandomState(seed).randn(m)

    sine = 0.9 * np.sin(2 * np.pi * 1000.0 * t)
    impulse = np.zeros(n)
    impulse[2000] = 1.0
    am = (0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t)) * np.sin(2 * np.pi * 180.0 * t)
    speech = np.clip(np.round(am * 32768.0), -32768, 32767) / 32768.0
    speech[2001], speech[2002] = -1.0, 32767.0 / 32768.0
    out = {
        "noise": noise(1, 0.1),
        "zeros": np.zeros(n),
        "noise_1e-6": noise(2, 1e-6),
        "noise_1e-5": noise(3, 1e-5),
        "sine": sine,
        "sine_noise": sine + noise(4, 1e-4),
        "dc": 0.5 + noise(5, 1e-3),
        "square": np.where(np.sin(2 * np.pi * 440.0 * t) >= 0, 1.0, -1.0),
        "nyquist": np.where(np.arange(n) % 2 == 0, 1.0, -1.0),
        "impulse": impulse,
        "speech_int16": speech,
        "silence_then_noise": np.concatenate([np.zeros(n // 2), noise(7, 0.3, n - n // 2)]),
    }
    return {k: v.astype(np.float32) for k, v in out.items()}


def frontend_tables(geom):
    """the tables sc_logmel takes for GEOMS[geom], built by speechcatcher_amd.mel: (cfg, window, mel_fb, twiddle) as
    a namespace of float32 torch CPU tensors"""
    import torch
    from speechcatcher_amd import mel
    n_fft, win, hop, n_mels = GEOMS[geom]
    cfg = types.SimpleNamespace(n_fft=n_fft, win_length=win, hop_length=hop, n_mels=n_mels, sample_rate=SAMPLE_RATE)
    return types.SimpleNamespace(
        cfg=cfg, window=mel.hann_window_periodic(win).contiguous(),
        mel_fb=mel.melscale_fbanks_slaney(n_fft // 2 + 1, 0.0, SAMPLE_RATE / 2.0, n_mels, SAMPLE_RATE),
        twiddle=torch.from_numpy(mel.fft_twiddles(n_fft)))


def mvn_stats(n_mels, mode):
    """(mean, std) of MVN mode 1 (float32 statistics) or 2 (float64); mode 0: (zeros, ones), not applied"""
    rng = np.random.RandomState(99)
    mean = -8.0 + rng.randn(n_mels)
    std = 2.0 + 0.5 * rng.rand(n_mels)
    if mode == 0:
        return np.zeros(n_mels), np.ones(n_mels)
    if mode == 1:
        return mean.astype(np.float32), std.astype(np.float32)
    return mean, std


def frontend_namespace(geom, mode, device="cpu"):
    """what HipBackend.logmel / SpecBackend.logmel read from the weights object, for GEOMS[geom] and an MVN mode"""
    import torch
    t = frontend_tables(geom)
    mean, std = mvn_stats(t.cfg.n_mels, mode)
    return types.SimpleNamespace(
        cfg=t.cfg, window=t.window.to(device), mel_fb=t.mel_fb.to(device), twiddle=t.twiddle.to(device),
        has_mvn=mode != 0, mvn_is_f64=mode == 2,
        mean64=torch.from_numpy(np.asarray(mean, np.float64)).to(device),
        std64=torch.from_numpy(np.asarray(std, np.float64)).to(device))


def logmel_case(geom, x):
    """The job table of one launch over slices of the signal x: -> namespace(pcm [S][stride] float32, NaN outside every
    stream's [seg_start, seg_start + seg_len); jobs int32 [n][8] = (s, seg_start, seg_len, eff_len, lo, n, dst0, 0);
    max_keep; n_rows of featbuf, with unwritten rows in front of, between and behind the jobs)."""
    n_fft, win, hop, _ = GEOMS[geom]
    n = len(x)
    full = 1 + n // hop
    lo5 = 3 if 2000 // hop >= 7 else 1
    # (stream, seg_start, source slice, eff_len, lo, keep_n)
    plan = [
        (0, 0, (0, n), n, 0, full),                              # final segment, seg_len = eff_len: right-hand reflection
        (1, 300, (500, 3500), 3000, 2, 1),                       # keep_n = 1 beside keep_n = max_keep; trimmed head
        (2, 0, (2000, 2001), win, 0, 1 + win // hop),            # final short segments, zero-padded to eff_len = win
        (3, 5, (2000, 2000 + hop - 1), win, 0, 1 + win // hop),
        (4, 0, (2000, 2000 + win), win, 1, win // hop),
        (5, 137, (1500, 3500), 2000, lo5, min(5, 1 + 2000 // hop - lo5)),   # seg_start > 0, lo > 0
    ]
    stride = n + 600
    pcm = np.full((len(plan), stride), np.nan, np.float32)
    jobs = np.zeros((len(plan), 8), np.int32)
    row = 2
    for j, (s, start, (a, b), eff, lo, keep) in enumerate(plan):
        assert lo + keep <= 1 + eff // hop and eff > n_fft // 2 and b - a <= eff
        pcm[s, start:start + b - a] = x[a:b]
        jobs[j] = (s, start, b - a, eff, lo, keep, row, 0)
        row += keep + 3
    return types.SimpleNamespace(pcm=pcm, stride=stride, jobs=jobs, max_keep=int(jobs[:, 5].max()), n_rows=row)


# ---------------------------------------------------------------------------------------------------------------------
# sc_logmel in float64
# ---------------------------------------------------------------------------------------------------------------------
def frames_f64(seg, eff_len, lo, n, n_fft, win, hop, window):
    """zero-pad the segment to eff_len, reflect-pad by n_fft / 2, frames lo .. lo + n at `hop`, times the periodic
    Hann(win) centred in n_fft: float64 [n][n_fft]"""
    x = np.zeros(eff_len)
    x[:len(seg)] = np.asarray(seg, np.float64)
    padded = np.pad(x, n_fft // 2, mode="reflect")
    w = np.zeros(n_fft)
    off = (n_fft - win) // 2
    w[off:off + win] = np.asarray(window, np.float64)
    idx = (lo + np.arange(n))[:, None] * hop + np.arange(n_fft)[None, :]
    return padded[idx] * w[None, :]


class LogmelRef:
    """float64 log-mel rows of one job table plus the pieces of the error model (module docstring)"""

    def __init__(self, rows, M, A, B):
        self.rows, self.M, self.A, self.B = rows, M, A, B      # rows: featbuf row of every reference row
        self.lg = np.log(np.maximum(M, CLAMP))

    def value(self, mode, mean, std):
        if mode == 0:
            return self.lg
        return (self.lg - np.asarray(mean, np.float64)[None, :]) / np.asarray(std, np.float64)[None, :]

    def tol(self, kappa, mode, mean, std):
        s = np.ones_like(self.lg) if mode == 0 else np.broadcast_to(np.asarray(std, np.float64)[None, :], self.lg.shape)
        bound = kappa * self.A + kappa * kappa * self.B + 4 * U * self.M
        return (bound / np.maximum(self.M, CLAMP) + 4 * U * np.abs(self.lg)) / s + 2 * U * np.abs(self.value(mode, mean, std))

    def kappa_needed(self, out, mode, mean, std):
        """the smallest kappa >= 0 at which every element of `out` (rows as self.rows) holds the bound; inf where no
        kappa can help (a frame without energy that is not at the clamp, or a non-finite output)"""
        s = np.ones_like(self.lg) if mode == 0 else np.broadcast_to(np.asarray(std, np.float64)[None, :], self.lg.shape)
        v = self.value(mode, mean, std)
        err = np.abs(np.asarray(out, np.float64) - v)
        fixed = 4 * U * np.abs(self.lg) / s + 2 * U * np.abs(v)
        # need kappa A + kappa^2 B >= E
        E = (err - fixed) * s * np.maximum(self.M, CLAMP) - 4 * U * self.M
        k = np.zeros_like(E)
        pos = E > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            quad = (-self.A + np.sqrt(self.A * self.A + 4 * self.B * E)) / (2 * self.B)
        k[pos] = np.where(self.B[pos] > 0, quad[pos], np.inf)
        k[~np.isfinite(err)] = np.inf
        return float(k.max()) if k.size else 0.0


def logmel_ref(pcm, jobs, geom, window, mel_fb):
    """-> LogmelRef of the job table (all jobs, rows in table order); pcm [S][stride] float32"""
    n_fft, win, hop, _ = GEOMS[geom] if isinstance(geom, str) else geom
    fb = np.asarray(mel_fb, np.float64)
    rows, Ms, As, Bs = [], [], [], []
    for s, start, seg_len, eff, lo, n, dst0, _ in np.asarray(jobs).tolist():
        xw = frames_f64(pcm[s, start:start + seg_len], eff, lo, n, n_fft, win, hop, window)
        absX = np.abs(np.fft.rfft(xw, axis=1))
        nrm = U * np.sqrt((xw * xw).sum(axis=1))[:, None]
        Ms.append((absX * absX) @ fb)
        As.append(((2.0 * absX) @ fb) * nrm)
        Bs.append(fb.sum(axis=0)[None, :] * nrm * nrm)
        rows.extend(range(dst0, dst0 + n))
    return LogmelRef(np.asarray(rows), np.concatenate(Ms), np.concatenate(As), np.concatenate(Bs))


@functools.lru_cache(maxsize=None)
def logmel_ref_of(geom, signal):
    """(case, LogmelRef) of one signal at one geometry: computed once, shared by every test, never modified"""
    t = frontend_tables(geom)
    case = logmel_case(geom, signals()[signal])
    return case, logmel_ref(case.pcm, case.jobs, geom, t.window.numpy(), t.mel_fb.numpy())


SENTINEL = -777.25


def run_logmel(logmel, ns, case, device="cpu"):
    """One launch of `logmel` (the bound method of a backend) over the case -> featbuf float32 numpy [n_rows][n_mels],
    pre-filled with SENTINEL"""
    import torch
    pcm = torch.from_numpy(case.pcm).to(device)
    jobs = torch.from_numpy(case.jobs).to(device)
    feat = torch.full((case.n_rows, ns.cfg.n_mels), SENTINEL, dtype=torch.float32, device=device)
    logmel(ns, pcm, case.stride, jobs, len(case.jobs), case.max_keep, feat)
    if str(device) != "cpu":
        torch.cuda.synchronize()
    return feat.cpu().numpy()


def untouched_rows_intact(feat, ref):
    """every featbuf row outside the jobs' [dst0, dst0 + n) still holds the pre-fill, byte for byte"""
    mask = np.ones(feat.shape[0], bool)
    mask[ref.rows] = False
    want = np.full((int(mask.sum()), feat.shape[1]), SENTINEL, np.float32)
    return feat[mask].tobytes() == want.tobytes()


_KAPPA_CACHE = {}


def measure_kappa(name, logmel, device="cpu", geoms=tuple(GEOMS), modes=(0, 1, 2), names=None):
    """-> {(geom, mode, signal): smallest kappa at which `logmel` holds the bound}, every signal and job of logmel_case;
    cached per `name` (None: not cached)"""
    key = (name, tuple(geoms), tuple(modes), names)
    if name is not None and key in _KAPPA_CACHE:
        return _KAPPA_CACHE[key]
    out = {}
    for geom in geoms:
        for mode in modes:
            ns = frontend_namespace(geom, mode, device)
            mean, std = mvn_stats(ns.cfg.n_mels, mode)
            for sig in names or signals():
                case, ref = logmel_ref_of(geom, sig)
                feat = run_logmel(logmel, ns, case, device)
                out[(geom, mode, sig)] = ref.kappa_needed(feat[ref.rows], mode, mean, std)
    if name is not None:
        _KAPPA_CACHE[key] = out
    return out


# ---------------------------------------------------------------------------------------------------------------------
# sc_conv1: Conv2d(1 -> d, 3x3, stride 2) + ReLU, channels-last
# ---------------------------------------------------------------------------------------------------------------------
def conv1_case(n_mels, d, seed=0):
    """Three jobs in one launch (T1 = 9, 3, 1; overlapping source rows; different r0), features like normalised log-mel
    and a bias that leaves about half the pre-activations negative.  jobs int32 [3][4] = (src0, t_in, r0, T1)."""
    rng = np.random.RandomState(1000 + 7 * n_mels + d + seed)
    F1 = (n_mels - 3) // 2 + 1
    feat = (-1.5 + 2.0 * rng.randn(24, n_mels)).astype(np.float32)
    w = ((rng.rand(d, 9) * 2 - 1) / 3.0).astype(np.float32)
    jobs = np.array([[0, 19, 5, 9], [4, 7, 1, 3], [10, 3, 20, 1]], np.int32)
    pre, _ = _conv1_sums(feat, w, np.zeros(d), jobs[0], F1)
    b = (-np.median(pre.reshape(-1, d), axis=0) + 0.01 * rng.randn(d)).astype(np.float32)
    return types.SimpleNamespace(feat=feat, w=w, b=b, jobs=jobs, max_t1=9, F1=F1, n_rows=24 * F1, n_mels=n_mels, d=d)


def _conv1_sums(feat, w, b, job, F1):
    src0, _, _, T1 = [int(v) for v in job]
    f = np.asarray(feat, np.float64)
    t = src0 + 2 * np.arange(T1)[:, None, None, None] + np.arange(3)[None, None, :, None]
    c = 2 * np.arange(F1)[None, :, None, None] + np.arange(3)[None, None, None, :]
    patch = f[t, c].reshape(T1, F1, 9)                                   # [T1][F1][kh*3 + kw]
    w64 = np.asarray(w, np.float64)
    pre = patch @ w64.T + np.asarray(b, np.float64)
    mag = np.abs(patch) @ np.abs(w64).T + np.abs(np.asarray(b, np.float64))
    return pre, mag


def conv1_ref(case):
    """-> (rows of c1 [n], relu(conv) float64 [n][d], tolerance [n][d] = 12 * 2^-24 (sum_q |x_q||w_q| + |b|): nine fused
    products and one add)"""
    rows, vals, tols = [], [], []
    for job in case.jobs:
        pre, mag = _conv1_sums(case.feat, case.w, case.b, job, case.F1)
        r0, T1 = int(job[2]), int(job[3])
        rows.append(((r0 + np.arange(T1))[:, None] * case.F1 + np.arange(case.F1)[None, :]).reshape(-1))
        vals.append(np.maximum(pre, 0.0).reshape(-1, case.d))
        tols.append(12 * U * mag.reshape(-1, case.d))
    return np.concatenate(rows), np.concatenate(vals), np.concatenate(tols)


def conv1_namespace(case, device="cpu"):
    import torch
    cfg = types.SimpleNamespace(n_mels=case.n_mels, d_model=case.d, conv_freq1=case.F1)
    return types.SimpleNamespace(cfg=cfg, conv1_w=torch.from_numpy(case.w).to(device), conv1_b=torch.from_numpy(case.b).to(device))


def run_conv1(conv1, case, device="cpu"):
    """-> c1 float32 numpy [n_rows][d], pre-filled with SENTINEL"""
    import torch
    ns = conv1_namespace(case, device)
    c1 = torch.full((case.n_rows, case.d), SENTINEL, dtype=torch.float32, device=device)
    conv1(ns, torch.from_numpy(case.feat).to(device), torch.from_numpy(case.jobs).to(device), len(case.jobs), case.max_t1, c1)
    if str(device) != "cpu":
        torch.cuda.synchronize()
    return c1.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# sc_block_pack: x * sqrt(d) + PE into (nb, R, d) blocks, context slot = mean
# ---------------------------------------------------------------------------------------------------------------------
BLOCK_PACK_LAUNCHES = {
    # name: (R, [(src0, clen, pe_f, pe_c, short)])
    "regular": (42, [(3, 1, 17, 93, 0), (0, 7, 0, 5, 0), (9, 40, 40, 199, 0)]),
    "short": (5, [(2, 5, 11, 0, 1), (30, 1, 57, 0, 1)]),
    "short_one_row": (1, [(4, 1, 3, 0, 1), (0, 1, 120, 0, 1)]),
}


def block_pack_case(name, d):
    from speechcatcher_amd import mel
    R, blocks = BLOCK_PACK_LAUNCHES[name]
    rng = np.random.RandomState(2000 + d)
    sub = (100.0 + rng.randn(64, d)).astype(np.float32)         # the mean is the hard part
    jobs = np.array([list(b) + [0] for b in blocks], np.int32)
    pe = mel.positional_encoding_table(200, d).numpy()
    return types.SimpleNamespace(sub=sub, jobs=jobs, R=R, nb=len(blocks), pe=pe, d=d, n_rows=len(blocks) * R + 2)


def block_pack_ref(case):
    """-> (value float64 [n_rows][d], tolerance [n_rows][d], written bool [n_rows]); value / tolerance 0 on the rows a
    regular block zeroes, rows with written False keep the pre-fill.  Body rows: 3 * 2^-24 (sqrt(d) |v| + |pe|) (a
    product, sqrt(d) itself, an add); context row: (clen + 4) * 2^-24 (sqrt(d) mean|v| + |pe|) (the clen - 1 adds of the
    sum, the division, then as a body row)."""
    d, R = case.d, case.R
    sq = math.sqrt(d)
    val = np.zeros((case.n_rows, d))
    tol = np.zeros((case.n_rows, d))
    written = np.zeros(case.n_rows, bool)
    pe = np.asarray(case.pe, np.float64)
    for b, (src0, clen, pe_f, pe_c, short, _) in enumerate(case.jobs.tolist()):
        v = np.asarray(case.sub[src0:src0 + clen], np.float64)
        body, body_tol = v * sq + pe[pe_f:pe_f + clen], 3 * U * (sq * np.abs(v) + np.abs(pe[pe_f:pe_f + clen]))
        r0 = b * R
        if short:
            val[r0:r0 + clen], tol[r0:r0 + clen], written[r0:r0 + clen] = body, body_tol, True
            continue
        written[r0:r0 + R] = True
        val[r0 + 1:r0 + 1 + clen], tol[r0 + 1:r0 + 1 + clen] = body, body_tol
        val[r0 + R - 1] = v.mean(axis=0) * sq + pe[pe_c]
        tol[r0 + R - 1] = (clen + 4) * U * (sq * np.abs(v).mean(axis=0) + np.abs(pe[pe_c]))
    return val, tol, written


def run_block_pack(block_pack, case, device="cpu"):
    """-> xblk float32 numpy [n_rows][d], pre-filled with SENTINEL"""
    import torch
    ns = types.SimpleNamespace(cfg=types.SimpleNamespace(d_model=case.d), pe=torch.from_numpy(case.pe).to(device))
    x = torch.full((case.n_rows, case.d), SENTINEL, dtype=torch.float32, device=device)
    block_pack(ns, torch.from_numpy(case.sub).to(device), torch.from_numpy(case.jobs).to(device), case.nb, case.R, x)
    if str(device) != "cpu":
        torch.cuda.synchronize()
    return x.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# context hand-off and the contextual encoder layer
# ---------------------------------------------------------------------------------------------------------------------
def chain_table(nblk, n_layers, flip=False):
    """Hand-off chains (b0, n_blocks, state row base = stream * n_layers, saved state valid) over `nblk` blocks, listed
    in non-ascending block order, with two blocks that belong to no chain; `flip` swaps valid and invalid.
    nblk = 12: chains of 5, 2, 1 and 1 blocks and a second chain of 1; nblk = 7: chains of 3, 1 and 1 blocks.
    -> (jobs int32 [ns][4], blocks outside every chain, number of streams of the state table)"""
    if nblk == 12:
        chains = [(7, 5, 3, 1), (0, 1, 0, 0), (4, 2, 5, 0), (2, 1, 1, 1), (6, 1, 4, 0)]      # (b0, n, stream, has)
        free = [1, 3]
    elif nblk == 7:
        chains = [(4, 3, 2, 0), (0, 1, 4, 1), (2, 1, 1, 0)]
        free = [1, 3]
    else:
        raise ValueError(nblk)
    covered = sorted(b for b0, n, _, _ in chains for b in range(b0, b0 + n))
    assert sorted(covered + free) == list(range(nblk))
    jobs = np.array([[b0, n, s * n_layers, int(bool(has) != flip)] for b0, n, s, has in chains], np.int32)
    return jobs, free, 6


def ctx_handoff_ref(x, R, jobs, state, layer):
    """the hand-off as pure copying, in place on numpy arrays of any dtype: slot 0 of every block of a chain <- row R - 1
    of the block before it (the first block's: the saved state if valid, else its own row R - 1); state <- row R - 1 of
    the chain's last block"""
    d = x.shape[-1]
    for b0, nbk, srow, has in np.asarray(jobs).tolist():
        xv = x[b0 * R:(b0 + nbk) * R].reshape(nbk, R, d)
        last = xv[:, R - 1].copy()
        xv[0, 0] = state[srow + layer] if has else last[0]
        xv[1:, 0] = last[:-1]
        state[srow + layer] = last[-1]


def block_attention_f64(qkv, nblk, R, H, masked):
    """encoder block attention in float64: qkv [nblk * R][3 d] -> [nblk * R][d].  masked: query row 0 gives zeros, key
    column R - 1 is not attended to"""
    d = qkv.shape[1] // 3
    dk = d // H
    q, k, v = (np.asarray(qkv, np.float64)[:nblk * R].reshape(nblk, R, 3, H, dk)[:, :, i].transpose(0, 2, 1, 3) for i in range(3))
    sc = q @ k.transpose(0, 1, 3, 2) / math.sqrt(dk)
    nk = R - 1 if masked else R
    out = np.zeros((nblk, H, R, dk))
    if nk > 0:
        s = sc[..., :nk]
        p = np.exp(s - s.max(axis=-1, keepdims=True))
        p /= p.sum(axis=-1, keepdims=True)
        out = p @ v[:, :, :nk]
    if masked:
        out[:, :, 0] = 0.0
    return out.transpose(0, 2, 1, 3).reshape(nblk * R, d)


def _ln64(x, g, b, eps):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def encoder_layers_f64(layers, x, nblk, R, H, masked, jobs, state, eps):
    """The contextual block encoder layers in float64, from the unpacked weights (dicts with ln1_g, ln1_b, wqkv, bqkv, wo,
    bo, ln2_g, ln2_b, w1, b1, w2, b2): norm1, q|k|v, masked block attention, output Linear + residual, norm2, feed-forward
    + residual, context hand-off.  -> (x, state) as new float64 arrays"""
    x = np.array(x, np.float64)
    state = np.array(state, np.float64)
    for li, lw in enumerate(layers):
        w = {k: np.asarray(v, np.float64) for k, v in lw.items()}
        qkv = _ln64(x, w["ln1_g"], w["ln1_b"], eps) @ w["wqkv"].T + w["bqkv"]
        x = x + block_attention_f64(qkv, nblk, R, H, masked) @ w["wo"].T + w["bo"]
        h = np.maximum(_ln64(x, w["ln2_g"], w["ln2_b"], eps) @ w["w1"].T + w["b1"], 0.0)
        x = x + h @ w["w2"].T + w["b2"]
        if masked and len(jobs):
            ctx_handoff_ref(x, R, jobs, state, li)
    return x, state


ENC_KEYS = ("ln1_g", "ln1_b", "wqkv", "bqkv", "wo", "bo", "ln2_g", "ln2_b", "w1", "b1", "w2", "b2")


def encoder_case(n_layers, flip=False, R=42, nblk=7, d=256):
    """inputs of the sc_encoder_layers tests: x at the scale 8 * randn, the chain table of 7 blocks, a state table with
    rows of streams and layers the chains never name"""
    jobs, free, n_streams = chain_table(nblk, n_layers, flip)
    rng = np.random.RandomState(4000 + n_layers)
    x0 = (8.0 * rng.randn(nblk * R, d)).astype(np.float32)
    state0 = rng.randn(n_streams * n_layers, d).astype(np.float32)
    return types.SimpleNamespace(x0=x0, state0=state0, jobs=jobs, free=free, nblk=nblk, R=R, n_layers=n_layers)


def run_encoder_layers(backend, w, case, device="cpu", jobs=None):
    """sc_encoder_layers of `backend` over the case (jobs: another chain table, e.g. an empty one) -> (x, state) numpy"""
    import torch
    cfg = w.cfg
    M, d, F = case.nblk * case.R, cfg.d_model, cfg.ffn_dim
    jobs = case.jobs if jobs is None else jobs
    jt = torch.from_numpy(np.ascontiguousarray(jobs if len(jobs) else np.zeros((1, 4), np.int32))).to(device)
    x, st = torch.from_numpy(case.x0.copy()).to(device), torch.from_numpy(case.state0.copy()).to(device)
    xn, att = torch.zeros(M, d, device=device), torch.zeros(M, d, device=device)
    qkv, ffh = torch.zeros(M, 3 * d, device=device), torch.zeros(M, F, device=device)
    backend.encoder_layers(w, x, case.nblk, case.R, True, jt, len(jobs), st, xn, qkv, att, ffh)
    if str(device) != "cpu":
        torch.cuda.synchronize()
    return x.cpu().numpy(), st.cpu().numpy()


@functools.lru_cache(maxsize=1)
def xl_state_dict():
    from speechcatcher_amd import synth
    from speechcatcher_amd.config import XL
    return synth.make_state_dict(XL, 1234)


@functools.lru_cache(maxsize=4)
def _xl_packed(device, dtype="float32"):
    from speechcatcher_amd.config import XL
    from speechcatcher_amd.weights import PackedWeights
    return PackedWeights(xl_state_dict(), XL, device, ffn_dtype=dtype, proj_dtype=dtype)


def xl_weights(n_layers, device="cpu", dtype="float32"):
    """the seeded XL weights, cut to the first `n_layers` encoder layers (a fresh object per call: backends cache their
    layer tables on it).  dtype: the weight form of the feed-forward and the attention projections (PackedWeights'
    ffn_dtype and proj_dtype: "float32", "float16" or "split16")"""
    w = copy.copy(_xl_packed(str(device), dtype))
    w.enc = w.enc[:n_layers]
    return w


def enc_layers_as_numpy(w):
    return [{k: lw[k].detach().cpu().numpy() for k in ENC_KEYS} for lw in w.enc]

"""The energy-curve contract of file mode in plain numpy float64, written independently of the host path
(segmenter.smoothed_negative_energy: numpy rfft, a dense filter matmul, scipy's gaussian_filter1d) and of
csrc/segment.hip: a plain radix-2 FFT with table twiddles, sparse filter sums, a hand-ordered Gaussian sum.

    s[0] = x[0];  s[i] = x[i] - 0.97 * x[i-1]                     (on the int16 values)
    F = 1 if n <= 400 else 1 + ceil((n - 400) / 160)                frames of 400 samples every 160, zeros after the end
    P_f[k] = |rfft_512(frame f zero-padded to 512)[k]|^2 / 512,  k = 0..256
    E_f[j] = sum_k P_f[k] * fb[j][k],  j = 0..25                    fb = segmenter._mel_filterbank(26, 512, 16000)
    E_f[j] == 0  ->  2.220446049250313e-16
    p[f] = (sum_j log E_f[j]) / 10
    w[d] = exp(-d^2 / 800) / sum,  d = -80..80
    y[f] = - sum_d w[d] * p[refl(f + d)],  refl(i): i mod 2F, then 2F-1-i if >= F
"""
import numpy as np

WIN, HOP, NFFT, NFILT, RADIUS = 400, 160, 512, 26, 80
EPS = 2.220446049250313e-16

# the eight signal kinds the contract was measured on, and the lengths that give F = 1, 1, 1, 2, 2, 3, 24, 80 and 81
KINDS = ("speechlike", "gaps", "square", "dc", "silence", "impulses", "sine", "lsb_noise")
EDGE_LENGTHS = (1, 399, 400, 401, 560, 561, 4000, 12960, 13121)


def frame_count(n: int) -> int:
    return 1 if n <= WIN else 1 + -((-(n - WIN)) // HOP)


def samples_for_frames(F: int) -> int:
    """the largest n with frame_count(n) == F"""
    return WIN if F == 1 else WIN + (F - 1) * HOP


def filterbank() -> np.ndarray:
    from speechcatcher_amd.segmenter import _mel_filterbank
    return _mel_filterbank(NFILT, NFFT, 16000)


def gauss_weights() -> np.ndarray:
    d = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    w = np.exp(-(d * d) / 800.0)
    return w / w.sum()


def refl(i, F: int):
    r = np.mod(np.asarray(i, dtype=np.int64), 2 * F)
    return np.where(r >= F, 2 * F - 1 - r, r)


def _fft512(frames: np.ndarray) -> np.ndarray:
    """radix-2 decimation in time over rows of 512 real values -> complex [rows][512]; twiddles from one table"""
    bits = NFFT.bit_length() - 1
    idx = np.arange(NFFT)
    rev = np.zeros(NFFT, dtype=np.int64)
    for b in range(bits):
        rev |= ((idx >> b) & 1) << (bits - 1 - b)
    z = frames[:, rev].astype(np.complex128)
    ang = 2.0 * np.pi * np.arange(NFFT // 2, dtype=np.float64) / NFFT
    tw = np.cos(ang) - 1j * np.sin(ang)
    for s in range(1, bits + 1):
        m, hm = 1 << s, 1 << (s - 1)
        z = z.reshape(-1, NFFT // m, m)
        u, v = z[:, :, :hm], z[:, :, hm:] * tw[:: NFFT // m][None, None, :]
        z = np.concatenate([u + v, u - v], axis=2).reshape(-1, NFFT)
    return z


def raw_curve(x, chunk: int = 8192) -> np.ndarray:
    """p[f]: summed log filterbank energies / 10 (the curve before the Gaussian and the sign flip)"""
    x = np.asarray(x)
    assert x.dtype == np.int16 and x.ndim == 1 and len(x) >= 1
    n, F = len(x), frame_count(len(x))
    s = x.astype(np.float64)
    s[1:] = s[1:] - 0.97 * x[:-1].astype(np.float64)
    pad = np.zeros((F - 1) * HOP + NFFT, dtype=np.float64)      # the zeros behind the end, and up to 512 for the last frame
    pad[:n] = s
    fb = filterbank()
    edges = [(int(np.flatnonzero(row)[0]), int(np.flatnonzero(row)[-1]) + 1) if row.any() else (0, 0) for row in fb]
    p = np.empty(F, dtype=np.float64)
    for a in range(0, F, chunk):
        b = min(F, a + chunk)
        idx = (np.arange(a, b) * HOP)[:, None] + np.arange(NFFT)[None, :]
        frames = pad[idx]
        frames[:, WIN:] = 0.0
        z = _fft512(frames)[:, : NFFT // 2 + 1]
        P = (z.real * z.real + z.imag * z.imag) * (1.0 / NFFT)
        acc = np.zeros(b - a, dtype=np.float64)
        for j, (lo, hi) in enumerate(edges):
            e = np.zeros(b - a, dtype=np.float64)
            for k in range(lo, hi):
                e = e + P[:, k] * fb[j, k]
            e = np.where(e == 0.0, EPS, e)
            acc = acc + np.log(e)
        p[a:b] = acc / 10.0
    return p


def smooth(p: np.ndarray) -> np.ndarray:
    """y[f] = - sum_d w[d] p[refl(f + d)], d ascending"""
    F = len(p)
    w = gauss_weights()
    f = np.arange(F, dtype=np.int64)
    acc = np.zeros(F, dtype=np.float64)
    for t, d in enumerate(range(-RADIUS, RADIUS + 1)):
        acc = acc + w[t] * p[refl(f + d, F)]
    return -acc


def energy_curve(x, smoothed: bool = True) -> np.ndarray:
    p = raw_curve(x)
    return smooth(p) if smoothed else p


def make_signal(kind: str, n: int, seed: int = 0) -> np.ndarray:
    """seeded int16 test recordings of n samples at 16 kHz"""
    rng = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    if kind == "speechlike":
        x = ((np.sin(2 * np.pi * t / 7.3) > 0.2) * 0.3 + 0.002) * rng.randn(n) * 8000
    elif kind == "gaps":
        x = (np.sin(2 * np.pi * t / 11.0) > 0) * 0.25 * rng.randn(n) * 8000
    elif kind == "square":
        x = np.where((np.arange(n) // 40) % 2 == 0, 32767.0, -32768.0)
    elif kind == "dc":
        x = np.full(n, 1234.0)
    elif kind == "silence":
        x = np.zeros(n)
    elif kind == "impulses":
        x = np.zeros(n)
        x[rng.randint(0, n, size=max(1, n // 20000))] = 20000.0
    elif kind == "sine":
        x = 12000.0 * np.sin(2 * np.pi * (32 * 16000.0 / 512) * t)     # centre of bin 32
    elif kind == "lsb_noise":
        x = rng.randint(-1, 2, size=n).astype(np.float64)
    else:
        raise ValueError(kind)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)

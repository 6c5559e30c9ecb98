"""A float64 numpy restatement of the sample-rate converter and of STOI / ESTOI, independent of the kernels' structure:
the resampler is ``scipy.signal.resample_poly`` with the table as its window, the silent-frame removal materialises the
overlap-added signals, the transform is ``np.fft.rfft``.  Also the deterministic test signals."""
import functools
import math

import numpy as np

FS, FRAME, HOP, N_FFT, N_BANDS, F_MIN, SEGMENT, BETA, DYN_RANGE = 10000, 256, 128, 512, 15, 150.0, 30, -15.0, 40.0
EPS = np.finfo(np.float64).eps
MARGIN_DB = 0.01            # no reference frame of a test signal may lie this close to the silence threshold
SNRS = (30.0, 10.0, 0.0, -10.0)


# ---- the resampler
def kaiser_sinc(U, D, zeros=10, beta=5.0):
    """h[0 .. 2 half], written out term by term (math.sin and the series of I0), as a check of ``audio.resample_filter``."""
    M = max(U, D)
    half = zeros * M

    def i0(v):
        s, t, k = 1.0, 1.0, 1
        while t > 1e-20 * s:
            t *= (v / (2.0 * k)) ** 2
            s += t
            k += 1
        return s
    h = np.empty(2 * half + 1)
    for k in range(2 * half + 1):
        n = k - half
        sinc = 1.0 if n == 0 else math.sin(math.pi * n / M) / (math.pi * n / M)
        h[k] = sinc * i0(beta * math.sqrt(max(0.0, 1.0 - (n / half) ** 2))) / i0(beta)
    return h * (U / h.sum())


def resample(x, U, D, h):
    """``y[m] = sum_i x[i] h[m D - i U + half]``, ``ceil(len U / D)`` samples, through scipy (which multiplies an array
    window by ``up``, hence ``h / U``)."""
    from scipy.signal import resample_poly
    if U == D == 1:
        return np.asarray(x, dtype=np.float64).copy()
    return resample_poly(np.asarray(x, dtype=np.float64), U, D, window=np.asarray(h, dtype=np.float64) / U)


def resample_bound(x, U, D, h32):
    """Per output sample ``(n + 2) 2^-24 sum_i |x_i| |h_k|`` (float64) for the fp32 fmaf chain over the float32 table
    ``h32``: gamma_n of the chain plus the rounding of the taps (the oracle runs on the float64 table)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    h = np.abs(np.asarray(h32, dtype=np.float64))
    half = (len(h) - 1) // 2
    out_len = -((-len(x) * U) // D)
    bound = np.empty(out_len)
    for m in range(out_len):
        c = m * D + half
        ilo = max(0, -((-(c - 2 * half)) // U))
        ihi = min(len(x) - 1, c // U)
        i = np.arange(ilo, ihi + 1)
        bound[m] = (len(i) + 2) * 2.0 ** -24 * float(np.sum(x[i] * h[c - i * U]))
    return bound


# ---- STOI
def bands():
    f = np.linspace(0.0, FS, N_FFT + 1)[:N_FFT // 2 + 1]
    obm = np.zeros((N_BANDS, len(f)))
    for k in range(N_BANDS):
        c = F_MIN * 2.0 ** (k / 3.0)
        lo = int(np.argmin(np.abs(f - c * 2.0 ** (-1.0 / 6.0))))
        hi = int(np.argmin(np.abs(f - c * 2.0 ** (1.0 / 6.0))))
        obm[k, lo:hi] = 1.0
    return obm


def remove_silent_frames(x, y):
    """The two signals without the frames whose reference energy is more than DYN_RANGE below the loudest: the kept
    windowed frames overlap-added at HOP.  Also K and every frame's distance |e_j - threshold| in dB."""
    w = np.hanning(FRAME + 2)[1:-1]
    starts = range(0, len(y) - FRAME + 1, HOP)
    xf = np.array([w * x[i:i + FRAME] for i in starts])
    yf = np.array([w * y[i:i + FRAME] for i in starts])
    e = 20.0 * np.log10(np.linalg.norm(yf, axis=1) + EPS)
    thr = e.max() - DYN_RANGE
    keep = e > thr
    xf, yf = xf[keep], yf[keep]
    K = len(xf)
    xs, ys = np.zeros((K - 1) * HOP + FRAME), np.zeros((K - 1) * HOP + FRAME)
    for k in range(K):
        xs[k * HOP:k * HOP + FRAME] += xf[k]
        ys[k * HOP:k * HOP + FRAME] += yf[k]
    return xs, ys, K, np.abs(e - thr)


def band_magnitudes(s, K):
    w = np.hanning(FRAME + 2)[1:-1]
    spec = np.array([np.fft.rfft(w * s[k * HOP:k * HOP + FRAME], N_FFT) for k in range(K)])
    return np.sqrt(np.abs(spec) ** 2 @ bands().T)          # [K, N_BANDS]


def stoi(x, y):
    """``(stoi, estoi, frames kept, segments, margins)`` of generated ``x`` against clean ``y``, both at 10 kHz; NaN with
    fewer than SEGMENT kept frames."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    xs, ys, K, margins = remove_silent_frames(x, y)
    M = max(K - SEGMENT + 1, 0)
    if M == 0:
        return float("nan"), float("nan"), K, 0, margins
    X, Y = band_magnitudes(xs, K), band_magnitudes(ys, K)
    clip = 1.0 + 10.0 ** (-BETA / 20.0)
    d_sum = e_sum = 0.0
    for m in range(M):
        xm, ym = X[m:m + SEGMENT].T, Y[m:m + SEGMENT].T    # [bands, N]
        alpha = np.linalg.norm(ym, axis=1, keepdims=True) / (np.linalg.norm(xm, axis=1, keepdims=True) + EPS)
        xp = np.minimum(alpha * xm, clip * ym)
        xp = xp - xp.mean(axis=1, keepdims=True)
        yc = ym - ym.mean(axis=1, keepdims=True)
        xp = xp / (np.linalg.norm(xp, axis=1, keepdims=True) + EPS)
        yc = yc / (np.linalg.norm(yc, axis=1, keepdims=True) + EPS)
        d_sum += float(np.sum(xp * yc))

        def row_col(a):
            a = a - a.mean(axis=1, keepdims=True)
            a = a / (np.linalg.norm(a, axis=1, keepdims=True) + EPS)
            a = a - a.mean(axis=0, keepdims=True)
            return a / (np.linalg.norm(a, axis=0, keepdims=True) + EPS)
        e_sum += float(np.sum(row_col(xm) * row_col(ym))) / SEGMENT
    return d_sum / (M * N_BANDS), e_sum / M, K, M, margins


def stoi_at(x, y, sr, h=None):
    """``stoi`` of two signals at ``sr``: converted to 10 kHz first (``h``: the float64 table; None at 10 kHz)."""
    if sr == FS:
        return stoi(x, y)
    g = math.gcd(sr, FS)
    return stoi(resample(x, FS // g, sr // g, h), resample(y, FS // g, sr // g, h))


# ---- signals
def speech_like(n, sr, seed):
    """24 harmonics of a wandering f0 under a syllable-rate envelope, gated to a low level at the start, in the middle and
    at the end (frames are removed inside and at both ends).  The gaps hold the signal 70 dB down: far below the 40 dB
    range, so no frame sits near the threshold by construction of the level alone (the tests assert the margin)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f0 = 120.0 + 25.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6)) + 8.0 * np.sin(2 * np.pi * 2.3 * t)
    phase = 2 * np.pi * np.cumsum(f0) / sr
    s = np.zeros(n)
    for k in range(1, 25):
        s += np.sin(k * phase + rng.uniform(0, 6)) / k ** 0.8 * (k * 145.0 < 0.45 * sr)
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t + 1.0)
    s *= env
    gate = np.ones(n)
    for a, b in ((0.0, 0.09), (0.46, 0.58), (0.93, 1.0)):
        gate[int(a * n):int(b * n)] = 10.0 ** (-70.0 / 20.0)
    s = s * gate + 1e-5 * rng.standard_normal(n)
    return 0.5 * s / np.abs(s).max()


def add_noise(y, snr_db, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(len(y))
    v *= np.sqrt(np.mean(y ** 2) / np.mean(v ** 2)) * 10.0 ** (-snr_db / 20.0)
    return y + v


def hard_clip(y, level=0.08):
    return np.clip(y, -level, level)


SETS = {"A": (22050, 1.2), "B": (16000, 1.0), "C": (10000, 0.9)}


@functools.lru_cache(maxsize=None)
def signal_set(name):
    """``(sr, y, [x ...])`` as float32 arrays: the reference and its five degradations (the four SNRS, then clipping)."""
    sr, seconds = SETS[name]
    n = int(round(sr * seconds))
    seed = 11 + ord(name)
    y = speech_like(n, sr, seed)
    xs = [add_noise(y, snr, seed + 100 + i) for i, snr in enumerate(SNRS)] + [hard_clip(y)]
    return sr, y.astype(np.float32), [x.astype(np.float32) for x in xs]


@functools.lru_cache(maxsize=None)
def stationary_noise(n, seed=5):
    """Set D: stationary noise at 10 kHz (every frame is kept) and a noisier copy."""
    rng = np.random.default_rng(seed)
    y = 0.1 * rng.standard_normal(n)
    x = y + 0.05 * rng.standard_normal(n)
    return x.astype(np.float32), y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference_values(name):
    """The restatement on set ``name``: a list of ``(stoi, estoi, K, M, margins)``, one per degradation, then y against
    itself.  float32 inputs (what the kernels see), the float64 filter table."""
    from diffwave_sashimi_amd.audio import resample_filter
    sr, y, xs = signal_set(name)
    h = None if sr == FS else resample_filter(sr, FS)[2]
    return [stoi_at(x, y, sr, h) for x in xs + [y]]

"""A float64 restatement of the inversion kernels (``csrc/griffinlim_kernels.hip``; include/dws.h: dws_istft,
dws_griffin_lim) in numpy ``rfft`` / ``irfft``, and the deterministic signals the tests run them on.  The public
spectrum is torch.stft's: ``X_k = sum_i frame[i] exp(-2 pi 1j i k / N)``."""
import functools

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)      # librosa.util.tiny of the reference's float32 window sum


def hann_window(win, n_fft):
    """The engine's window: periodic Hann of ``win`` points centred in ``n_fft``, float32 (``mel.padded_hann``)."""
    n = np.arange(win, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win)
    lpad = (n_fft - win) // 2
    return np.pad(w, (lpad, n_fft - win - lpad)).astype(np.float32)


def _frames(T, hop):
    assert T % hop == 0
    return T // hop + 1


def stft64(x, window, hop):
    """``x`` [B, T] (T a multiple of hop) -> complex128 [B, K, T / hop + 1]: reflect padding by n_fft/2, centred frames."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(window, dtype=np.float64)
    n_fft = len(w)
    B, T = x.shape
    assert T >= n_fft // 2 + 1
    xp = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    F = _frames(T, hop)
    fr = np.stack([xp[:, f * hop:f * hop + n_fft] for f in range(F)], axis=1) * w      # [B, F, n_fft]
    return np.fft.rfft(fr, axis=-1).transpose(0, 2, 1)


def istft64(spec, window, hop):
    """complex [B, K, F] -> [B, (F - 1) hop]: windowed irfft frames overlap-added, divided by the window's sum of squares
    where that exceeds FLT_MIN (the reference's ``tiny`` rule; elsewhere undivided), n_fft/2 trimmed at both ends."""
    spec = np.asarray(spec, dtype=np.complex128)
    w = np.asarray(window, dtype=np.float64)
    n_fft = len(w)
    B, K, F = spec.shape
    assert K == n_fft // 2 + 1
    rows = np.fft.irfft(spec.transpose(0, 2, 1), n=n_fft, axis=-1) * w                  # [B, F, n_fft]
    n = n_fft + hop * (F - 1)
    s, wss = np.zeros((B, n)), np.zeros(n)
    for f in range(F):
        s[:, f * hop:f * hop + n_fft] += rows[:, f]
        wss[f * hop:f * hop + n_fft] += w * w
    ok = wss > FLT_MIN
    s[:, ok] /= wss[ok]
    return s[:, n_fft // 2:n_fft // 2 + (F - 1) * hop]


def project64(x, mag, window, hop):
    """The STFT of ``x`` with its magnitudes replaced by ``mag`` and its phases kept.  A condition on the inputs: no bin of
    the iterate is exactly zero (there the kernel takes phase 0, as atan2(0, 0) gives; these signals never get there)."""
    X = stft64(x, window, hop)
    a = np.abs(X)
    assert np.all(a > 0.0), "a bin of an iterate is exactly zero"
    return mag * (X / a)


def griffin_lim64(mag, phase0, window, hop, n, momentum=0.0):
    """dws_griffin_lim in float64: ``x_0 = istft(mag e^{i phase0})``, then n rounds of projection and inverse, with
    ``y_n = x_n + momentum (x_n - x_{n-1})`` feeding the next projection.  Returns ``x_n`` [B, (F - 1) hop]."""
    mag = np.asarray(mag, dtype=np.float64)
    x = istft64(mag * np.exp(1j * np.asarray(phase0, dtype=np.float64)), window, hop)
    y = x
    for _ in range(n):
        xn = istft64(project64(y, mag, window, hop), window, hop)
        y = xn + momentum * (xn - x)
        x = xn
    return x


def spectral_convergence(x, mag, window, hop):
    """``|| |STFT(x)| - M || / || M ||`` over the whole batch, in float64."""
    mag = np.asarray(mag, dtype=np.float64)
    return float(np.linalg.norm(np.abs(stft64(x, window, hop)) - mag) / np.linalg.norm(mag))


def rel_l2(a, b):
    """Relative l2 distance of ``a`` from ``b`` (real or complex), in float64."""
    kind = np.complex128 if np.iscomplexobj(a) or np.iscomplexobj(b) else np.float64
    a, b = np.asarray(a, dtype=kind), np.asarray(b, dtype=kind)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def test_signal(B, T, seed=0):
    """[B, T] float64 in (-1, 1): a chirp plus a tone plus weak noise per row, deterministic."""
    rng = np.random.RandomState(1234 + seed)
    t = np.arange(T, dtype=np.float64)
    rows = []
    for b in range(B):
        f0, f1 = 0.01 + 0.007 * b, 0.19 - 0.02 * b                     # cycles per sample
        chirp = np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / T) + 0.3 * b)
        tone = 0.5 * np.sin(2 * np.pi * (0.083 + 0.011 * b) * t + 1.1)
        rows.append(0.45 * chirp + 0.3 * tone + 0.02 * rng.standard_normal(T))
    out = np.stack(rows)
    out.setflags(write=False)
    return out


test_signal.__test__ = False        # a helper, not a test


@functools.lru_cache(maxsize=None)
def phases(B, K, F, seed=0):
    """Uniform phases in [-pi, pi), float32 values held in float64 (what both sides of a parity test start from)."""
    rng = np.random.RandomState(77 + seed)
    out = ((rng.rand(B, K, F) * 2.0 - 1.0) * np.pi).astype(np.float32).astype(np.float64)
    out.setflags(write=False)
    return out

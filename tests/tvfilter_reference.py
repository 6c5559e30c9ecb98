"""A float64 restatement of the time-varying spectral filter (``csrc/tvfilter_kernels.hip``; include/dws.h:
dws_tv_filter) on ``tests/griffinlim_reference.py``'s ``stft64`` / ``istft64``, of its exact transpose, and of the filter
design of ``mel.minimum_phase_filter``, in numpy.  The public spectrum is torch.stft's."""
import numpy as np

from tests.griffinlim_reference import FLT_MIN, istft64, stft64


def _clip(x, filt, lengths, b, hop):
    n = x.shape[1] if lengths is None else int(lengths[b])
    return np.asarray(x[b:b + 1, :n], dtype=np.float64), np.asarray(filt[b:b + 1, :, :n // hop + 1], dtype=np.complex128)


def tv_forward64(x, filt, window, hop, lengths=None):
    """``istft64(filt * stft64(x))`` clip by clip: [B, T] -> [B, T], 0 behind a clip's own length."""
    out = np.zeros(np.shape(x), dtype=np.float64)
    for b in range(out.shape[0]):
        xb, fb = _clip(x, filt, lengths, b, hop)
        out[b, :xb.shape[1]] = istft64(fb * stft64(xb, window, hop), window, hop)[0]
    return out


def _adjoint_clip(g, filt, window, hop):
    """The transpose of ``x -> istft64(filt * stft64(x))`` for one clip: g [T], filt [K, F] -> [T]."""
    w = np.asarray(window, dtype=np.float64)
    n_fft, half = len(w), len(w) // 2
    T = g.shape[0]
    F = T // hop + 1
    n = n_fft + hop * (F - 1)
    wss = np.zeros(n)
    for f in range(F):
        wss[f * hop:f * hop + n_fft] += w * w
    q = np.zeros(n)
    q[half:half + T] = g
    ok = wss > FLT_MIN
    q[ok] /= wss[ok]
    rows = np.stack([w * q[f * hop:f * hop + n_fft] for f in range(F)])          # [F, n_fft]
    k = np.arange(half + 1)
    h = np.where((k == 0) | (k == half), 1.0, 2.0) / n_fft
    R = np.fft.rfft(rows, axis=-1)                       # sum_i row[i] (cos - i sin)
    dY = h * R                                           # dRe = h sum row cos, dIm = -h sum row sin
    dY.imag[:, 0] = 0.0
    dY.imag[:, half] = 0.0
    dX = np.conj(filt.T) * dY                            # [F, K]
    ang = 2.0 * np.pi * np.outer(np.arange(n_fft), k) / n_fft
    u = (dX.real @ np.cos(ang).T - dX.imag @ np.sin(ang).T) * w                   # [F, n_fft], no h weights
    pad = np.zeros(n)
    for f in range(F):
        pad[f * hop:f * hop + n_fft] += u[f]
    idx = np.pad(np.arange(T), (half, half), mode="reflect")                      # the padded position's source sample
    out = np.zeros(T)
    np.add.at(out, idx, pad)
    return out


def tv_adjoint64(g, filt, window, hop, lengths=None):
    """The exact transpose of ``tv_forward64`` (same ``filt``): [B, T] -> [B, T], 0 behind a clip's own length."""
    out = np.zeros(np.shape(g), dtype=np.float64)
    for b in range(out.shape[0]):
        gb, fb = _clip(g, filt, lengths, b, hop)
        out[b, :gb.shape[1]] = _adjoint_clip(gb[0], fb[0], window, hop)
    return out


def design64(magnitude, n_frames, ref, floor=0.01, lifter=24):
    """``mel.minimum_phase_filter`` in numpy float64: magnitudes [B, K, frames] -> complex128 [B, K, n_frames]."""
    m = np.asarray(magnitude, dtype=np.float64).transpose(0, 2, 1)
    n_fft = 2 * (m.shape[-1] - 1)
    p = np.maximum(m, floor * ref) ** 2 / ref ** 2
    c = np.fft.irfft(np.log(p), n=n_fft, axis=-1)
    c_mp = np.zeros_like(c)
    c_mp[..., 0] = c[..., 0]
    c_mp[..., 1:lifter + 1] = 2.0 * c[..., 1:lifter + 1]
    F = np.exp(0.5 * np.fft.rfft(c_mp, axis=-1))
    idx = np.minimum(np.arange(n_frames), m.shape[1] - 1)
    return F[:, idx].transpose(0, 2, 1)


def liftered_envelope64(magnitude, ref, floor=0.01, lifter=24):
    """The cepstrally smoothed envelope ``|F|^2`` should equal: exp of the log envelope with its cepstrum cut to
    ``|n| <= lifter`` (symmetric lifter), [B, K, frames]."""
    m = np.asarray(magnitude, dtype=np.float64).transpose(0, 2, 1)
    n_fft = 2 * (m.shape[-1] - 1)
    c = np.fft.irfft(2.0 * np.log(np.maximum(m, floor * ref) / ref), n=n_fft, axis=-1)
    keep = np.zeros(n_fft)
    keep[:lifter + 1] = 1.0
    keep[n_fft - lifter:] = 1.0
    return np.exp(np.fft.rfft(c * keep, axis=-1).real).transpose(0, 2, 1)

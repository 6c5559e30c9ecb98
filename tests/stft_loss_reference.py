"""Float64 CPU restatement of ``diffwave_sashimi_amd.metrics.mr_stft_loss`` (include/dws.h,
``dws_spectral_loss_backward``) -- the checker of tests/test_stft_loss.py, tests/test_stft_loss_gpu.py and
tests/test_stft_loss_cli_gpu.py, never a product path.

``loss`` is written from the formulas with ``spectral_reference.power`` (``torch.stft``) as the transform and is
differentiated by torch autograd, clip by clip for a ragged batch.  ``adjoint`` is the hand-written float64 adjoint of
one resolution in the notation of include/dws.h (explicit reflect map, explicit cos / +sin tables), which the kernel
implements in float32; tests/test_stft_loss.py holds the two against each other, which pins the conventions (the floor
rule, sgn(0) = 0, each bin once, the reflection about the clip's own ends) without a GPU.

One convention differs from plain autograd on purpose: a clip whose spectral-convergence numerator is exactly 0 gets a
zero gradient from that term, where the square root's derivative gives NaN.
"""
import functools
import math

import torch

from diffwave_sashimi_amd.mel import padded_hann
from tests.spectral_reference import FLOOR, RESOLUTIONS, power, signal_pair


def clip_terms(x, y, n_fft, hop, win):
    """(sc_num, sc_den, mag_abs) of one clip pair (x, y [T], float64), differentiable in x."""
    px, py = power(x, n_fft, hop, win), power(y, n_fft, hop, win)
    mx, my = torch.sqrt(px.clamp_min(FLOOR)), torch.sqrt(py.clamp_min(FLOOR))
    return ((my - mx) ** 2).sum(), (my ** 2).sum(), (torch.log(my) - torch.log(mx)).abs().sum()


def clip_loss(x, y, resolutions=RESOLUTIONS, sc_weight=1.0, mag_weight=1.0):
    """The loss of one clip pair (x, y [T]): a float64 scalar, differentiable in x."""
    x, y = x.double(), y.double().detach()
    total = 0.0
    for n_fft, hop, win in resolutions:
        num, den, mag = clip_terms(x, y, n_fft, hop, win)
        sc = torch.sqrt(num / den) if float(num.detach()) != 0.0 else num * 0.0      # (an exact match: zero, and zero gradient)
        total = total + sc_weight * sc + mag_weight * mag / ((x.shape[0] // hop + 1) * (n_fft // 2 + 1))
    return total / len(resolutions)


def loss(x, y, lengths=None, resolutions=RESOLUTIONS, sc_weight=1.0, mag_weight=1.0):
    """x, y [B, T] (any device, any float dtype) -> float64 [B] on the CPU, differentiable in x across the devices; clip b
    is its first ``lengths[b]`` samples (nothing behind them is read)."""
    B, T = x.shape
    lengths = [T] * B if lengths is None else [int(n) for n in lengths]
    xc, yc = x.cpu(), y.detach().cpu()
    return torch.stack([clip_loss(xc[b, :n], yc[b, :n], resolutions, sc_weight, mag_weight) for b, n in enumerate(lengths)])


def gradient(x, y, resolutions=RESOLUTIONS, sc_weight=1.0, mag_weight=1.0):
    """d clip_loss / d x of one clip pair by autograd: float64 [T]."""
    x = x.double().clone().requires_grad_(True)
    clip_loss(x, y, resolutions, sc_weight, mag_weight).backward()
    return x.grad


@functools.lru_cache(maxsize=None)
def signal_gradient(kind, length, resolutions=RESOLUTIONS, sc_weight=1.0, mag_weight=1.0):
    """``gradient`` of ``signal_pair(kind, length)``, computed once per session.  Do not modify the result."""
    return gradient(*signal_pair(kind, length), resolutions, sc_weight, mag_weight)


def adjoint(x, y, coef, n_fft, hop, win):
    """include/dws.h, ``dws_spectral_loss_backward``, for one clip in float64: x, y [T], coef = (c0, c1) -> dx [T]."""
    x, y = x.double(), y.double()
    n, half, K = x.shape[0], n_fft // 2, n_fft // 2 + 1
    w = torch.from_numpy(padded_hann(win, n_fft)).double()
    f = torch.arange(n // hop + 1)[:, None]
    i = torch.arange(n_fft)[None, :]
    j = f * hop + i - half
    j = torch.where(j < 0, -j, j)
    j = torch.where(j >= n, 2 * (n - 1) - j, j)               # rho_b: [frames, n_fft]
    ang = 2.0 * math.pi * ((torch.arange(n_fft)[:, None] * torch.arange(K)[None, :]) % n_fft).double() / n_fft
    cos, sin = torch.cos(ang), torch.sin(ang)                 # [n_fft, K]
    fx, fy = x[j] * w, y[j] * w
    xr, xi, yr, yi = fx @ cos, fx @ sin, fy @ cos, fy @ sin   # [frames, K]
    px, py = xr ** 2 + xi ** 2, yr ** 2 + yi ** 2
    mx, my = torch.sqrt(px.clamp_min(FLOOR)), torch.sqrt(py.clamp_min(FLOOR))
    sg = torch.sign(torch.log(my) - torch.log(mx))
    dmag = -(coef[0] * (my - mx) + coef[1] * sg / mx)
    dmag = torch.where(px >= FLOOR, dmag, torch.zeros_like(dmag))
    dre, dim = dmag * xr / mx, dmag * xi / mx
    dframe = (dre @ cos.T + dim @ sin.T) * w                  # [frames, n_fft]
    return torch.zeros(n, dtype=torch.float64).index_add_(0, j.reshape(-1), dframe.reshape(-1))


def adjoint_gradient(x, y, resolutions=RESOLUTIONS, sc_weight=1.0, mag_weight=1.0):
    """d clip_loss / d x through ``adjoint`` with the coefficients ``mr_stft_loss`` forms: float64 [T]."""
    dx = torch.zeros(x.shape[0], dtype=torch.float64)
    for n_fft, hop, win in resolutions:
        with torch.no_grad():
            num, den, _ = clip_terms(x.double(), y.double(), n_fft, hop, win)
        c0 = 0.0 if float(num) == 0.0 else sc_weight / math.sqrt(float(num) * float(den))
        c1 = mag_weight / ((x.shape[0] // hop + 1) * (n_fft // 2 + 1))
        dx += adjoint(x, y, (c0 / len(resolutions), c1 / len(resolutions)), n_fft, hop, win)
    return dx


def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float(torch.linalg.vector_norm(got - want) / torch.linalg.vector_norm(want))


def rel_max(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max())

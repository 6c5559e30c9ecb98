"""Float64 torch restatement of the mel front-end's formulas (include/dws.h, `dws_mel_spectrogram_backward`), written
from the formulas alone: no import of `diffwave_sashimi_amd.mel` or `oracle/mel.py`, no stft / conv call.  Differentiable
by torch autograd, with the magnitude built so that its gradient is 0 where the magnitude is 0 (plain autograd through
sqrt gives NaN there).  The window [N] and the filterbank [n_mels, N/2+1] are inputs.  Shared by
tests/test_mel_operator.py (CPU), tests/test_mel_backward_gpu.py and tests/test_mel_guided_gpu.py (as the operator of the
float64 guided loop).

    frame_f[i] = w[i] x[rho(f hop + i - N/2)],  rho: j < 0 -> -j, j >= T -> 2(T-1) - j,  f = 0 .. T // hop
    Re_k = sum_i frame_f[i] cos(2 pi i k / N),  Im_k = sum_i frame_f[i] sin(2 pi i k / N),  k = 0 .. N/2
    mag_k = sqrt(Re_k^2 + Im_k^2),  s_m = sum_k W[m,k] mag_k,  out[m,f] = log(max(s_m, clip))"""
import math

import torch

CLIP = 1e-5

# (n_fft, hop, win, T, bands, sampling rate): the smallest shapes at which the adjoint's indexing can go wrong
CASES = [(256, 64, 256, 129, 80, 16000),        # N/2 < T < N: one sample receives both reflections
         (256, 64, 256, 255, 80, 16000), (256, 64, 256, 256, 80, 16000), (256, 64, 256, 1000, 80, 16000),
         (256, 64, 256, 4097, 80, 16000),
         (64, 16, 64, 33, 20, 16000), (64, 16, 64, 100, 20, 16000),
         (256, 64, 200, 1000, 80, 16000),       # window shorter than the filter
         (256, 100, 256, 1000, 80, 16000),      # a hop that divides neither N nor T
         (1024, 256, 1024, 513, 80, 22050)]     # LJ's transform, three frames
CASE_SEED = 5


def case_inputs(case, B=3, seed=CASE_SEED):
    """x [B, T] = (rand 2 - 1) 0.8 and a random cotangent g [B, bands, F], float32, the same for every caller."""
    n_fft, hop, win, T, bands, sr = case
    gen = torch.Generator().manual_seed(seed * 100003 + n_fft * 7 + hop * 3 + win + T)
    x = (torch.rand(B, T, generator=gen) * 2 - 1) * 0.8
    g = torch.randn(B, bands, T // hop + 1, generator=gen)
    return x, g


def reflect_index(T, n_fft, hop):
    """int64 [F, N]: the sample every (frame, tap) reads."""
    F = T // hop + 1
    j = torch.arange(F)[:, None] * hop + torch.arange(n_fft)[None, :] - n_fft // 2
    j = torch.where(j < 0, -j, j)
    return torch.where(j >= T, 2 * (T - 1) - j, j)


def safe_magnitude(re, im):
    """sqrt(re^2 + im^2) whose gradient is exactly 0 where the magnitude is 0."""
    sq = re * re + im * im
    live = sq > 0
    return torch.where(live, torch.sqrt(torch.where(live, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def mel_energies(x, window, basis, n_fft, hop):
    """x [B, T] float64 -> s [B, n_mels, F] (before clamp and log)."""
    B, T = x.shape
    assert T > n_fft // 2 and x.dtype == torch.float64
    frames = x[:, reflect_index(T, n_fft, hop)] * window.double()            # [B, F, N]
    ik = (torch.arange(n_fft)[:, None] * torch.arange(n_fft // 2 + 1)[None, :]) % n_fft      # exact phase index
    ang = ik.double() * (2.0 * math.pi / n_fft)
    mag = safe_magnitude(frames @ torch.cos(ang), frames @ torch.sin(ang))   # [B, F, K]
    return torch.einsum("mk,bfk->bmf", basis.double(), mag)


def mel_spectrogram(x, window, basis, n_fft, hop, clip=CLIP):
    """x [B, T] -> log-mel [B, n_mels, T // hop + 1], float64."""
    return torch.log(torch.clamp(mel_energies(x.double(), window, basis, n_fft, hop), min=clip))


def mel_gradient(x, g, window, basis, n_fft, hop, clip=CLIP):
    """d<g, mel(x)>/dx in float64 (x [B, T], g [B, n_mels, F])."""
    xin = x.detach().double().clone().requires_grad_(True)
    (dx,) = torch.autograd.grad((mel_spectrogram(xin, window, basis, n_fft, hop, clip) * g.double()).sum(), xin)
    return dx


def reference_operator(window, basis, n_fft, hop, clip=CLIP, frames=None):
    """The differentiable float64 operator of the guided reference loop: [B, 1, L] or [B, L] -> [B, n_mels, L // hop + 1]
    (the first `frames` of them where given)."""
    def A(x):
        m = mel_spectrogram(x[:, 0] if x.dim() == 3 else x, window, basis, n_fft, hop, clip)
        return m if frames is None else m[..., :frames]
    return A

"""Float64 torch restatement, on the CPU, of the objective metrics of ``diffwave_sashimi_amd.metrics`` (include/dws.h,
``dws_spectral_distance``), written from the formulas with ``torch.stft`` as the transform -- the checker of
tests/test_metrics.py, tests/test_metrics_gpu.py and tests/test_evaluate_cli_gpu.py, never a product path.

With ``S = stft(s, n_fft, hop, window=padded_hann(win, n_fft), center=True, pad_mode="reflect")`` of one clip (frames
``f = 0 .. len // hop``, bins ``k = 0 .. n_fft/2``), ``|S| = sqrt(max(re^2 + im^2, 1e-7))`` and ``x`` the generated, ``y``
the reference signal:

    sc_num = sum (|Y|-|X|)^2      sc_den = sum |Y|^2      mag_abs = sum |ln|Y| - ln|X||
    lsd_sum = sum_f sqrt(mean_k (log10|Y|^2 - log10|X|^2)^2)
    logmel(S) = ln(max(basis @ sqrt(re^2 + im^2), 1e-5))                (unfloored magnitudes)
    mel_abs = sum |logmel(Y) - logmel(X)|      mcd_sum = sum_f ||D (logmel(Y)_f - logmel(X)_f)||_2
    D[d-1, k] = sqrt(2/K) cos(pi d (k + 1/2) / K),  d = 1 .. n_cep,  K = bands
"""
import math

import numpy as np
import torch

from diffwave_sashimi_amd.mel import mel_filterbank, padded_hann

FLOOR = 1e-7
CLIP = 1e-5
RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
MEL_RESOLUTION = (1024, 256, 1024)          # TacotronSTFT()'s transform
MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)
HEADLINE = ("mr_stft", "ls_mae", "lsd", "mcd")
RTOL, ATOL = 1e-5, 1e-6                     # parity bound of a kernel result against this module
ATOL_MCD = 1e-5                             # ... for mcd, in dB


def default_basis(sampling_rate=22050, n_fft=1024, n_mels=80, fmin=0.0, fmax=8000.0):
    return torch.from_numpy(mel_filterbank(sampling_rate, n_fft, n_mels, fmin, fmax))


def cepstral_table(n_cep, n_mels):
    D = np.zeros((n_cep, n_mels))
    for d in range(1, n_cep + 1):
        for k in range(n_mels):
            D[d - 1, k] = math.sqrt(2.0 / n_mels) * math.cos(math.pi * d * (k + 0.5) / n_mels)
    return torch.from_numpy(D)


def power(s, n_fft, hop, win, dtype=torch.float64):
    """s [T] or [B, T] -> re^2 + im^2, ``dtype`` [..., n_fft/2 + 1, T // hop + 1], on the device of s."""
    w = torch.from_numpy(padded_hann(win, n_fft)).to(device=s.device, dtype=dtype)
    S = torch.stft(s.to(dtype), n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode="reflect",
                   return_complex=True)
    assert S.shape[-2:] == (n_fft // 2 + 1, s.shape[-1] // hop + 1)
    return S.real ** 2 + S.imag ** 2


def sums(x, y, n_fft, hop, win, basis=None, n_cep=0, dtype=torch.float64):
    """The six sums of one clip pair (x, y [T]) as a ``dtype`` tensor [6]; of a batch of full-length clips ([B, T]) as
    [B, 6].  float64 is the reference; float32 (on any device) is the restatement whose time tools/metrics_times.py puts
    beside the kernel's."""
    px, py = power(x, n_fft, hop, win, dtype), power(y, n_fft, hop, win, dtype)
    mx, my = torch.sqrt(px.clamp_min(FLOOR)), torch.sqrt(py.clamp_min(FLOOR))
    out = torch.zeros(x.shape[:-1] + (6,), dtype=dtype, device=x.device)
    out[..., 0] = ((my - mx) ** 2).sum(dim=(-2, -1))
    out[..., 1] = (my ** 2).sum(dim=(-2, -1))
    out[..., 2] = (torch.log(my) - torch.log(mx)).abs().sum(dim=(-2, -1))
    out[..., 3] = torch.sqrt(((torch.log10(my ** 2) - torch.log10(mx ** 2)) ** 2).mean(dim=-2)).sum(dim=-1)
    if basis is not None:
        basis = basis.to(device=x.device, dtype=dtype)
        lx = torch.log((basis @ torch.sqrt(px)).clamp_min(CLIP))
        ly = torch.log((basis @ torch.sqrt(py)).clamp_min(CLIP))
        out[..., 4] = (ly - lx).abs().sum(dim=(-2, -1))
        if n_cep:
            D = cepstral_table(n_cep, basis.shape[0]).to(device=x.device, dtype=dtype)
            out[..., 5] = torch.linalg.vector_norm(D @ (ly - lx), dim=-2).sum(dim=-1)
    return out


def metrics(x, y, resolutions=RESOLUTIONS, mel_resolution=MEL_RESOLUTION, basis=None, n_cep=13):
    """Every metric of ``spectral_metrics`` for one clip pair (x, y [T]): a dict of Python floats."""
    basis = default_basis() if basis is None else basis
    T = x.shape[0]
    out, total = {}, 0.0
    for r in resolutions:
        s = sums(x, y, *r)
        sc = math.sqrt(float(s[0]) / float(s[1]))
        mag = float(s[2]) / ((T // r[1] + 1) * (r[0] // 2 + 1))
        out["sc_{}_{}_{}".format(*r)], out["mag_{}_{}_{}".format(*r)] = sc, mag
        total += sc + mag
    out["mr_stft"] = total / len(resolutions)
    s = sums(x, y, *mel_resolution, basis=basis, n_cep=n_cep)
    frames = T // mel_resolution[1] + 1
    out["ls_mae"] = float(s[4]) / (frames * basis.shape[0])
    out["lsd"] = float(s[3]) / frames
    out["mcd"] = MCD_DB * float(s[5]) / frames
    return out


def close(got, want, key):
    """|got - want| <= RTOL |want| + ATOL (ATOL_MCD for mcd)."""
    atol = ATOL_MCD if key == "mcd" else ATOL
    return abs(float(got) - float(want)) <= RTOL * abs(float(want)) + atol


# ---- the signals of the parity tests: seeded in float64, cast to float32
KINDS = ("noise", "gain", "silence", "xsilent")
LENGTHS = (4000, 2500, 1300, 1025)          # 1025: the shortest clip n_fft = 2048 admits


def signal_pair(kind, length, seed=11):
    """(x, y) float32 [length]: y two sines in noise, x one of four distortions of it."""
    gen = torch.Generator().manual_seed(seed * 7919 + length)
    t = torch.arange(length, dtype=torch.float64)
    y = 0.3 * torch.sin(2 * math.pi * 440 * t / 22050) + 0.2 * torch.sin(2 * math.pi * 3000 * t / 22050) \
        + 0.05 * torch.randn(length, generator=gen, dtype=torch.float64)
    extra = torch.randn(length, generator=gen, dtype=torch.float64)
    if kind == "noise":
        x = y + 0.05 * extra
    elif kind == "gain":
        x = 0.5 * y
    elif kind == "silence":     # both exactly zero on samples 300 .. 2899, x quieter before and noisier behind
        x = y.clone()
        x[:300] *= 0.7
        x[2900:] += 0.02 * extra[2900:]
        x[300:2900] = 0.0
        y[300:2900] = 0.0
    elif kind == "xsilent":
        x = torch.zeros_like(y)
    else:
        raise KeyError(kind)
    return x.float(), y.float()

"""The adaptive prior (PriorGrad: Lee et al., ICLR 2022) in numpy float64, written from the definitions alone and
independently of the package: the yardstick of tests/test_prior*.py.

    energy[b, f]   = sqrt(sum_k exp(m[b, k, f]))
    sigma_f[b, f]  = clamp((energy[b, f] - e_min) / (e_max - e_min), std_min, 1)
    sigma[b, 0, l] = sigma_f[b, l // hop]            l = 0 .. L-1
    x_t  = sqrt(abar_t) x_0 + sqrt(1 - abar_t) (sigma z)
    loss = mean(((eps_theta - sigma z) / sigma)^2)
"""
import numpy as np


def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64)


def energy(mel):
    """[B, bands, frames] -> [B, frames]"""
    return np.sqrt(np.exp(_f64(mel)).sum(axis=1))


def prior_std(mel, hop, L=None, *, energy_max, energy_min=0.0, std_min=0.1):
    """[B, bands, frames] -> [B, 1, L]"""
    e = energy(mel)
    sf = np.clip((e - float(energy_min)) / (float(energy_max) - float(energy_min)), float(std_min), 1.0)
    L = e.shape[1] * hop if L is None else L
    idx = np.arange(L) // hop
    return sf[:, None, idx]


def q_sample(x0, abar_t, z, sigma):
    """abar_t [B, 1, 1]"""
    x0, abar_t, z, sigma = _f64(x0), _f64(abar_t), _f64(z), _f64(sigma)
    return np.sqrt(abar_t) * x0 + np.sqrt(1.0 - abar_t) * (sigma * z)


def loss(eps_theta, z, sigma):
    eps_theta, z, sigma = _f64(eps_theta), _f64(z), _f64(sigma)
    return float(np.mean(((eps_theta - sigma * z) / sigma) ** 2))

"""Float64 reference of the guided (DPS) sampler, independent of `sampling.sampling_guided`: the loop of the issue
written out with torch autograd through the CPU oracle.  Shared by tests/test_guided_sampling.py (CPU) and
tests/test_guided_sampling_gpu.py.

Per step s = S-1..0:  eps = net(x, t_s);  u = (x - k1 eps) / k2;  n_b = ||y_b - A(u)_b||;  g = d(sum n_b)/dx;
x = update(x, eps, z_s) - scale g, with update the plain DDIM step (k1..k5 of `ddim_coefficients`) or the reference's
DDPM step (`generate.py:51-54`) on Alpha / Alpha_bar / Sigma; k1 = sqrt(1 - Alpha_bar), k2 = sqrt(Alpha_bar) there."""
import numpy as np
import torch

from oracle import sashimi as osa
from oracle import wavenet as own


def oracle_net(cfg, sd, dtype, mel=None):
    """Differentiable `net((x, t), mel_spec=None)` through the CPU oracle with `sd` in `dtype`."""
    fwd = own.wavenet_forward if cfg["_name_"] == "wavenet" else osa.sashimi_forward
    sdd = {k: (v.detach().to(dtype) if v.is_floating_point() else v.detach().clone()) for k, v in sd.items()}

    def net(inp, mel_spec=None):
        m = mel if mel_spec is None else mel_spec
        return fwd(sdd, cfg, inp[0].to(dtype), inp[1], mel_spec=None if m is None else m.to(dtype))
    return net


def reference_guided(net, size, dh, *, y, operator, scale, sampler, steps=None, eta=0.0, x_T, noise, residuals=None):
    """The float64 loop; `scale = 0` gives the unguided run (and still records the residuals)."""
    from diffwave_sashimi_amd.sampling import ddim_coefficients, ddim_steps
    B = size[0]
    x = x_T.double().clone()
    y = y.double()
    if sampler == "ddim":
        tau = ddim_steps(dh["T"], steps)
        k = ddim_coefficients(dh["Alpha_bar"], tau, eta).astype(np.float64)
    else:
        tau = list(range(dh["T"]))
        A_, Ab, Sg = (dh[n].double() for n in ("Alpha", "Alpha_bar", "Sigma"))
    for s in range(len(tau) - 1, -1, -1):
        xin = x.clone().requires_grad_(True)
        eps = net((xin, torch.full((B, 1), float(tau[s]))))
        if sampler == "ddim":
            u = (xin - k[0, s] * eps) / k[1, s]
            new, sigma = k[2, s] * u + k[3, s] * eps, k[4, s]
        else:
            u = (xin - torch.sqrt(1 - Ab[s]) * eps) / torch.sqrt(Ab[s])
            new, sigma = (xin - (1 - A_[s]) / torch.sqrt(1 - Ab[s]) * eps) / torch.sqrt(A_[s]), Sg[s]
        n = torch.linalg.vector_norm((y - operator(u)).reshape(B, -1), dim=1)
        (g,) = torch.autograd.grad(n.sum(), xin)
        if residuals is not None:
            residuals.append(n.detach())
        x = new.detach()
        if s > 0:
            x = x + sigma * noise[s].double()
        x = x - scale * g
    return x

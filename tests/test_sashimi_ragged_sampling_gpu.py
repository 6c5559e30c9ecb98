"""GPU: the samplers on a ragged SaShiMi batch (``lengths=``; mel-conditional ``ss_cond_d32``, a mel per clip).  Every
sampler entry against its per-step loop written out with module calls carrying the same ``lengths`` and the numpy float32
update the other sampler tests use (bit for bit over the valid region), the zero padding of the result, the graph cache (the
S4 convolutions read the length table from device memory: a new table replays the captured step), the independence of a
clip from the batch around it under per-clip seeds, and the known samples of an inpainting run."""
import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu

S = 6
L_MAX, LENS = 1024, [1024, 768, 256, 16]          # 4, 3, 1 and 1 mel frames of 256 samples; 16 = the pooling factors' product
B = len(LENS)


def _net(gpu):
    cfg, _, _, wseed, _, _ = cases.SASHIMI_COND_CASES["ss_cond_d32"]
    return cases.build_ours(cfg, wseed).to(gpu)


def _mel(gpu, rows=None):
    mel = cases.mel_inputs(B, 4, 172)              # random in the frames behind a clip's own, too
    return (mel if rows is None else mel[rows]).to(gpu)


def _inputs(seed=77):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 1, L_MAX, generator=g), torch.randn(S, B, 1, L_MAX, generator=g)


def _eps(net, x, t, gpu, lens, mel):
    with torch.no_grad():
        return net((torch.from_numpy(x).to(gpu), torch.full((x.shape[0], 1), float(t), device=gpu)), mel_spec=mel,
                   lengths=lens).cpu().numpy()


def _graphs(net):
    net._ensure_handle()
    return int(net.read_tap("sampler_graphs", (1,)).item())


def _ddpm_loop(net, dh, steps, x_T, noise, gpu, lens, mel):
    al, ab, sg = (dh[k] for k in ("Alpha", "Alpha_bar", "Sigma"))
    x = x_T.numpy().copy()
    for s in range(len(steps) - 1, -1, -1):
        eps = _eps(net, x, steps[s], gpu, lens, mel)
        a_t, ab_t = np.float32(al[s]), np.float32(ab[s])
        c1 = (np.float32(1) - a_t) / np.sqrt(np.float32(1) - ab_t)
        x = (x - c1 * eps) / np.sqrt(a_t)
        if s > 0:
            x = x + np.float32(sg[s]) * noise[s].numpy()
    assert x.dtype == np.float32
    return torch.from_numpy(x).to(gpu)


def _ddim_loop(net, k, tau, x_T, noise, gpu, lens, mel):
    x = x_T.numpy().copy()
    for s in range(len(tau) - 1, -1, -1):
        eps = _eps(net, x, float(tau[s]), gpu, lens, mel)
        k1, k2, k3, k4, k5 = (np.float32(v) for v in k[:, s])
        u = (x - k1 * eps) / k2
        x = k3 * u + k4 * eps
        if s > 0 and k5 > 0:
            x = x + k5 * noise[s].numpy()
    assert x.dtype == np.float32
    return torch.from_numpy(x).to(gpu)


def _dpmpp_loop(net, m, tau, x_T, gpu, lens, mel):
    x, hist = x_T.numpy().copy(), None
    for s in range(len(tau) - 1, -1, -1):
        eps = _eps(net, x, float(tau[s]), gpu, lens, mel)
        m1, m2, m3, m4, m5 = (np.float32(c) for c in m[:, s])
        p = m1 * eps
        d = x - p
        x0 = d / m2
        D = x0
        if hist is not None and m5 != 0:
            g = x0 - hist
            e = m5 * g
            D = x0 + e
        a_, b_ = m3 * x, m4 * D
        x = a_ + b_
        hist = x0
    assert x.dtype == np.float32
    return torch.from_numpy(x).to(gpu)


def _check(got, want, what):
    for b, n in enumerate(LENS):
        assert torch.equal(got[b, :, :n], want[b, :, :n]), (what, b, float((got[b, :, :n] - want[b, :, :n]).abs().max()))
        assert torch.count_nonzero(got[b, :, n:]) == 0, (what, b)
    assert torch.isfinite(got).all()


@pytest.mark.parametrize("kind", ["ddpm", "ddpm-schedule", "ddim-eta0", "ddim-eta0.5", "dpmpp2m"])
def test_ragged_sampler_equals_its_per_step_loop(gpu, kind):
    from diffwave_sashimi_amd.sampling import (calc_diffusion_hyperparams, ddim_coefficients, ddim_steps, dpmpp_coefficients,
                                               logsnr_steps, sampling, sampling_ddim, sampling_dpmpp)
    net, mel = _net(gpu), _mel(gpu)
    x_T, noise = _inputs()
    size = (B, 1, L_MAX)
    if kind.startswith("ddpm"):
        dh = calc_diffusion_hyperparams(S, 1e-4, 0.05)
        steps = np.arange(S, dtype=np.float32)
        want = _ddpm_loop(net, dh, steps, x_T, noise, gpu, LENS, mel)
        kw = dict(net_steps=steps) if kind == "ddpm-schedule" else {}      # else the full-T entry (dws_sampler_run)
        run = lambda g: sampling(net, size, dh, condition=mel, x_T=x_T, noise=noise, use_graph=g, lengths=LENS, **kw)
    elif kind.startswith("ddim"):
        eta = float(kind.split("eta")[1])
        dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
        tau = ddim_steps(50, S)
        want = _ddim_loop(net, ddim_coefficients(dh["Alpha_bar"], tau, eta), tau, x_T, noise, gpu, LENS, mel)
        run = lambda g: sampling_ddim(net, size, dh, S, eta, condition=mel, x_T=x_T, noise=noise, use_graph=g, lengths=LENS)
    else:
        dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
        tau = logsnr_steps(dh["Alpha_bar"], S)
        want = _dpmpp_loop(net, dpmpp_coefficients(dh["Alpha_bar"], tau), tau, x_T, gpu, LENS, mel)
        run = lambda g: sampling_dpmpp(net, size, dh, S, condition=mel, x_T=x_T, use_graph=g, lengths=torch.tensor(LENS))
    for use_graph in (True, False):
        _check(run(use_graph), want, (kind, use_graph))


def test_a_new_length_table_replays_the_captured_step(gpu):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling_ddim
    net, mel = _net(gpu), _mel(gpu)
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    size = (B, 1, L_MAX)
    other = [16, 1024, 1008, 256]
    run = lambda lens: sampling_ddim(net, size, dh, S, 0.5, condition=mel, seed=11, lengths=lens)
    a = run(LENS)
    g1 = _graphs(net)
    b = run(other)
    assert _graphs(net) == g1                                   # another table at the same (B, L): a replay
    for i, n in enumerate(other):
        assert torch.count_nonzero(b[i, :, n:]) == 0 and torch.count_nonzero(b[i, :, :n]) > 0
    plain = run(None)                                           # lengths off: a graph of its own
    g2 = _graphs(net)
    assert g2 <= g1 + 1
    assert torch.equal(run(LENS), a) and torch.equal(run(None), plain)
    assert _graphs(net) == g2                                   # off and on again: nothing new is captured
    assert torch.count_nonzero(plain[3, :, 16:]) > 0


def test_clip_with_its_own_seed_does_not_depend_on_the_batch(gpu):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling, sampling_ddim
    net = _net(gpu)
    seeds = [101, 202, 303, 404]
    dh50, dh6 = calc_diffusion_hyperparams(50, 1e-4, 0.05), calc_diffusion_hyperparams(S, 1e-4, 0.05)
    runs = {"ddim": lambda sz, sd, ln, m: sampling_ddim(net, sz, dh50, S, 0.5, condition=m, seed=sd, lengths=ln),
            "ddpm": lambda sz, sd, ln, m: sampling(net, sz, dh6, condition=m, seed=sd, lengths=ln)}
    for what, run in runs.items():
        got = run((B, 1, L_MAX), seeds, LENS, _mel(gpu))
        for b, n in enumerate(LENS):
            one = run((1, 1, L_MAX), [seeds[b]], [n], _mel(gpu, slice(b, b + 1)))
            assert torch.equal(got[b], one[0]), (what, b)
            assert torch.count_nonzero(got[b, :, n:]) == 0


def test_inpainting_keeps_the_known_samples_of_every_clip(gpu):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling_ddim
    net, mel = _net(gpu), _mel(gpu)
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    g = torch.Generator().manual_seed(5)
    known = torch.randn(B, 1, L_MAX, generator=g)
    mask = torch.zeros(B, 1, L_MAX, dtype=torch.bool)
    for b, n in enumerate(LENS):
        mask[b, :, :max(n // 2, 1)] = True                      # inside the valid region of every clip
    for use_graph in (True, False):
        x = sampling_ddim(net, (B, 1, L_MAX), dh, S, 0.5, condition=mel, seed=3, known=known, mask=mask, lengths=LENS,
                          use_graph=use_graph).cpu()
        assert torch.equal(x[mask], known[mask])
        for b, n in enumerate(LENS):
            assert torch.count_nonzero(x[b, :, n:]) == 0
            assert not torch.equal(x[b, :, :n], known[b, :, :n])

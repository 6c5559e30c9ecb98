"""GPU: the few-step samplers of `dws_sampler_run_schedule` -- DiffWave's fast schedule with the network at the aligned
fractional steps, and DDIM -- against their per-step loops written out with module calls and a numpy float32 update
(bit for bit), against the float64 oracle, and the step-table / graph caches behind them.  Not the reference's loop:
these pin the arithmetic, not the audio (no trained weights exist offline)."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.conftest import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

SIX = [1e-4, 1e-3, 1e-2, 0.05, 0.2, 0.5]     # DiffWave's fast inference schedule for T = 50, beta in [1e-4, 0.05]


def _net(kind, gpu):
    """(net, B, L, mel) of a small model of each kind."""
    if kind == "wavenet":
        cfg, B, L, wseed, _, _ = cases.WAVENET_CASES["wn_c64"]
        return cases.build_ours(cfg, wseed).to(gpu), B, L, None
    if kind == "sashimi":
        cfg = cases.ss_cfg(d_model=32, n_layers=2, L=1024, diffusion_step_embed_dim_mid=64)
        return cases.build_ours(cfg, 5).to(gpu), 3, 1024, None
    cfg, B, Tmel, wseed, iseed, _ = cases.SASHIMI_COND_CASES["ss_cond_d32"]
    return cases.build_ours(cfg, wseed).to(gpu), B, Tmel * 256, cases.mel_inputs(B, Tmel, iseed).to(gpu)


def _inputs(B, L, S, seed=77):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 1, L, generator=g), torch.randn(S, B, 1, L, generator=g)


def _eps(net, x, t, gpu, mel):
    with torch.no_grad():
        return net((torch.from_numpy(x).to(gpu), torch.full((x.shape[0], 1), float(t), device=gpu)),
                   mel_spec=mel).cpu().numpy()


def _ddpm_loop(net, dh, steps, x_T, noise, gpu, mel=None):
    """DDPM update of `dh` with the network at steps[s]: numpy float32, every operation rounded once, as the engine."""
    al, ab, sg = (dh[k] for k in ("Alpha", "Alpha_bar", "Sigma"))
    x = x_T.numpy().copy()
    for s in range(len(steps) - 1, -1, -1):
        eps = _eps(net, x, steps[s], gpu, mel)
        a_t, ab_t = np.float32(al[s]), np.float32(ab[s])
        c1 = (np.float32(1) - a_t) / np.sqrt(np.float32(1) - ab_t)
        x = (x - c1 * eps) / np.sqrt(a_t)
        if s > 0:
            x = x + np.float32(sg[s]) * noise[s].numpy()
    assert x.dtype == np.float32
    return torch.from_numpy(x).to(gpu)


def _ddim_loop(net, k, tau, x_T, noise, gpu, mel=None):
    """u = (x - k1 eps) / k2; x = k3 u + k4 eps; + k5 z for s > 0 and k5 > 0 -- numpy float32, in this order."""
    x = x_T.numpy().copy()
    for s in range(len(tau) - 1, -1, -1):
        eps = _eps(net, x, float(tau[s]), gpu, mel)
        k1, k2, k3, k4, k5 = (np.float32(v) for v in k[:, s])
        u = (x - k1 * eps) / k2
        x = k3 * u + k4 * eps
        if s > 0 and k5 > 0:
            x = x + k5 * noise[s].numpy()
    assert x.dtype == np.float32
    return torch.from_numpy(x).to(gpu)


def _graphs(net):
    net._ensure_handle()
    return int(net.read_tap("sampler_graphs", (1,)).item())


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_identity_steps_reproduce_the_plain_sampler(gpu, kind):
    """net_steps = align_steps of the training schedule itself = 0..T-1: bit-identical to sampling() -- seed-driven
    (same Philox streams for x_T and z) and with injected noise, graph and eager."""
    from diffwave_sashimi_amd.sampling import align_steps, calc_diffusion_hyperparams, sampling
    net, B, L, _ = _net(kind, gpu)
    T = 6
    dh = calc_diffusion_hyperparams(T, 1e-4, 0.05)
    steps = align_steps(T, 1e-4, 0.05, np.linspace(1e-4, 0.05, T))
    x_T, noise = _inputs(B, L, T)
    for use_graph in (True, False):
        a = sampling(net, (B, 1, L), dh, seed=5, use_graph=use_graph)
        b = sampling(net, (B, 1, L), dh, seed=5, use_graph=use_graph, net_steps=steps)
        assert torch.equal(a, b), (use_graph, float((a - b).abs().max()))
        a = sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise, use_graph=use_graph)
        b = sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise, use_graph=use_graph, net_steps=steps)
        assert torch.equal(a, b), (use_graph, float((a - b).abs().max()))


@pytest.mark.parametrize("kind", ["wavenet", "sashimi", "sashimi_cond"])
def test_aligned_sampler_equals_its_per_step_loop(gpu, kind):
    """Six fractional steps (the six-beta list on T = 50): the step table at those values, the reference's update
    tables of the short list -- equal to the loop of module calls, bit for bit, graph and eager."""
    from diffwave_sashimi_amd.sampling import align_steps, calc_diffusion_hyperparams, sampling, sampling_aligned
    net, B, L, mel = _net(kind, gpu)
    cfg = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=SIX)
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05, beta=SIX, fast=True)
    steps = align_steps(50, 1e-4, 0.05, SIX)
    assert np.any(steps != np.round(steps))
    x_T, noise = _inputs(B, L, 6)
    want = _ddpm_loop(net, dh, steps, x_T, noise, gpu, mel)
    for use_graph in (True, False):
        got = sampling_aligned(net, (B, 1, L), cfg, mel, x_T=x_T, noise=noise, use_graph=use_graph)
        assert torch.equal(got, want), (use_graph, float((got - want).abs().max()))
    # the reference's own short loop (integer steps 0..5) is another trajectory
    plain = sampling(net, (B, 1, L), dh, mel, x_T=x_T, noise=noise)
    assert not torch.equal(plain, want)


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_ddim_equals_its_per_step_loop(gpu, kind, eta):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, ddim_coefficients, ddim_steps, sampling_ddim
    net, B, L, _ = _net(kind, gpu)
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    tau = ddim_steps(50, 8)
    k = ddim_coefficients(dh["Alpha_bar"], tau, eta)
    x_T, noise = _inputs(B, L, 8)
    want = _ddim_loop(net, k, tau, x_T, noise, gpu)
    got = sampling_ddim(net, (B, 1, L), dh, 8, eta, x_T=x_T, noise=noise, use_graph=True)
    eager = sampling_ddim(net, (B, 1, L), dh, 8, eta, x_T=x_T, noise=noise, use_graph=False)
    assert torch.equal(got, want), float((got - want).abs().max())
    assert torch.equal(eager, got)
    # seed-driven: graph == eager, finite
    a = sampling_ddim(net, (B, 1, L), dh, 8, eta, seed=3, use_graph=True)
    b = sampling_ddim(net, (B, 1, L), dh, 8, eta, seed=3, use_graph=False)
    assert torch.equal(a, b) and torch.isfinite(a).all()


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_ddim_eta1_over_every_step_is_ddpm(gpu, kind):
    """DDIM(eta = 1, tau = 0..T-1) is the DDPM posterior step: within 1e-4 of sampling() with the same noise (an index
    error in p_s = abar[tau_{s-1}] would be far off)."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling, sampling_ddim
    net, B, L, _ = _net(kind, gpu)
    T = 20
    dh = calc_diffusion_hyperparams(T, 1e-4, 0.05)
    x_T, noise = _inputs(B, L, T)
    ddpm = sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise)
    ddim = sampling_ddim(net, (B, 1, L), dh, list(range(T)), 1.0, x_T=x_T, noise=noise)
    err = rel_err(ddim, ddpm)
    assert err < 1e-4, err


def test_aligned_trajectory_matches_the_float64_oracle(gpu):
    from diffwave_sashimi_amd.sampling import align_steps, calc_diffusion_hyperparams, sampling
    from oracle import wavenet as own
    cfg, B, L, wseed, _, _ = cases.WAVENET_CASES["wn_tiny"]
    net = cases.build_ours(cfg, wseed).to(gpu)
    sd64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu())
            for k, v in net.state_dict().items()}
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05, beta=SIX, fast=True)
    steps = align_steps(50, 1e-4, 0.05, SIX)
    x_T, noise = _inputs(B, L, 6)
    got = sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise, net_steps=steps)
    al, ab, sg = (dh[k].double() for k in ("Alpha", "Alpha_bar", "Sigma"))
    x = x_T.double()
    with torch.no_grad():
        for s in range(5, -1, -1):
            eps = own.wavenet_forward(sd64, cfg, x, torch.full((B, 1), float(steps[s]), dtype=torch.float64))
            x = (x - (1 - al[s]) / torch.sqrt(1 - ab[s]) * eps) / torch.sqrt(al[s])
            if s > 0:
                x = x + sg[s] * noise[s].double()
    err = rel_err(got, x)
    assert err < REL_TOL, err


def test_step_table_follows_the_step_values_and_the_weights(gpu):
    from diffwave_sashimi_amd.sampling import align_steps, calc_diffusion_hyperparams, sampling
    cfg, B, L, wseed, _, _ = cases.WAVENET_CASES["wn_c64"]
    net = cases.build_ours(cfg, wseed).to(gpu)
    other = [2e-4, 2e-3, 2e-2, 0.08, 0.3, 0.5]
    dh_a = calc_diffusion_hyperparams(50, 1e-4, 0.05, beta=SIX, fast=True)
    dh_b = calc_diffusion_hyperparams(50, 1e-4, 0.05, beta=other, fast=True)
    st_a, st_b = align_steps(50, 1e-4, 0.05, SIX), align_steps(50, 1e-4, 0.05, other)
    dh6 = calc_diffusion_hyperparams(6, 1e-4, 0.05)
    x_T, noise = _inputs(B, L, 6)
    run = lambda n, dh, st: sampling(n, (B, 1, L), dh, x_T=x_T, noise=noise, net_steps=st)
    fresh = lambda: cases.build_ours(cfg, wseed).to(gpu)
    want_a, want_b = run(fresh(), dh_a, st_a), run(fresh(), dh_a, st_b)
    want_plain = sampling(fresh(), (B, 1, L), dh6, x_T=x_T, noise=noise)
    # same S, other step values: rebuilt (a stale table would reproduce the first trajectory)
    assert torch.equal(run(net, dh_a, st_a), want_a)
    assert torch.equal(run(net, dh_a, st_b), want_b) and not torch.equal(want_a, want_b)
    # plain T = 6 (integer rows) alternating with aligned S = 6 on one model
    for _ in range(2):
        assert torch.equal(sampling(net, (B, 1, L), dh6, x_T=x_T, noise=noise), want_plain)
        assert torch.equal(run(net, dh_b, st_a), run(fresh(), dh_b, st_a))
    # new weights, same steps: rebuilt
    with torch.no_grad():
        for p_ in net.parameters():
            if p_.is_floating_point():
                p_.mul_(1.01)
    got = run(net, dh_a, st_a)
    assert torch.equal(got, _ddpm_loop(net, dh_a, st_a, x_T, noise, gpu)) and not torch.equal(got, want_a)


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_one_graph_per_shape_not_per_call(gpu, kind):
    """A new seed and a new output tensor replay the graph already captured: the count of instantiated graphs rises on
    the first call of each (shape, schedule) only; results differ by seed and equal the eager results."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling_aligned, sampling_ddim
    net, B, L, _ = _net(kind, gpu)
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    cfg = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=SIX)
    runs = (lambda seed, g: sampling_ddim(net, (B, 1, L), dh, 8, 0.5, seed=seed, use_graph=g),
            lambda seed, g: sampling_aligned(net, (B, 1, L), cfg, seed=seed, use_graph=g))
    for run in runs:
        n0 = _graphs(net)
        a = run(11, True)
        n1 = _graphs(net)
        b = run(12, True)
        assert n1 == n0 + 1 and _graphs(net) == n1
        assert not torch.equal(a, b) and a.data_ptr() != b.data_ptr()
        assert torch.equal(a, run(11, False)) and torch.equal(b, run(12, False))
        # the eager calls kept the table: the graph is still the current one
        n2 = _graphs(net)
        assert torch.equal(run(11, True), a) and _graphs(net) == n2


@pytest.mark.parametrize("precision", ["f32", "bf16x6"])
def test_aligned_at_the_vocoder_size(gpu, precision):
    """BASELINE config 4's network and shape (unet_d32_n6 cond, B = 32, L = 16000, mel [1, 80, 63]), aligned S = 6."""
    from diffwave_sashimi_amd.sampling import align_steps, calc_diffusion_hyperparams, sampling_aligned
    cfg, _, Tmel, wseed, iseed = cases.SASHIMI_C4
    B, L = 32, 16000
    net = cases.build_ours(cfg, wseed).to(gpu)
    mel = cases.mel_inputs(1, Tmel, iseed).to(gpu)
    dcfg = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=SIX)
    x_T, noise = _inputs(B, L, 6)
    f32 = sampling_aligned(net, (B, 1, L), dcfg, mel, x_T=x_T, noise=noise)
    if precision == "f32":
        dh = calc_diffusion_hyperparams(50, 1e-4, 0.05, beta=SIX, fast=True)
        want = _ddpm_loop(net, dh, align_steps(50, 1e-4, 0.05, SIX), x_T, noise, gpu, mel)
        assert torch.equal(f32, want), float((f32 - want).abs().max())
    else:
        net.set_option("precision", "bf16x6")
        got = sampling_aligned(net, (B, 1, L), dcfg, mel, x_T=x_T, noise=noise)
        assert torch.isfinite(got).all()
        err = rel_err(got, f32)
        assert err < 1e-5, err


@pytest.mark.parametrize("sampler", ["aligned", "ddim"])
def test_generate_cli_few_step_samplers(tmp_path, gpu, sampler):
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import _worker, load_config, local_path_name
    from tests.test_generate_cli import _tree
    d = _tree(tmp_path / "conf")
    ov = ["model=wavenet", "model.res_channels=64", "model.skip_channels=64", "model.num_res_layers=4",
          "model.dilation_cycle=4", "dataset.segment_length=1600", "generate.n_samples=2", "generate.ckpt_iter=init",
          "generate.seed=4"]
    if sampler == "aligned":
        ov += ["generate.sampler=aligned", "diffusion.beta=[0.0001,0.001,0.01,0.05,0.2,0.5]"]
    else:
        ov += ["generate.sampler=ddim", "generate.steps=8"]
    cfg = load_config(d, ov)
    root = str(tmp_path / "exp")
    _worker(0, cfg, root)
    outdir = os.path.join(root, local_path_name(None, cfg["model"], cfg["diffusion"], cfg["dataset"]), "waveforms", "0")
    assert sorted(os.listdir(outdir)) == ["0k_0.wav", "0k_1.wav"]
    for f in ("0k_0.wav", "0k_1.wav"):
        sr, w = wavfile.read(os.path.join(outdir, f))
        assert sr == 16000 and w.dtype == np.float32 and w.shape == (1600,) and np.isfinite(w).all()

"""GPU: `sampling.sampling_guided` on the engine -- every step a training forward and a data-only backward
(`dws_model_backward_input`) -- against the float64 loop through the CPU oracle (tests/guided_reference.py) on the same
weights, x_T and noise: <= 1e-3 of max|x| (the project's rule; a six-step fp32 loop sits 2e-7 .. 3e-7 from its float64
twin, the guidance moves the result by 1e-2 .. 1e-1)."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.conftest import REL_TOL, rel_err
from tests.guided_reference import oracle_net, reference_guided

pytestmark = pytest.mark.gpu

WN = cases.wn_cfg(res_channels=64, skip_channels=64, num_res_layers=3, dilation_cycle=3)
SS = cases.ss_cfg(d_model=32, n_layers=1, L=1024, diffusion_step_embed_dim_mid=64)
SS_COND = cases.ss_cfg(unconditional=False, d_model=32, n_layers=1, L=1024, mel_upsample=[16, 16],
                       diffusion_step_embed_dim_mid=64)
MODELS = {"wavenet": (WN, 2, 200, 5), "sashimi": (SS, 2, 1024, 15), "sashimi_cond": (SS_COND, 2, 1024, 35)}
BETA6 = [1e-4, 1e-3, 1e-2, 0.05, 0.2, 0.5]
SAMPLERS = {"ddim_eta0": ("ddim", 0.0), "ddim_eta1": ("ddim", 1.0), "ddpm6": ("ddpm", 0.0)}


def _schedule(sampler):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    if sampler == "ddim":
        return calc_diffusion_hyperparams(50, 1e-4, 0.05), 6
    return calc_diffusion_hyperparams(50, 1e-4, 0.05, beta=BETA6, fast=True), None


def _model(name):
    def make():
        cfg, B, L, wseed = MODELS[name]
        net = cases.build_ours(cfg, wseed)
        if cfg["_name_"] == "sashimi":
            net._setup_C()
        return cfg, B, L, wseed, {k: v.detach().clone() for k, v in net.state_dict().items()}
    return cases.cached(("guided_gpu_model", name), make)


def _problem(name, op_name, S=6):
    from diffwave_sashimi_amd.sampling import declip_operator, lowpass_operator
    cfg, B, L, wseed, sd = _model(name)
    g = torch.Generator().manual_seed(41)
    clean = torch.randn(B, 1, L, generator=g) * 0.3
    x_T = torch.randn(B, 1, L, generator=g)
    noise = torch.randn(S, B, 1, L, generator=g)
    op = declip_operator(0.2) if op_name == "declip" else lowpass_operator(2)
    mel = cases.mel_inputs(1, L // 256, 47) if not cfg["unconditional"] else None      # ONE mel for the B clips
    return cfg, B, L, wseed, sd, op, op(clean), x_T, noise, mel


def _reference(name, op_name, sampler_key):
    """Float64 guided run and the unguided one, once per (model, operator, sampler)."""
    def make():
        cfg, B, L, wseed, sd, op, y, x_T, noise, mel = _problem(name, op_name)
        sampler, eta = SAMPLERS[sampler_key]
        dh, steps = _schedule(sampler)
        net64 = oracle_net(cfg, sd, torch.float64, mel=None if mel is None else mel.expand(B, -1, -1))
        run = lambda scale: reference_guided(net64, (B, 1, L), dh, y=y, operator=op, scale=scale, sampler=sampler,
                                             steps=steps, eta=eta, x_T=x_T, noise=noise)
        return run(0.5), run(0.0)
    return cases.cached(("guided_gpu_reference", name, op_name, sampler_key), make)


def _engine(name, gpu, precision="f32"):
    cfg, B, L, wseed, sd = _model(name)
    net = cases.build_ours(cfg, wseed)
    if cfg["_name_"] == "sashimi":
        net._setup_C()      # (as _model did: the state dict the oracle runs on)
    net = net.to(gpu).eval()
    net.set_option("precision", precision)
    return net


@pytest.mark.parametrize("precision", ["f32", "bf16x6"])
@pytest.mark.parametrize("sampler_key", list(SAMPLERS))
@pytest.mark.parametrize("op_name", ["declip", "lowpass"])
@pytest.mark.parametrize("name", ["wavenet", "sashimi"])
def test_engine_guided_run_matches_the_float64_oracle_loop(gpu, name, op_name, sampler_key, precision):
    from diffwave_sashimi_amd.sampling import sampling_guided
    cfg, B, L, wseed, sd, op, y, x_T, noise, mel = _problem(name, op_name)
    sampler, eta = SAMPLERS[sampler_key]
    dh, steps = _schedule(sampler)
    ref, plain = _reference(name, op_name, sampler_key)
    net = _engine(name, gpu, precision)
    got = sampling_guided(net, (B, 1, L), dh, measurement=y.to(gpu), operator=op, scale=0.5, sampler=sampler, steps=steps,
                          eta=eta, x_T=x_T.to(gpu), noise=noise.to(gpu))
    assert got.device.type == "cuda" and got.shape == (B, 1, L) and torch.isfinite(got).all()
    err, moved = rel_err(got.cpu(), ref), rel_err(plain, ref)
    print(f"{name} {op_name} {sampler_key} {precision}: engine vs float64 loop {err:.2e} (guidance moves the result by {moved:.2e})")
    assert err <= REL_TOL
    assert moved > 10 * REL_TOL          # the bound tells a guided run from an unguided one
    assert all(p.grad is None for p in net.parameters())


@pytest.mark.parametrize("precision", ["f32", "bf16x6"])
def test_engine_guided_run_with_one_mel_for_the_batch(gpu, precision):
    from diffwave_sashimi_amd.sampling import sampling_guided
    name, op_name, sampler_key = "sashimi_cond", "lowpass", "ddim_eta1"
    cfg, B, L, wseed, sd, op, y, x_T, noise, mel = _problem(name, op_name)
    assert mel.shape[0] == 1 and B == 2
    dh, steps = _schedule("ddim")
    ref, plain = _reference(name, op_name, sampler_key)
    net = _engine(name, gpu, precision)
    got = sampling_guided(net, (B, 1, L), dh, measurement=y.to(gpu), operator=op, scale=0.5, sampler="ddim", steps=steps,
                          eta=1.0, condition=mel.to(gpu), x_T=x_T.to(gpu), noise=noise.to(gpu))
    err = rel_err(got.cpu(), ref)
    print(f"conditional sashimi, Bm = 1, B = 2, {precision}: engine vs float64 loop {err:.2e}")
    assert err <= REL_TOL and rel_err(plain, ref) > 10 * REL_TOL


@pytest.mark.parametrize("name", ["wavenet", "sashimi"])
def test_seeded_guided_run_is_reproducible_and_leaves_no_state_behind(gpu, name):
    from diffwave_sashimi_amd.sampling import sampling_ddim, sampling_guided
    cfg, B, L, wseed, sd, op, y, x_T, noise, mel = _problem(name, "declip")
    dh, steps = _schedule("ddim")
    net = _engine(name, gpu)
    plain = lambda: sampling_ddim(net, (B, 1, L), dh, steps, eta=1.0, seed=5)
    guided = lambda seed: sampling_guided(net, (B, 1, L), dh, measurement=y.to(gpu), operator=op, scale=0.5, sampler="ddim",
                                          steps=steps, eta=1.0, seed=seed)
    before = plain()
    a, b, c = guided(7), guided(7), guided(8)
    after = plain()
    assert torch.isfinite(a).all() and torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(before, after)
    # the drawn x_T and noise are the plain sampler's Philox streams: with a vanishing guidance step the guided run is
    # the plain one up to the rounding of one more addition per step
    tiny = sampling_guided(net, (B, 1, L), dh, measurement=y.to(gpu), operator=op, scale=1e-12, sampler="ddim", steps=steps,
                           eta=1.0, seed=5)
    assert rel_err(tiny, before) < 1e-4


def test_generate_cli_restores_from_a_degraded_wav(tmp_path, gpu, capsys):
    """checkpoint -> degraded wav -> generate.guide_* -> wav written, network evaluations printed; both samplers."""
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import generate, local_path_name
    cfg = dict(WN)
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=BETA6)
    data = tmp_path / "wavs"
    os.makedirs(data)
    rng = np.random.default_rng(3)
    clean = rng.standard_normal(640).astype(np.float32) * 0.3
    wavfile.write(str(data / "clipped.wav"), 16000, np.clip(clean, -0.2, 0.2))
    ds = dict(_name_="sc09", data_path=str(data), segment_length=640, sampling_rate=16000)
    root = str(tmp_path / "exp")
    run = local_path_name(None, cfg, diff, ds)
    os.makedirs(os.path.join(root, run, "checkpoint"))
    torch.save({"model_state_dict": cases.build_ours(cfg, 5).state_dict()}, os.path.join(root, run, "checkpoint", "1000.pkl"))
    written = []
    a = generate(0, diff, dict(cfg), ds, ckpt_iter="max", n_samples=2, exp_root=root, seed=11, written=written,
                 guide_name="clipped", guide_op="declip", guide_scale=0.5)
    text = capsys.readouterr().out
    assert a.shape == (2, 1, 640) and torch.isfinite(a).all()
    assert "guided sampler ddpm (declip, scale 0.5): 6 network evaluations" in text
    assert len(written) == 2 and all(os.path.exists(f) for f in written)
    sr, w = wavfile.read(written[0])
    assert sr == 16000 and w.dtype == np.float32 and np.array_equal(w, a[0, 0].cpu().numpy())
    again = generate(0, diff, dict(cfg), ds, ckpt_iter="max", n_samples=2, exp_root=root, seed=11,
                     guide_name="clipped", guide_op="declip", guide_scale=0.5)
    assert torch.equal(a, again)
    unguided = generate(0, diff, dict(cfg), ds, ckpt_iter="max", n_samples=2, exp_root=root, seed=11)
    assert not torch.equal(a, unguided)
    capsys.readouterr()
    b = generate(0, diff, dict(cfg), ds, ckpt_iter="max", n_samples=2, exp_root=root, seed=11, sampler="ddim", steps=4,
                 eta=0.5, guide_name="clipped", guide_op="lowpass", guide_factor=2, guide_scale=0.25)
    assert "guided sampler ddim (lowpass, scale 0.25): 4 network evaluations" in capsys.readouterr().out
    assert b.shape == (2, 1, 640) and torch.isfinite(b).all()

"""CPU: the guided (DPS) sampler `sampling.sampling_guided` and its measurement operators, run with the CPU oracle as the
network (the function takes any differentiable `net`): the formula is pinned against an independent float64 loop
(tests/guided_reference.py), <= 1e-5 of max|x| -- an fp32 six-step loop sits 2e-7 .. 3e-7 from its float64 twin, while
the guidance itself moves the result by 3e-2 .. 1e-1."""
import pytest
import torch

from tests import cases
from tests.conftest import rel_err
from tests.guided_reference import oracle_net, reference_guided

WN = cases.wn_cfg(res_channels=64, skip_channels=64, num_res_layers=3, dilation_cycle=3)
SS = cases.ss_cfg(d_model=32, n_layers=1, L=1024, diffusion_step_embed_dim_mid=64)
MODELS = {"wavenet": (WN, 2, 200, 5), "sashimi": (SS, 2, 1024, 15)}


def _model(name):
    def make():
        cfg, B, L, wseed = MODELS[name]
        net = cases.build_ours(cfg, wseed)
        if cfg["_name_"] == "sashimi":
            net._setup_C()
        return cfg, B, L, {k: v.detach().clone() for k, v in net.state_dict().items()}
    return cases.cached(("guided_model", name), make)


def _problem(name, op_name, S=6):
    from diffwave_sashimi_amd.sampling import declip_operator, lowpass_operator
    cfg, B, L, sd = _model(name)
    g = torch.Generator().manual_seed(41)
    clean = torch.randn(B, 1, L, generator=g) * 0.3
    x_T = torch.randn(B, 1, L, generator=g)
    noise = torch.randn(S, B, 1, L, generator=g)
    op = declip_operator(0.2) if op_name == "declip" else lowpass_operator(2)
    return cfg, B, L, sd, op, op(clean), x_T, noise


def test_declip_operator():
    from diffwave_sashimi_amd.sampling import declip_operator
    x = torch.linspace(-1, 1, 41, dtype=torch.float64).reshape(1, 1, 41).requires_grad_(True)
    y = declip_operator(0.25)(x)
    assert y.shape == x.shape and float(y.detach().max()) == 0.25 and float(y.detach().min()) == -0.25
    inside = x.detach().abs() < 0.25
    assert torch.equal(y.detach()[inside], x.detach()[inside])
    (g,) = torch.autograd.grad(y.sum(), x)
    assert torch.equal(g[inside], torch.ones_like(g[inside])) and float(g[x.detach().abs() > 0.25].abs().max()) == 0
    with pytest.raises(ValueError):
        declip_operator(0.0)


@pytest.mark.parametrize("factor,taps,L", [(2, 33, 200), (2, 33, 201), (3, 21, 100), (4, 33, 64), (1, 9, 17)])
def test_lowpass_operator_shape_gain_and_adjoint(factor, taps, L):
    from diffwave_sashimi_amd.sampling import lowpass_operator, lowpass_taps
    h = lowpass_taps(factor, taps)
    assert h.shape == (taps,) and abs(h.sum() - 1.0) < 1e-12 and abs(h - h[::-1]).max() < 1e-15
    A = lowpass_operator(factor, taps)
    n_out = -(-L // factor)
    ones = torch.ones(2, 1, L, dtype=torch.float64)
    y = A(ones)
    assert y.shape == (2, 1, n_out)
    half = (taps - 1) // 2
    inner = [j for j in range(n_out) if j * factor - half >= 0 and j * factor + half < L]      # every tap inside the clip
    if inner:
        assert float((y[..., inner] - 1).abs().max()) < 1e-12        # unit DC gain
    # <A x, v> = <x, A^T v>: A^T v is the autograd gradient of <A x, v>
    g = torch.Generator().manual_seed(factor * 100 + L)
    x = torch.randn(2, 1, L, generator=g, dtype=torch.float64)
    v = torch.randn(2, 1, n_out, generator=g, dtype=torch.float64)
    x0 = torch.zeros_like(x).requires_grad_(True)
    (ATv,) = torch.autograd.grad((A(x0) * v).sum(), x0)
    lhs, rhs = float((A(x) * v).sum()), float((x * ATv).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    # and against the definition at one position
    j = n_out // 2
    want = sum(h[k] * (x[0, 0, j * factor + k - half] if 0 <= j * factor + k - half < L else 0.0) for k in range(taps))
    assert abs(float(A(x)[0, 0, j]) - float(want)) < 1e-12
    with pytest.raises(ValueError):
        lowpass_operator(2, 32)
    with pytest.raises(ValueError):
        lowpass_operator(0)


RUNS = [("wavenet", "declip", "ddim", 0.0), ("wavenet", "lowpass", "ddim", 1.0), ("wavenet", "declip", "ddpm", 0.0),
        ("sashimi", "lowpass", "ddim", 0.0), ("sashimi", "declip", "ddim", 1.0), ("sashimi", "lowpass", "ddpm", 0.0)]


def _schedule(sampler):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    if sampler == "ddim":
        return calc_diffusion_hyperparams(50, 1e-4, 0.05), 6
    return calc_diffusion_hyperparams(50, 1e-4, 0.05, beta=[1e-4, 1e-3, 1e-2, 0.05, 0.2, 0.5], fast=True), None


@pytest.mark.parametrize("model,op_name,sampler,eta", RUNS)
def test_guided_sampler_is_the_float64_loop_and_lowers_the_residual(model, op_name, sampler, eta):
    from diffwave_sashimi_amd.sampling import sampling_guided
    cfg, B, L, sd, op, y, x_T, noise = _problem(model, op_name)
    dh, steps = _schedule(sampler)
    res32 = []
    got = sampling_guided(oracle_net(cfg, sd, torch.float32), (B, 1, L), dh, measurement=y, operator=op, scale=0.5,
                          sampler=sampler, steps=steps, eta=eta, x_T=x_T, noise=noise, residuals=res32)
    net64 = oracle_net(cfg, sd, torch.float64)
    res_g, res_u = [], []
    ref = reference_guided(net64, (B, 1, L), dh, y=y, operator=op, scale=0.5, sampler=sampler, steps=steps, eta=eta,
                           x_T=x_T, noise=noise, residuals=res_g)
    plain = reference_guided(net64, (B, 1, L), dh, y=y, operator=op, scale=0.0, sampler=sampler, steps=steps, eta=eta,
                             x_T=x_T, noise=noise, residuals=res_u)
    err, moved = rel_err(got, ref), rel_err(plain, ref)
    mg, mu = float(torch.stack(res_g).mean()), float(torch.stack(res_u).mean())
    print(f"{model} {op_name} {sampler} eta={eta}: guided vs float64 loop {err:.2e}; guidance moves the result by {moved:.2e}; "
          f"mean residual guided {mg:.4f} / unguided {mu:.4f}")
    assert got.dtype == torch.float32 and got.shape == (B, 1, L)
    assert err <= 1e-5
    assert moved > 30 * 1e-5            # the bound separates "guided" from "not guided"
    assert len(res32) == 6 and rel_err(torch.stack(res32), torch.stack(res_g)) < 1e-5
    assert mg < mu


def test_guided_sampler_draws_its_own_noise_reproducibly_on_the_cpu():
    from diffwave_sashimi_amd.sampling import sampling_guided
    cfg, B, L, sd, op, y, x_T, noise = _problem("wavenet", "declip")
    dh, steps = _schedule("ddim")
    net = oracle_net(cfg, sd, torch.float32)
    run = lambda seed: sampling_guided(net, (B, 1, L), dh, measurement=y, operator=op, scale=0.5, sampler="ddim", steps=3,
                                       eta=1.0, seed=seed)
    a, b, c = run(7), run(7), run(8)
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(a).all()


def test_a_clip_with_zero_residual_gets_no_guidance():
    """y = A(u) exactly for an operator that maps everything to the measurement: n_b = 0, its gradient is taken as 0
    (not the NaN of sqrt at 0), so the run is the unguided one."""
    from diffwave_sashimi_amd.sampling import sampling_guided
    cfg, B, L, sd, op, y, x_T, noise = _problem("wavenet", "declip")
    dh, steps = _schedule("ddim")
    net = oracle_net(cfg, sd, torch.float32)
    zero = lambda u: u * 0.0
    got = sampling_guided(net, (B, 1, L), dh, measurement=torch.zeros(B, 1, L), operator=zero, scale=3.0, sampler="ddim",
                          steps=3, x_T=x_T, noise=noise[:3])
    ref = reference_guided(oracle_net(cfg, sd, torch.float64), (B, 1, L), dh, y=y, operator=op, scale=0.0, sampler="ddim",
                           steps=3, x_T=x_T, noise=noise[:3])
    assert torch.isfinite(got).all() and rel_err(got, ref) < 1e-5


def test_guided_sampler_argument_validation():
    from diffwave_sashimi_amd.sampling import sampling_guided
    cfg, B, L, sd, op, y, x_T, noise = _problem("wavenet", "declip")
    dh, steps = _schedule("ddim")
    net = oracle_net(cfg, sd, torch.float32)
    kw = dict(measurement=y, operator=op, scale=0.5, sampler="ddim", steps=6, x_T=x_T, noise=noise)
    with pytest.raises(ValueError, match="sampling_ddim"):
        sampling_guided(net, (B, 1, L), dh, **dict(kw, scale=0))
    with pytest.raises(ValueError, match="scale"):
        sampling_guided(net, (B, 1, L), dh, **dict(kw, scale=0.0))
    for bad in ("dpmpp2m", "aligned", "euler"):
        with pytest.raises(ValueError, match="sampler"):
            sampling_guided(net, (B, 1, L), dh, **dict(kw, sampler=bad))
    for extra in (dict(known=y, mask=torch.ones(1, 1, L, dtype=torch.bool)), dict(resample=(2, 2)), dict(x_start=y),
                  dict(net_steps=[0.0] * 6)):
        with pytest.raises(ValueError, match="not built"):
            sampling_guided(net, (B, 1, L), dh, **dict(kw, **extra))
    with pytest.raises(TypeError):
        sampling_guided(net, (B, 1, L), dh, **dict(kw, bogus=1))
    with pytest.raises(ValueError, match="steps"):
        sampling_guided(net, (B, 1, L), dh, **dict(kw, steps=None))
    with pytest.raises(ValueError, match="steps"):
        sampling_guided(net, (B, 1, L), dh, **dict(kw, sampler="ddpm", steps=6))
    with pytest.raises(ValueError, match="noise"):
        sampling_guided(net, (B, 1, L), dh, **dict(kw, noise=noise[:5]))
    with pytest.raises(ValueError, match="x_T"):
        sampling_guided(net, (B, 1, L), dh, **dict(kw, x_T=x_T[:1]))
    with pytest.raises(ValueError, match="measurement"):
        sampling_guided(net, (B, 1, L), dh, **dict(kw, measurement=y[..., :50]))


def test_generate_cli_checks_the_guide_keys_before_any_gpu_work(tmp_path):
    from diffwave_sashimi_amd.generate import generate
    diff = dict(T=5, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="sc09", segment_length=640, sampling_rate=16000, data_path=str(tmp_path))
    call = lambda **kw: generate(0, diff, dict(WN), ds, ckpt_iter="init", n_samples=1, exp_root=str(tmp_path / "exp"), **kw)
    with pytest.raises(ValueError, match="guide_name"):
        call(guide_scale=0.5)
    with pytest.raises(ValueError, match="guide_op"):
        call(guide_name="y", guide_scale=0.5)
    with pytest.raises(ValueError, match="guide_scale"):
        call(guide_name="y", guide_op="declip")
    with pytest.raises(ValueError, match="guide_scale"):
        call(guide_name="y", guide_op="declip", guide_scale=0)
    with pytest.raises(ValueError, match="guide_factor"):
        call(guide_name="y", guide_op="declip", guide_scale=0.5, guide_factor=2)
    with pytest.raises(ValueError, match="guide_clip"):
        call(guide_name="y", guide_op="lowpass", guide_scale=0.5, guide_clip=0.3)
    with pytest.raises(ValueError, match="ddpm and ddim"):
        call(guide_name="y", guide_op="lowpass", guide_scale=0.5, sampler="dpmpp2m", steps=4)
    with pytest.raises(ValueError, match="editing"):
        call(guide_name="y", guide_op="lowpass", guide_scale=0.5, known_name="k", keep=[[0, 10]])

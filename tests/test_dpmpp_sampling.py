"""CPU: the host side of the DPM-Solver++(2M) sampler (`sampling_dpmpp`, `DWS_SAMPLER_DPMPP2M`): `dpmpp_coefficients`
against an independent float64 evaluation, its first-order case against DDIM at eta = 0, the solver's order on an
analytic model (Gaussian data, where the optimal epsilon and the probability-flow ODE solution are closed form), the
log-SNR step selection, the argument errors that are raised before any GPU work, and the new `generate.*` keys.  These
pin the arithmetic and the order, not the audio (no trained weights exist offline)."""
import math

import numpy as np
import pytest
import torch

from tests.test_edit_sampling import _StubNet


def _abar(T, beta_T):
    """(float32 Alpha_bar tensor, the same levels as exact Python doubles)"""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    ab = calc_diffusion_hyperparams(T, 1e-4, beta_T)["Alpha_bar"]
    return ab, [float(v) for v in ab.numpy()]


@pytest.mark.parametrize("T,beta_T", [(50, 0.05), (200, 0.02)])
def test_dpmpp_coefficients_match_a_float64_evaluation(T, beta_T):
    from diffwave_sashimi_amd.sampling import dpmpp_coefficients, logsnr_steps
    ab, lv = _abar(T, beta_T)
    lam = lambda v: math.log(math.sqrt(v) / math.sqrt(1.0 - v))
    for tau in (logsnr_steps(ab, 6), logsnr_steps(ab, 11), list(range(T)), [T - 1]):
        S = len(tau)
        m = dpmpp_coefficients(ab, tau)
        assert m.dtype == np.float32 and m.shape == (5, S)
        h = [math.inf] + [lam(lv[tau[s - 1]]) - lam(lv[tau[s]]) for s in range(1, S)]
        for s in range(S):
            a = lv[tau[s]]
            p = 1.0 if s == 0 else lv[tau[s - 1]]
            want = [math.sqrt(1.0 - a), math.sqrt(a), math.sqrt((1.0 - p) / (1.0 - a)),
                    math.sqrt(p) * -math.expm1(-h[s]), h[s] / (2.0 * h[s + 1]) if 1 <= s <= S - 2 else 0.0]
            for r in range(5):
                w32 = np.float32(want[r])
                # one float32 rounding of the float64 value (the two evaluations may differ in the last float64 bits)
                assert abs(float(m[r, s]) - want[r]) <= float(np.spacing(w32)) * 0.5 * (1 + 1e-6), (r, s, m[r, s], want[r])
        assert m[4, 0] == 0.0 and m[4, S - 1] == 0.0 and m[2, 0] == 0.0 and m[3, 0] == 1.0
        assert np.all(m[1] > 0) and np.all(m[4] >= 0) and np.all(np.isfinite(m))


def test_dpmpp_m5_spot_row():
    from diffwave_sashimi_amd.sampling import dpmpp_coefficients
    ab, _ = _abar(200, 0.02)
    m = dpmpp_coefficients(ab, [0, 40, 80, 119, 159, 199])
    assert np.allclose(m[4], [0, 2.29979, 0.74036, 0.55212, 0.49867, 0], rtol=0, atol=1e-4), m[4]


@pytest.mark.parametrize("T,beta_T", [(50, 0.05), (200, 0.02)])
def test_first_order_is_ddim(T, beta_T):
    """m3 x + m4 ((x - m1 eps) / m2) is DDIM's k3 u + k4 eps at eta = 0, at every step (float64 over the float32
    tables; the difference is measured against the largest value of the step)."""
    from diffwave_sashimi_amd.sampling import ddim_coefficients, dpmpp_coefficients, logsnr_steps
    ab, _ = _abar(T, beta_T)
    rng = np.random.default_rng(5)
    x, eps = rng.standard_normal(512), rng.standard_normal(512)
    for tau in (logsnr_steps(ab, 11), list(range(T))):
        m = dpmpp_coefficients(ab, tau).astype(np.float64)
        k = ddim_coefficients(ab, tau, 0.0).astype(np.float64)
        assert np.all(k[4] == 0)
        for s in range(len(tau)):
            ours = m[2, s] * x + m[3, s] * ((x - m[0, s] * eps) / m[1, s])
            ddim = k[2, s] * ((x - k[0, s] * eps) / k[1, s]) + k[3, s] * eps
            assert np.abs(ours - ddim).max() <= 1e-6 * np.abs(ddim).max(), (s, np.abs(ours - ddim).max())


def _gaussian_eps(x, a, c):
    """the optimal epsilon for data N(0, c^2) at level a"""
    return math.sqrt(1.0 - a) * x / (a * c * c + 1.0 - a)


def _dpmpp_loop(m, levels, c, x_T):
    x, hist = x_T.copy(), None
    for s in range(m.shape[1] - 1, -1, -1):
        x0 = (x - m[0, s] * _gaussian_eps(x, levels[s], c)) / m[1, s]
        D = x0
        if hist is not None and m[4, s] != 0:
            D = x0 + m[4, s] * (x0 - hist)
        x = m[2, s] * x + m[3, s] * D
        hist = x0
    return x


def _ddim_loop(k, levels, c, x_T):
    x = x_T.copy()
    for s in range(k.shape[1] - 1, -1, -1):
        eps = _gaussian_eps(x, levels[s], c)
        x = k[2, s] * ((x - k[0, s] * eps) / k[1, s]) + k[3, s] * eps
    return x


@pytest.mark.parametrize("S", [6, 11, 21])
@pytest.mark.parametrize("c", [0.1, 0.3, 1.0])
def test_second_order_on_the_analytic_model(c, S):
    """Gaussian data N(0, c^2), T = 200, beta in [1e-4, 0.02], log-SNR steps: the endpoint of the probability-flow ODE is
    x_T c / sqrt(abar_{T-1} c^2 + 1 - abar_{T-1}).  2M's largest error is at most a quarter of DDIM's at the same step
    count (a float64 prototype's smallest ratio over these nine cases was 9.0; the factor 4 leaves room for the rounding of
    the tables).  With the m5 row zeroed the loop is the DDIM loop."""
    from diffwave_sashimi_amd.sampling import ddim_coefficients, dpmpp_coefficients, logsnr_steps
    ab, lv = _abar(200, 0.02)
    tau = logsnr_steps(ab, S)
    assert len(tau) == (20 if S == 21 else S)
    levels = [lv[t] for t in tau]
    x_T = np.random.default_rng(1234).standard_normal(4096)
    exact = x_T * c / math.sqrt(lv[-1] * c * c + 1.0 - lv[-1])
    m = dpmpp_coefficients(ab, tau).astype(np.float64)
    k = ddim_coefficients(ab, tau, 0.0).astype(np.float64)
    e2 = np.abs(_dpmpp_loop(m, levels, c, x_T) - exact).max()
    e1 = np.abs(_ddim_loop(k, levels, c, x_T) - exact).max()
    print(f"c = {c}, S = {S} ({len(tau)} evaluations): max error DDIM {e1:.3e}, 2M {e2:.3e}, ratio {e1 / e2:.1f}")
    assert e2 <= e1 / 4, (e1, e2)
    m[4] = 0
    first, ddim = _dpmpp_loop(m, levels, c, x_T), _ddim_loop(k, levels, c, x_T)
    assert np.abs(first - ddim).max() <= 1e-6 * np.abs(ddim).max()


def test_logsnr_steps():
    """The S = 11 list of T = 200, beta in [1e-4, 0.02] is the one a float64 cumprod rounded to float32 gave; the
    project's float32 `Alpha_bar` recurrence gives the same list."""
    from diffwave_sashimi_amd.sampling import logsnr_steps
    ab, _ = _abar(200, 0.02)
    assert logsnr_steps(ab, 11) == [0, 1, 3, 6, 11, 21, 37, 63, 102, 150, 199]
    for T, beta_T in ((200, 0.02), (50, 0.05)):
        ab, _ = _abar(T, beta_T)
        for S in (2, 3, 6, 11, 21, T):
            tau = logsnr_steps(ab, S)
            assert all(isinstance(t, int) for t in tau) and len(tau) <= S
            assert tau[0] == 0 and tau[-1] == T - 1 and all(b > a for a, b in zip(tau, tau[1:])), (T, S, tau)
        assert logsnr_steps(ab, 1) == [T - 1]
        assert logsnr_steps(ab.numpy(), 6) == logsnr_steps(ab, 6)
        assert logsnr_steps(ab, [0, 5, T - 1]) == [0, 5, T - 1]                  # an explicit list passes through
        assert logsnr_steps(ab, np.array([3, 4])) == [3, 4]
        for bad in (0, T + 1, -1, 2.5, [], [3, 3], [5, 2], [-1, 4], [0, T], [0.5, 3]):
            with pytest.raises(ValueError):
                logsnr_steps(ab, bad)


def test_argument_errors_are_value_errors_before_any_gpu_work(tmp_path):
    from diffwave_sashimi_amd.generate import generate, load_config
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling_dpmpp
    from tests.test_generate_cli import _tree
    size = B, C, L = (2, 1, 16)
    net = _StubNet()
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    y, x = torch.zeros(size), torch.zeros(size)
    m = torch.zeros(size, dtype=torch.bool)
    bad = [
        dict(noise=torch.zeros(6, B, C, L)),                        # the solver is deterministic: noise without resample
        dict(noise=torch.zeros(6, B, C, L), known=y, mask=m),
        dict(spacing="cosine"),                                     # unknown spacing
        dict(spacing=None),
        dict(known=y, mask=m, resample=(2, 2), noise=torch.zeros(6, B, C, L)),   # not [V, B, C, L] (V = 12)
        dict(resample=(2, 2)),                                      # resample without known / mask
        dict(known=y),                                              # the editing checks of the other samplers
        dict(mask=m),
        dict(known_noise=torch.zeros(6, B, C, L)),
        dict(x_start=x, x_T=x),
        dict(start_step=2),
        dict(x_start=x, start_step=6),
        dict(x_start=x, start_step=2, start_noise=torch.zeros(B, C, L + 1)),
    ]
    for kw in bad:
        for use_graph in (True, False):
            with pytest.raises(ValueError):
                sampling_dpmpp(net, size, dh, 6, use_graph=use_graph, **kw)
    for steps in (0, 51, [4, 4], [0, 50]):
        for spacing in ("logsnr", "uniform"):
            with pytest.raises(ValueError):
                sampling_dpmpp(net, size, dh, steps, spacing=spacing)
    # the CLI keys: refused before a model is built or a GPU is touched
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="sc09", segment_length=640, sampling_rate=16000, data_path=str(tmp_path))
    model = dict(load_config(_tree(tmp_path / "conf"))["model"])     # never constructed
    gen = lambda **kw: generate(0, diff, model, ds, ckpt_iter="init", exp_root=str(tmp_path / "exp"), **kw)
    with pytest.raises(ValueError, match="eta"):
        gen(sampler="dpmpp2m", steps=6, eta=0.5)
    with pytest.raises(ValueError, match="steps"):
        gen(sampler="dpmpp2m")
    with pytest.raises(ValueError, match="spacing"):
        gen(sampler="dpmpp2m", steps=6, spacing="cosine")
    with pytest.raises(ValueError, match="spacing"):
        gen(sampler="ddim", steps=6, spacing="logsnr")              # the key belongs to dpmpp2m
    with pytest.raises(ValueError):
        gen(sampler="dpmpp2m", steps=[5, 3])
    with pytest.raises(ValueError, match="known_name"):
        gen(sampler="dpmpp2m", steps=6, resample_jump=2, resample_n=2)


def test_generate_keys_compose_and_are_checked(tmp_path):
    from diffwave_sashimi_amd.generate import load_config
    from tests.test_generate_cli import _tree
    d = _tree(tmp_path)
    cfg = load_config(d)
    assert "spacing" not in cfg["generate"]                            # absent = today's behaviour
    cfg = load_config(d, ["generate.sampler=dpmpp2m", "generate.steps=6"])
    g = cfg["generate"]
    assert g["sampler"] == "dpmpp2m" and g["steps"] == 6 and "spacing" not in g and g["n_samples"] == 16
    cfg = load_config(d, ["generate.sampler=dpmpp2m", "generate.steps=[0,3,11,49]", "generate.spacing=uniform",
                          "generate.known_name=clip", "generate.keep=[[0,8000]]", "generate.resample_jump=2",
                          "generate.resample_n=2", "generate.start_name=noisy", "generate.start_step=2"])
    g = cfg["generate"]
    assert g["steps"] == [0, 3, 11, 49] and g["spacing"] == "uniform" and g["known_name"] == "clip"
    assert g["keep"] == [[0, 8000]] and (g["resample_jump"], g["resample_n"]) == (2, 2)
    assert g["start_name"] == "noisy" and g["start_step"] == 2

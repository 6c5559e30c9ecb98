"""CPU: the host side of the few-step samplers -- DiffWave's step alignment, DDIM's step sub-sequence and update
coefficients, and the `generate.sampler` keys of the config tree."""
import numpy as np
import pytest

from tests.test_generate_cli import _tree

SIX = [1e-4, 1e-3, 1e-2, 0.05, 0.2, 0.5]     # DiffWave's fast inference schedule for T = 50, beta in [1e-4, 0.05]


def _interp(T, b0, bT, betas):
    """Independent evaluation: sqrt(abar) is decreasing in t, so the aligned step is a linear interpolation of t
    against sqrt(abar), evaluated at sqrt(gamma)."""
    abar = np.cumprod(1.0 - np.linspace(b0, bT, T))
    gamma = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))
    t = np.arange(T, dtype=np.float64)
    return np.interp(np.sqrt(gamma), np.sqrt(abar)[::-1], t[::-1])


@pytest.mark.parametrize("T,bT", [(50, 0.05), (200, 0.02)])
def test_align_steps_matches_an_independent_interpolation(T, bT):
    from diffwave_sashimi_amd.sampling import align_steps
    got = align_steps(T, 1e-4, bT, SIX)
    assert got.dtype == np.float32 and got.shape == (6,)
    ref = _interp(T, 1e-4, bT, SIX)
    # 1e-6 absolute, beyond the one rounding to float32 (half an ulp: 7.6e-6 at t = 138)
    half_ulp = np.spacing(ref.astype(np.float32)).astype(np.float64) / 2
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 1e-6 + half_ulp)
    assert np.all(np.diff(got) > 0) and got[0] == 0.0 and got[-1] < T - 1
    assert np.any(got != np.round(got))       # fractional: these are not the integer indices 0..5


def test_align_steps_identity_gives_the_integer_steps():
    from diffwave_sashimi_amd.sampling import align_steps
    for T, bT in ((6, 0.05), (50, 0.05), (200, 0.02)):
        got = align_steps(T, 1e-4, bT, np.linspace(1e-4, bT, T))
        assert np.array_equal(got, np.arange(T, dtype=np.float32)), T


def test_align_steps_rejects_a_noise_level_beyond_the_training_range():
    from diffwave_sashimi_amd.sampling import align_steps
    with pytest.raises(ValueError, match="gamma_6"):
        align_steps(50, 1e-4, 0.05, SIX + [0.9])      # gamma_6 below abar_49
    # within a relative 1e-9 of the end: clamped
    T, b0, bT = 50, 1e-4, 0.05
    abar = np.cumprod(1.0 - np.linspace(b0, bT, T))
    betas = list(np.linspace(b0, bT, T))
    betas[-1] = 1.0 - abar[-1] * (1 - 1e-12) / abar[-2]
    assert align_steps(T, b0, bT, betas)[-1] == np.float32(T - 1)


def test_ddim_steps():
    from diffwave_sashimi_amd.sampling import ddim_steps
    for T, S in ((200, 20), (200, 50), (50, 6), (200, 200), (7, 3), (200, 2)):
        tau = ddim_steps(T, S)
        assert len(tau) == S and tau[0] == 0 and tau[-1] == T - 1
        assert all(b > a for a, b in zip(tau, tau[1:]))
    assert ddim_steps(200, 1) == [199]
    assert ddim_steps(200, [0, 10, 99]) == [0, 10, 99]
    for bad in ((200, 0), (200, 201), (10, [3, 3]), (10, [5, 2]), (10, [0, 10]), (10, [])):
        with pytest.raises(ValueError):
            ddim_steps(*bad)


def test_ddim_coefficients():
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, ddim_coefficients, ddim_steps
    dh = calc_diffusion_hyperparams(200, 1e-4, 0.02)
    tau = ddim_steps(200, 20)
    k = ddim_coefficients(dh["Alpha_bar"], tau, 0.0)
    assert k.dtype == np.float32 and k.shape == (5, 20)
    assert np.all(k[4] == 0)                                  # eta = 0: deterministic
    assert k[2, 0] == 1 and k[3, 0] == 0                      # s = 0: p_0 = 1
    ab = dh["Alpha_bar"].numpy().astype(np.float64)
    assert k[1, 5] == np.float32(np.sqrt(ab[tau[5]])) and k[2, 5] == np.float32(np.sqrt(ab[tau[4]]))
    k5 = ddim_coefficients(dh["Alpha_bar"], tau, 0.5)
    assert np.all(k5[4, 1:] > 0) and k5[4, 0] == 0 and np.array_equal(k5[:3], k[:3])
    # eta = 1 over every training step is DDPM: sigma_s^2 = beta_tilde_s = (1 - abar_{s-1}) / (1 - abar_s) beta_s
    T = 50
    dh = calc_diffusion_hyperparams(T, 1e-4, 0.05)
    k = ddim_coefficients(dh["Alpha_bar"], list(range(T)), 1.0).astype(np.float64)
    ab = dh["Alpha_bar"].numpy().astype(np.float64)
    beta_tilde = (1 - ab[:-1]) / (1 - ab[1:]) * (1 - ab[1:] / ab[:-1])       # p_s = abar_{s-1}
    assert np.abs(k[4, 1:] ** 2 / beta_tilde - 1).max() < 1e-6
    assert k[4, 0] == 0
    # against the fp32 Sigma of calc_diffusion_hyperparams: that table's beta_s is the fp32 linspace value while
    # 1 - abar_s / abar_{s-1} carries the rounding of the fp32 abar (an ulp of abar over beta: 2e-5 at s = 1)
    sig2 = dh["Sigma"].numpy().astype(np.float64) ** 2
    assert np.abs(k[4, 1:] ** 2 / sig2[1:] - 1).max() < 5e-5


def test_generate_sampler_keys_compose(tmp_path):
    from diffwave_sashimi_amd.generate import load_config
    d = _tree(tmp_path)
    cfg = load_config(d)
    assert "sampler" not in cfg["generate"]                   # default: the reference's loop
    cfg = load_config(d, ["experiment=lj", "generate.sampler=aligned", "diffusion.beta=[0.0001,0.001,0.01,0.05,0.2,0.5]"])
    assert cfg["generate"]["sampler"] == "aligned" and cfg["diffusion"]["beta"] == SIX
    assert cfg["diffusion"]["T"] == 50 and cfg["generate"]["mel_name"] == "LJ001-0001"
    cfg = load_config(d, ["generate.sampler=ddim", "generate.steps=8", "generate.eta=0.5"])
    assert cfg["generate"]["sampler"] == "ddim" and cfg["generate"]["steps"] == 8 and cfg["generate"]["eta"] == 0.5
    assert cfg["diffusion"]["T"] == 200 and cfg["generate"]["n_samples"] == 16


def test_generate_rejects_aligned_without_a_beta_list(tmp_path):
    from diffwave_sashimi_amd.generate import generate
    from tests import cases
    cfg = cases.WAVENET_CASES["wn_tiny"][0]
    with pytest.raises(ValueError, match="diffusion.beta"):
        generate(0, dict(T=5, beta_0=1e-4, beta_T=0.05, beta=None), dict(cfg), dict(segment_length=64),
                 ckpt_iter="init", sampler="aligned", exp_root=str(tmp_path))
    with pytest.raises(ValueError, match="generate.steps"):
        generate(0, dict(T=5, beta_0=1e-4, beta_T=0.05, beta=None), dict(cfg), dict(segment_length=64),
                 ckpt_iter="init", sampler="ddim", exp_root=str(tmp_path))

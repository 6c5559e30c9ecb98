"""CPU: the adaptive prior (PriorGrad) -- sigma from a mel against the float64 definitions, the argument checks of the
samplers and the CLIs (all before an engine is touched), the weighted training loss and the eager guided loop."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import prior_reference as ref

HOP = 6


def _mel(B=3, frames=5, seed=5):
    """U(-11.5, 2) log-mels whose frame 0 is silent (every band at the clip floor log 1e-5: energy 0.028, below
    std_min e_max) and whose frame 1 is loud (every band at 2: energy 24, above e_max)."""
    mel = cases.mel_inputs(B, frames, seed).clone()
    mel[:, :, 0] = float(np.log(1e-5))
    if frames > 1:
        mel[:, :, 1] = 2.0
    return mel


# ------------------------------------------------------------------------------------------------- sigma from a mel
@pytest.mark.parametrize("e_min,cut", [(0.0, 0), (0.5, 3)])
def test_prior_std_of_a_cpu_mel_is_the_float64_definition(e_min, cut):
    """Bound 1e-5 relative: the fp32 evaluation rounds exp (<= 1 ulp), adds 80 positive terms (<= 80 x 6e-8 = 4.8e-6 in
    the worst case, halved by the square root), and subtracts / divides once each; with e_min = 0.5 the subtraction
    amplifies the error of an unclamped energy (>= 1.2 here) by less than 2."""
    from diffwave_sashimi_amd.mel import mel_energy, prior_std_from_mel
    mel = _mel()
    frames = mel.shape[-1]
    L = frames * HOP - cut
    kw = dict(energy_max=8.0, energy_min=e_min, std_min=0.1)
    got = prior_std_from_mel(mel, HOP, None if cut == 0 else L, **kw)
    want = ref.prior_std(mel, HOP, L, **kw)
    assert got.shape == (3, 1, L) and got.dtype == torch.float32 and got.device.type == "cpu"
    err = float(np.abs(got.double().numpy() / want - 1).max())
    print(f"cpu sigma against float64 (e_min {e_min}, L {L}): worst relative error {err:.3e}")
    assert err <= 1e-5
    assert torch.all(got[:, :, :HOP] == np.float32(0.1)) and torch.all(got[:, :, HOP:2 * HOP] == 1.0)    # both clamps
    inner = got[:, :, 2 * HOP:]
    assert float(inner.min()) > 0.1 and float(inner.max()) < 1.0                # and frames between them
    e = mel_energy(mel)
    assert e.shape == (3, frames) and float(np.abs(e.double().numpy() / ref.energy(mel) - 1).max()) <= 1e-5
    # a clip's row does not depend on the batch around it
    assert torch.equal(prior_std_from_mel(mel[1:2], HOP, L, **kw), got[1:2])


def test_prior_std_argument_checks():
    from diffwave_sashimi_amd.mel import mel_energy, prior_std_from_mel
    mel = _mel()
    with pytest.raises(TypeError):                      # energy_max is required: it depends on the dataset
        prior_std_from_mel(mel, HOP)
    for bad in (dict(energy_max=0.0), dict(energy_max=1.0, energy_min=1.0), dict(energy_max=float("nan")),
                dict(energy_max=float("inf")), dict(energy_max=2.0, std_min=0.0), dict(energy_max=2.0, std_min=1.5),
                dict(energy_max="big")):
        with pytest.raises(ValueError, match="prior"):
            prior_std_from_mel(mel, HOP, **bad)
    with pytest.raises(ValueError, match="L ="):
        prior_std_from_mel(mel, HOP, mel.shape[-1] * HOP + 1, energy_max=8.0)
    with pytest.raises(ValueError, match="L ="):
        prior_std_from_mel(mel, HOP, 0, energy_max=8.0)
    with pytest.raises(ValueError, match="hop"):
        prior_std_from_mel(mel, 0, energy_max=8.0)
    with pytest.raises(ValueError, match="bands, frames"):
        prior_std_from_mel(mel[0], HOP, energy_max=8.0)
    with pytest.raises(ValueError, match="bands, frames"):
        mel_energy(mel[0])


# ------------------------------------------------------------------------------------------ the samplers' checks
class _NoEngine:
    """Stands where a network stands; any use of it fails the test."""
    n_classes = 2

    def _label_list(self, labels, B):       # (the host-side label check of an engine model)
        return tuple(int(v) for v in labels)

    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("entry", ["sampling", "sampling_ddim", "sampling_dpmpp", "sampling_aligned", "sampling_guided"])
def test_sampler_argument_checks_come_before_the_engine(entry):
    from diffwave_sashimi_amd import sampling as smp
    B, C, L = 2, 1, 12
    dh = smp.calc_diffusion_hyperparams(50, 1e-4, 0.05)
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=[1e-4, 1e-2, 0.2])

    def run(prior_std, **kw):
        net = _NoEngine()
        if entry == "sampling":
            return smp.sampling(net, (B, C, L), dh, prior_std=prior_std, **kw)
        if entry == "sampling_ddim":
            return smp.sampling_ddim(net, (B, C, L), dh, 4, prior_std=prior_std, **kw)
        if entry == "sampling_dpmpp":
            return smp.sampling_dpmpp(net, (B, C, L), dh, 4, prior_std=prior_std, **kw)
        if entry == "sampling_aligned":
            return smp.sampling_aligned(net, (B, C, L), diff, prior_std=prior_std, **kw)
        return smp.sampling_guided(net, (B, C, L), dh, measurement=torch.zeros(B, C, L), operator=lambda x: x, scale=0.5,
                                   prior_std=prior_std, **kw)
    ok = torch.full((B, 1, L), 0.5)
    for bad in (torch.full((B, 1, L + 1), 0.5), torch.full((1, 1, L), 0.5), torch.full((B, 2, L), 0.5), torch.full((L,), 0.5),
                torch.ones(B, 1, L, dtype=torch.int64)):
        with pytest.raises(ValueError, match="prior_std of shape"):
            run(bad)
    for v in (0.0, -0.5, float("nan"), float("inf")):
        bad = ok.clone()
        bad[1, 0, 7] = v
        with pytest.raises(ValueError, match="finite and > 0"):
            run(bad)
    with pytest.raises(ValueError, match="prior_std.*classifier-free|classifier-free.*prior_std"):
        run(ok, labels=[0, 1], cfg_scale=1.5)


# ------------------------------------------------------------------------------------------------ the CLIs' checks
def test_cli_prior_keys():
    from diffwave_sashimi_amd.generate import generate, prior_settings, resolve_prior
    from diffwave_sashimi_amd.train import train
    full = {"kind": "energy", "energy_max": 7.5, "energy_min": 0.0, "std_min": 0.1}
    assert prior_settings(None) is None and prior_settings("none") == "none"
    assert prior_settings("energy", 7.5) == full
    assert prior_settings("energy", 7.5, 0.25, 0.2) == dict(full, energy_min=0.25, std_min=0.2)
    with pytest.raises(ValueError, match="mel-conditional"):
        prior_settings("energy", 7.5, unconditional=True)
    with pytest.raises(ValueError, match="prior_energy_max"):
        prior_settings("energy")
    with pytest.raises(ValueError, match="needs generate.prior=energy"):
        prior_settings(None, 7.5)
    with pytest.raises(ValueError, match="needs generate.prior=energy"):
        prior_settings("none", None, None, 0.1)
    with pytest.raises(ValueError, match="expected energy or none"):
        prior_settings("loud", 7.5)
    for bad in ((0.0, None, None), (1.0, 2.0, None), (7.5, None, 0.0), (7.5, None, 1.5), (True, None, None)):
        with pytest.raises(ValueError):
            prior_settings("energy", *bad)
    # against the checkpoint's entry
    assert resolve_prior(None, None) is None
    assert resolve_prior(None, full) == full                             # no keys: the checkpoint's prior
    assert resolve_prior("none", full) is None                           # prior=none forces N(0, I)
    assert resolve_prior(prior_settings("energy", 7.5), None) == full    # keys alone (no entry, e.g. ckpt_iter=init)
    assert resolve_prior(prior_settings("energy", 7.5), full, ["energy_max"]) == full
    trained = dict(full, std_min=0.2)
    assert resolve_prior(prior_settings("energy", 7.5), trained, ["energy_max"]) == trained     # unspoken keys follow it
    with pytest.raises(ValueError, match="contradicts the checkpoint"):
        resolve_prior(prior_settings("energy", 8.0), full, ["energy_max"])
    with pytest.raises(ValueError, match="contradicts the checkpoint"):
        resolve_prior(prior_settings("energy", 7.5, std_min=0.1), trained, ["energy_max", "std_min"])
    with pytest.raises(ValueError, match="not one this version writes"):
        resolve_prior(None, {"kind": "other"})

    # the hop of sigma is the conditioner's: prod(model.mel_upsample), which dataset.hop_length must equal
    from diffwave_sashimi_amd.generate import prior_hop, same_prior, smooth_ckpt
    assert prior_hop({"mel_upsample": [16, 16]}, {"hop_length": 256}) == 256
    assert prior_hop({"mel_upsample": [3, 5]}, {"hop_length": 15}) == 15
    with pytest.raises(ValueError, match="mel_upsample"):
        prior_hop({"mel_upsample": [16, 16]}, {"hop_length": 300})
    assert same_prior(None, None) and same_prior(full, dict(full)) and same_prior(full, dict(full, energy_max=7.5))
    assert not same_prior(full, None) and not same_prior(None, full) and not same_prior(full, trained)

    # the entry points themselves, before a model is built (no GPU here: building one would fail otherwise)
    uncond = dict(cases.WAVENET_CASES["wn_tiny"][0])
    cond = dict(cases.WAVENET_COND_CASES["wn_cond_tiny"][0])
    diff = dict(T=4, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="ljspeech", data_path="/nonexistent", segment_length=512, sampling_rate=22050, hop_length=256)
    with pytest.raises(ValueError, match="mel-conditional"):
        generate(0, diff, uncond, ds, ckpt_iter="init", prior="energy", prior_energy_max=7.5)
    with pytest.raises(ValueError, match="cfg_scale does not combine"):
        generate(0, diff, dict(cond, n_classes=2), ds, ckpt_iter="init", mel_name="a", prior="energy", prior_energy_max=7.5,
                 label=0, cfg_scale=1.0)
    with pytest.raises(ValueError, match="mel_name"):
        generate(0, diff, cond, ds, ckpt_iter="init", prior="energy", prior_energy_max=7.5)
    with pytest.raises(ValueError, match="needs generate.prior=energy"):
        generate(0, diff, cond, ds, ckpt_iter="init", mel_name="a", prior="none", prior_energy_max=7.5)
    tr = dict(ckpt_iter=-1, n_iters=1, iters_per_ckpt=1, iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=1)
    with pytest.raises(ValueError, match="train.prior=energy needs a mel-conditional"):
        train(0, 1, diff, uncond, ds, {}, prior="energy", prior_energy_max=7.5, **tr)
    with pytest.raises(ValueError, match="train.prior_energy_max"):
        train(0, 1, diff, cond, ds, {}, prior="energy", **tr)
    with pytest.raises(ValueError, match="mel_upsample"):
        train(0, 1, diff, cond, dict(ds, hop_length=128), {}, prior="energy", prior_energy_max=7.5, **tr)
    with pytest.raises(ValueError, match="mel_upsample"):
        generate(0, diff, cond, dict(ds, hop_length=128), ckpt_iter="init", mel_name="a", prior="energy", prior_energy_max=7.5)


def test_checkpoint_smoothing_reports_the_priors(tmp_path):
    """``smooth_ckpt`` hands back the ``prior`` entry of every checkpoint it averages (``generate`` refuses a mean of
    checkpoints trained with different priors and samples from the common one otherwise)."""
    from diffwave_sashimi_amd.generate import same_prior, smooth_ckpt
    entry = {"kind": "energy", "energy_max": 7.5, "energy_min": 0.0, "std_min": 0.1}
    for it, e in ((1, None), (2, entry), (3, dict(entry))):
        saved = {"model_state_dict": {"w": torch.full((2,), float(it))}}
        if e is not None:
            saved["prior"] = e
        torch.save(saved, str(tmp_path / f"{it}.pkl"))
    got = []
    sd = smooth_ckpt(str(tmp_path), 1, 3, priors=got)
    assert torch.equal(sd["w"], torch.full((2,), 2.5)) and got == [(2, entry), (3, entry)]
    assert all(same_prior(e, got[0][1]) for _, e in got)
    got = []
    smooth_ckpt(str(tmp_path), 0, 3, priors=got)
    assert [it for it, e in got if not same_prior(e, got[0][1])] == [2, 3]
    assert torch.equal(smooth_ckpt(str(tmp_path), 0, 3)["w"], torch.full((2,), 2.0))          # without the list: as before


# ------------------------------------------------------------------------------------------------------- training
class _StandIn(torch.nn.Module):
    """A differentiable network of the reference surface: eps = conv(x) + t / 100."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.conv = torch.nn.Conv1d(1, 1, 5, padding=2)
        self.seen = None

    def forward(self, inp, mel_spec=None, labels=None):
        x, t = inp
        self.seen = (x.detach().clone(), t.detach().clone())
        return self.conv(x) + t.reshape(-1, 1, 1) / 100.0


def test_training_loss_with_a_prior():
    """rtol 1e-5: the hand-written fp32 expression differs by at most three roundings per element and the order of an
    fp32 mean over 2 x 500 positive terms; against float64 the same three roundings (1.8e-7 relative each)."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import q_sample, training_loss
    B, L = 2, 500
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    g0 = torch.Generator().manual_seed(17)
    audio = torch.rand(B, 1, L, generator=g0) * 0.6 - 0.3
    sigma = torch.rand(B, 1, L, generator=g0) * 0.9 + 0.1
    net, mse = _StandIn(), torch.nn.MSELoss()

    gen = torch.Generator().manual_seed(23)
    loss = training_loss(net, mse, audio, dh, generator=gen, prior_std=sigma)
    state = gen.get_state()
    x_t, t = net.seen
    # the same draws, by hand
    gen2 = torch.Generator().manual_seed(23)
    steps = torch.randint(50, size=(B, 1, 1), generator=gen2)
    z = torch.normal(0, 1, size=audio.shape, generator=gen2)
    assert torch.equal(t, steps.view(B, 1))
    ab = dh["Alpha_bar"][steps]
    want_x = ref.q_sample(audio, ab, z, sigma)
    # x_t = sqrt(ab) x0 + sqrt(1-ab) (sigma z): five fp32 roundings on values below 5
    assert float(np.abs(x_t.double().numpy() - want_x).max()) <= 4e-6
    assert torch.equal(q_sample(audio, steps, dh["Alpha_bar"], z, prior_std=sigma), x_t)
    with torch.no_grad():
        eps_theta = net((x_t, t))
        by_hand = (((eps_theta - sigma * z) / sigma) ** 2).mean()
    f64 = ref.loss(eps_theta, z, sigma)
    print(f"weighted loss {float(loss.detach()):.6f}, by hand {float(by_hand):.6f}, float64 {f64:.6f}")
    assert abs(float(loss.detach()) - float(by_hand)) <= 1e-5 * abs(float(by_hand))
    assert abs(float(loss.detach()) - f64) <= 1e-5 * abs(f64)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for p in net.parameters())

    # prior_std = ones is the unweighted call, and a prior consumes the generator as the call without one does
    gen3, gen4 = torch.Generator().manual_seed(23), torch.Generator().manual_seed(23)
    plain = training_loss(net, mse, audio, dh, generator=gen3).detach()
    ones = training_loss(net, mse, audio, dh, generator=gen4, prior_std=torch.ones(B, 1, L)).detach()
    assert abs(float(ones) - float(plain)) <= 1e-5 * abs(float(plain))
    assert torch.equal(gen3.get_state(), state) and torch.equal(gen4.get_state(), state)
    assert abs(float(plain) - float(loss.detach())) > 1e-3 * abs(float(plain))                   # and the weighting is not a no-op
    with pytest.raises(ValueError, match="prior_std"):
        training_loss(net, mse, audio, dh, prior_std=torch.ones(B, 1, L + 1))
    for v in (0.0, -1.0, float("nan"), float("inf")):          # the values of a CPU table are checked
        bad = sigma.clone()
        bad[1, 0, 3] = v
        with pytest.raises(ValueError, match="finite and > 0"):
            training_loss(net, mse, audio, dh, prior_std=bad)


# ---------------------------------------------------------------------------------------------- the eager guided loop
@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_guided_loop_with_a_prior_is_the_loop_with_prescaled_noise(sampler):
    from diffwave_sashimi_amd import sampling as smp
    B, L, S = 2, 64, 4
    g = torch.Generator().manual_seed(31)
    x_T = torch.randn(B, 1, L, generator=g)
    z = torch.randn(S, B, 1, L, generator=g)
    sigma = torch.rand(B, 1, L, generator=g) * 0.9 + 0.1
    y = smp.declip_operator(0.2)(torch.randn(B, 1, L, generator=g) * 0.3)
    net = _StandIn()
    if sampler == "ddpm":
        dh, kw = smp.calc_diffusion_hyperparams(S, 1e-4, 0.05), {}
    else:
        dh, kw = smp.calc_diffusion_hyperparams(50, 1e-4, 0.05), dict(steps=S, eta=0.5)
    run = lambda **more: smp.sampling_guided(net, (B, 1, L), dh, measurement=y, operator=smp.declip_operator(0.2), scale=0.5,
                                             sampler=sampler, x_T=x_T, **kw, **more)
    with_prior = run(noise=z, prior_std=sigma)
    assert torch.equal(with_prior, run(noise=sigma * z))
    assert not torch.equal(with_prior, run(noise=z))
    assert torch.equal(run(noise=z, prior_std=torch.ones(B, 1, L)), run(noise=z))
    # drawn noise (a torch generator with this net) is scaled too, the drawn initial state included
    drawn = smp.sampling_guided(net, (B, 1, L), dh, measurement=y, operator=smp.declip_operator(0.2), scale=0.5,
                                sampler=sampler, seed=7, prior_std=sigma, **kw)
    gen = torch.Generator().manual_seed(7)
    x0 = torch.randn((B, 1, L), generator=gen)
    zs = {s: torch.randn((B, 1, L), generator=gen) for s in range(S - 1, 0, -1)}
    noise = torch.stack([torch.zeros(B, 1, L)] + [zs[s] for s in range(1, S)])
    assert torch.equal(drawn, smp.sampling_guided(net, (B, 1, L), dh, measurement=y, operator=smp.declip_operator(0.2),
                                                  scale=0.5, sampler=sampler, x_T=sigma * x0, noise=sigma * noise, **kw))

"""GPU: the spectral prior (``prior_filter=`` / ``prior_stft=``) on the training loss and on the samplers, on the small
mel-conditional WaveNet and SaShiMi of the prior tests at L = 2 .. 4 hops of 256, with an STFT of 512 / 256 / 512.

Training: the loss and every parameter gradient against a float64 restatement (tests/tvfilter_reference.py) around the
engine's own eps_theta.  The loss is a mean of squares of one ``dws_tv_filter`` result: 1e-5 relative, the tolerance of
tests/test_prior_gpu.py.  The gradient, in two places, both with the recipe of tests/test_tvfilter_gpu.py (a float32 torch
restatement of the same two filter stages -- autograd through ``tv_torch`` -- is measured against float64 on the same
inputs, and the kernels are held to 8 times that):
  * the cotangent d loss / d eps_theta that reaches the engine's backward (a tensor hook on the network's output) against
    ``2 / (B L) T^T T (eps_theta - eps)`` in float64, max |error| / max |cotangent|;
  * every parameter gradient against the engine's backward from that float64 cotangent (rounded to float32 once) through
    the same forward.  The yardstick is the same backward from the float32 torch cotangent.  A parameter's gradient is a
    sum over all positions with cancellation, so errors are taken in the l2 norm, not against the largest entry: the
    whole gradient at 8 times the yardstick's, and each parameter at 8 times its own yardstick.  A parameter's own
    yardstick is one draw of rounding noise -- exactly 0 now and then for a bias of one entry -- so it is floored by
    the whole gradient's relative yardstick applied to the parameter's norm; and 2^-23 of the whole gradient's norm is
    added, the float32 rounding of the engine's own sums, which is all that is left of a gradient that is analytically
    0 (a weight-normalised direction with one entry per channel).

Sampling: bit for bit.  A run with ``prior_filter=F`` that draws its own noise equals the run without it that is handed
``x_T = T_F(z_S)`` and ``noise[s] = T_F(z_s)``, ``z_s`` Philox stream s of the seed (or of every clip's own seed)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cases
from tests import tvfilter_reference as tvr
from tests.test_tvfilter_gpu import tv_torch

pytestmark = pytest.mark.gpu

SEED = 4321
S = 6
HOP = 256
DCFG = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=[1e-4, 1e-3, 1e-2, 0.05, 0.2, 0.5])


def _stft():
    from diffwave_sashimi_amd.mel import TacotronSTFT
    return TacotronSTFT(filter_length=512, hop_length=HOP, win_length=512, n_mel_channels=80, sampling_rate=22050)


def _filter(stft, mel, L):
    F = stft.spectral_filter(mel, L, ref=stft.spectral_prior_ref(mel), floor=0.05, lifter=12)
    assert F.dtype == torch.complex64 and tuple(F.shape) == (mel.shape[0], 257, L // HOP + 1) and F.device == mel.device
    assert bool(torch.isfinite(torch.view_as_real(F)).all()) and float(F.abs().std()) > 0
    return F


# ---------------------------------------------------------------------------------------------------------- training
def _training_case(name, gpu):
    if name.startswith("wn"):
        cfg, B, L, Tmel, wseed, iseed, _ = cases.WAVENET_COND_CASES["wn_cond_c64"]
    else:
        cfg, B, Tmel, wseed, iseed, _ = cases.SASHIMI_COND_CASES["ss_cond_d32"]
        L = cfg["L"]
    net = cases.build_ours(cfg, wseed).to(gpu).train()
    if name.endswith("bf16x6"):
        net.set_option("precision", "bf16x6")
    audio = (torch.rand(B, 1, L, generator=torch.Generator().manual_seed(iseed)) * 0.6 - 0.3).to(gpu)
    return net, audio, cases.mel_inputs(B, Tmel, iseed).to(gpu)


@pytest.mark.parametrize("name", ["wn_cond_c64", "wn_cond_c64_bf16x6", "ss_cond_d32"])
def test_training_loss_with_a_spectral_prior(gpu, name):
    from diffwave_sashimi_amd import mel as melmod
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import q_sample, training_loss
    net, audio, mel = _training_case(name, gpu)
    B, _, L = audio.shape
    stft = _stft()
    F = _filter(stft, mel, L)
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    seen = []
    caught = []

    def keep(mod, args, out):
        seen.append(out.detach().clone())
        out.register_hook(lambda g: caught.append(g.detach().clone()))
    hook = net.register_forward_hook(keep)
    loss = training_loss(net, None, audio, dh, mel_spec=mel, generator=torch.Generator().manual_seed(29), prior_filter=F,
                         prior_stft=stft)
    hook.remove()
    loss.backward()
    # the float64 restatement around the engine's own eps_theta
    gen = torch.Generator().manual_seed(29)
    steps = torch.randint(50, size=(B, 1, 1), generator=gen)
    z = torch.normal(0, 1, size=audio.shape, generator=gen)
    w = stft.window.numpy()
    inv = (1.0 / F).cpu().numpy()
    eps = melmod.tv_filter(z.to(gpu).view(B, L), F, window=stft.window.to(gpu), hop_length=HOP)        # what was added
    d = (seen[0].view(B, L) - eps).cpu()                                    # float32, as the loss forms it
    r = tvr.tv_forward64(d.numpy(), inv, w, HOP)
    want = float((r ** 2).mean())
    print(f"{name}: loss with a spectral prior {float(loss.detach()):.6f}, float64 from the engine's eps {want:.6f}")
    assert abs(float(loss.detach()) - want) <= 1e-5 * abs(want)
    # the cotangent the engine's backward received, against float64; the yardstick is float32 torch on the same inputs
    cot = 2.0 / (B * L) * tvr.tv_adjoint64(r, inv, w, HOP)
    d32 = d.clone().requires_grad_()
    (tv_torch(d32, torch.from_numpy(inv), torch.from_numpy(w), HOP) ** 2).mean().backward()
    err32 = float(np.abs(d32.grad.numpy() - cot).max() / np.abs(cot).max())
    assert len(caught) == 1 and tuple(caught[0].shape) == (B, 1, L)
    err = float(np.abs(caught[0].view(B, L).cpu().numpy() - cot).max() / np.abs(cot).max())
    print(f"{name}: cotangent of eps_theta: kernels {err:.3e}, float32 torch {err32:.3e}")
    assert err <= 8 * err32
    # every parameter gradient: the engine's backward from the float64 cotangent, and from float32 torch's as the yardstick
    got = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    assert all(torch.isfinite(g).all() for g in got.values()) and any(float(g.abs().max()) > 0 for g in got.values())
    x_t = q_sample(audio, steps.to(gpu), dh["Alpha_bar"], eps.view(B, 1, L))

    def backward_from(c):
        net.zero_grad()
        out = net((x_t, steps.view(B, 1).to(gpu)), mel_spec=mel)
        assert torch.equal(out.detach(), seen[0])
        out.backward(c.to(torch.float32).view(B, 1, L).to(gpu))
        return {k: p.grad.detach().double() for k, p in net.named_parameters()}
    want_g = backward_from(torch.from_numpy(cot))
    yard_g = backward_from(d32.grad)
    norm = lambda g: float(torch.sqrt(sum((v.double() ** 2).sum() for v in g.values())))
    whole = norm(want_g)
    err_all = norm({k: got[k].double() - want_g[k] for k in got})
    yard_all = norm({k: yard_g[k] - want_g[k] for k in got})
    print(f"{name}: parameter gradients: kernels {err_all / whole:.3e}, float32 torch {yard_all / whole:.3e} of the "
          "gradient's norm")
    assert err_all <= 8 * yard_all
    for k in got:
        e, y = float((got[k].double() - want_g[k]).norm()), float((yard_g[k] - want_g[k]).norm())
        floor = yard_all / whole * float(want_g[k].norm())
        assert e <= 8 * max(y, floor) + 2.0 ** -23 * whole, (k, e, y, floor, whole)


def test_training_loss_combinations(gpu):
    """``stft_weight`` on top of the prior, the plain call untouched by the new arguments, and the refusals that need a
    device."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    net, audio, mel = _training_case("wn_cond_c64", gpu)
    stft = _stft()
    F = _filter(stft, mel, audio.shape[-1])
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    run = lambda **kw: training_loss(net, torch.nn.MSELoss(), audio, dh, mel_spec=mel,
                                     generator=torch.Generator().manual_seed(31), **kw)
    plain = run()
    assert torch.equal(run(prior_filter=None, prior_stft=None), plain)
    base = run(prior_filter=F, prior_stft=stft)
    assert torch.equal(run(prior_filter=F, prior_stft=stft), base) and not torch.equal(base, plain)
    parts = {}
    both = run(prior_filter=F, prior_stft=stft, stft_weight=0.5, stft_resolutions=[[256, 64, 256]], parts=parts)
    assert torch.equal(parts["eps"], base.detach()) and float(parts["stft"]) > 0
    assert abs(float(both.detach()) - (float(base) + 0.5 * float(parts["stft"]))) <= 1e-6 * abs(float(both.detach()))
    both.backward()
    assert all(torch.isfinite(p.grad).all() for p in net.parameters())
    with pytest.raises(ValueError, match="requires grad"):
        run(prior_filter=F.clone().requires_grad_(), prior_stft=stft)
    with pytest.raises(ValueError, match="filt"):
        run(prior_filter=F[:, :, :-1], prior_stft=stft)


def test_labels_with_a_spectral_prior(gpu):
    """A class-conditional mel-conditional WaveNet (``n_classes = 2``): the loss with labels, and a labelled DDIM run at
    eta = 1 against the plain labelled run handed the shaped noise."""
    from diffwave_sashimi_amd import sampling as smp
    from diffwave_sashimi_amd.training import training_loss
    cfg, B, L, Tmel, wseed, iseed, _ = cases.WAVENET_COND_CASES["wn_cond_c64"]
    net = cases.build_ours(dict(cfg, n_classes=2), wseed).to(gpu).train()
    audio = (torch.rand(B, 1, L, generator=torch.Generator().manual_seed(iseed)) * 0.6 - 0.3).to(gpu)
    mel = cases.mel_inputs(B, Tmel, iseed).to(gpu)
    stft = _stft()
    F = _filter(stft, mel, L)
    dh = smp.calc_diffusion_hyperparams(50, 1e-4, 0.05)
    run = lambda labels: training_loss(net, None, audio, dh, mel_spec=mel, generator=torch.Generator().manual_seed(31),
                                       labels=labels, prior_filter=F, prior_stft=stft)
    first, other = run(torch.tensor([0, 1])).detach(), run(torch.tensor([1, 0])).detach()
    a = run(torch.tensor([0, 1]))        # (the engine keeps one forward's activations: the one that is differentiated runs last)
    assert torch.equal(a.detach(), first) and bool(torch.isfinite(a)) and not torch.equal(other, first)
    a.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    net.eval()
    size = (B, 1, L)
    sample = lambda **kw: smp.sampling_ddim(net, size, dh, S, 1.0, mel, labels=[0, 1], **kw)
    got = sample(seed=SEED, prior_filter=F, prior_stft=stft)
    want = sample(x_T=_shaped(size, SEED, S, F, stft, gpu),
                  noise=torch.stack([_shaped(size, SEED, s, F, stft, gpu) for s in range(S)]))
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert not torch.equal(got, smp.sampling_ddim(net, size, dh, S, 1.0, mel, labels=[1, 0], seed=SEED, prior_filter=F,
                                                  prior_stft=stft))


# ---------------------------------------------------------------------------------------------------------- sampling
def _sampling_case(name, gpu):
    if name == "wn_cond_tiny":
        cfg, B, _, _, wseed, iseed, _ = cases.WAVENET_COND_CASES[name]
        L, Tmel = 3 * HOP, 3
    else:
        cfg, B, Tmel, wseed, iseed, _ = cases.SASHIMI_COND_CASES[name]
        L = cfg["L"]
    net = cases.build_ours(cfg, wseed).to(gpu)
    mel = cases.mel_inputs(B, Tmel, iseed).to(gpu)
    stft = _stft()
    return net, mel, (B, 1, L), stft, _filter(stft, mel, L)


def _z(size, seed, stream, gpu):
    """Philox stream `stream` as the samplers draw it: of a scalar seed over the whole batch, of a seed list per clip."""
    from diffwave_sashimi_amd import _lib
    B, C, L = size
    z = torch.empty(size, device=gpu)
    if isinstance(seed, list):
        _lib.check(_lib.load().dws_philox_normal_clips(z.data_ptr(), B, C * L, (ctypes.c_uint64 * B)(*seed), stream,
                                                       _lib.current_stream()))
    else:
        _lib.check(_lib.load().dws_philox_normal(z.data_ptr(), z.numel(), seed, stream, _lib.current_stream()))
    return z


def _shaped(size, seed, stream, F, stft, gpu, lengths=None):
    from diffwave_sashimi_amd.mel import tv_filter
    B, _, L = size
    return tv_filter(_z(size, seed, stream, gpu).view(B, L), F, window=stft.window.to(gpu), hop_length=HOP,
                     lengths=lengths).view(B, 1, L)


def _runs(net, size, mel):
    """kind -> (steps, noisy, run(**kw))"""
    from diffwave_sashimi_amd import sampling as smp
    dh6 = smp.calc_diffusion_hyperparams(S, 1e-4, 0.05)
    dh = smp.calc_diffusion_hyperparams(50, 1e-4, 0.05)
    return {
        "ddpm": (S, True, lambda **kw: smp.sampling(net, size, dh6, mel, **kw)),
        "aligned": (len(DCFG["beta"]), True, lambda **kw: smp.sampling_aligned(net, size, DCFG, mel, **kw)),
        "ddim0": (S, False, lambda **kw: smp.sampling_ddim(net, size, dh, S, 0.0, mel, **kw)),
        "ddim1": (S, True, lambda **kw: smp.sampling_ddim(net, size, dh, S, 1.0, mel, **kw)),
        "dpmpp2m": (len(smp.logsnr_steps(dh["Alpha_bar"], S)), False, lambda **kw: smp.sampling_dpmpp(net, size, dh, S, mel, **kw)),
    }


@pytest.mark.parametrize("seed", [SEED, [11, 2 ** 63 + 5]], ids=["scalar", "per_clip"])
@pytest.mark.parametrize("kind", ["ddpm", "aligned", "ddim0", "ddim1", "dpmpp2m"])
@pytest.mark.parametrize("name", ["wn_cond_tiny", "ss_cond_tiny"])
def test_a_spectral_prior_run_is_the_plain_run_with_shaped_noise(gpu, name, kind, seed):
    net, mel, size, stft, F = _sampling_case(name, gpu)
    n, noisy, run = _runs(net, size, mel)[kind]
    got = run(seed=seed, prior_filter=F, prior_stft=stft)
    explicit = dict(x_T=_shaped(size, seed, n, F, stft, gpu))
    if noisy:       # (row 0 is read by no sampler: whatever it holds)
        explicit["noise"] = torch.stack([_shaped(size, seed, s, F, stft, gpu) for s in range(n)])
    want = run(**explicit)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    plain = run(seed=seed)
    assert not torch.equal(got, plain)
    assert torch.equal(run(seed=seed, prior_filter=None, prior_stft=None), plain)          # without it: the run as it was
    assert torch.equal(run(seed=seed, prior_filter=F, prior_stft=stft, use_graph=False), got)
    if noisy:       # injected noise stays standard normal and is shaped; an injected x_T is a state
        z = torch.stack([_z(size, seed, s, gpu) for s in range(n)])
        assert torch.equal(run(x_T=explicit["x_T"], noise=z, prior_filter=F, prior_stft=stft), got)
    if isinstance(seed, list):      # a clip with its seed and its filter is its B = 1 run
        n1, _, run1 = _runs(net, (1,) + tuple(size[1:]), mel[1:2])[kind]
        assert torch.equal(run1(seed=seed[1], prior_filter=F[1:2], prior_stft=stft), got[1:2])


@pytest.mark.parametrize("kind", ["ddpm", "ddim1", "dpmpp2m"])
def test_ragged_batch_with_a_spectral_prior(gpu, kind):
    """wn_cond_tiny at lengths [768, 512] with per-clip seeds: the shaped noise of clip 1 is that of its own two hops (frames
    behind them, NaN here, are not read), the padding comes back as exact zeros."""
    net, mel, size, stft, F = _sampling_case("wn_cond_tiny", gpu)
    lens, seeds = [3 * HOP, 2 * HOP], [5, 6]
    n, noisy, run = _runs(net, size, mel)[kind]
    dirty = F.clone()
    dirty[1, :, 3:] = float("nan")
    got = run(seed=seeds, lengths=lens, prior_filter=dirty, prior_stft=stft)
    explicit = dict(x_T=_shaped(size, seeds, n, F, stft, gpu, lens))
    if noisy:
        explicit["noise"] = torch.stack([_shaped(size, seeds, s, F, stft, gpu, lens) for s in range(n)])
    assert torch.equal(got, run(lengths=lens, **explicit)) and bool(torch.isfinite(got).all())
    assert torch.count_nonzero(got[1, :, lens[1]:]) == 0 and torch.count_nonzero(got[1, :, :lens[1]]) > 0
    # with a scalar seed too (its numbering runs over the padded batch)
    got = run(seed=SEED, lengths=lens, prior_filter=F, prior_stft=stft)
    explicit = dict(x_T=_shaped(size, SEED, n, F, stft, gpu, lens))
    if noisy:
        explicit["noise"] = torch.stack([_shaped(size, SEED, s, F, stft, gpu, lens) for s in range(n)])
    assert torch.equal(got, run(lengths=lens, **explicit))


def test_refused_combinations(gpu):
    from diffwave_sashimi_amd import sampling as smp
    net, mel, size, stft, F = _sampling_case("wn_cond_tiny", gpu)
    B, _, L = size
    runs = _runs(net, size, mel)
    known = torch.zeros(size)
    mask = smp.spans_to_mask(size, [(0, 100)])
    for kind in ("ddpm", "aligned", "ddim1", "dpmpp2m"):
        run = runs[kind][2]
        ok = dict(seed=1, prior_filter=F, prior_stft=stft)
        for bad in (dict(prior_std=torch.ones(B, 1, L)), dict(cfg_scale=1.0, labels=[0, 1]), dict(known=known, mask=mask),
                    dict(known=known, mask=mask, resample=(2, 2)), dict(x_start=known, start_step=3),
                    dict(x_start=known, start_step=3, start_noise=False), dict(known_noise=torch.zeros((6,) + size))):
            with pytest.raises(ValueError, match="prior_filter"):
                run(**ok, **bad)
        with pytest.raises(ValueError, match="come together"):
            run(seed=1, prior_filter=F)
        with pytest.raises(ValueError, match="come together"):
            run(seed=1, prior_stft=stft)
        with pytest.raises(ValueError, match="cuda tensor"):
            run(seed=1, prior_filter=F.cpu(), prior_stft=stft)
        with pytest.raises(ValueError, match="filt"):
            run(seed=1, prior_filter=F[:, :, :-1], prior_stft=stft)
        with pytest.raises(ValueError, match="multiple of hop_length"):
            run(seed=1, prior_filter=F, prior_stft=stft, lengths=[L, 300])
    with pytest.raises(ValueError, match="one audio channel"):
        smp.sampling(net, (B, 2, L), smp.calc_diffusion_hyperparams(S, 1e-4, 0.05), mel, seed=1, prior_filter=F, prior_stft=stft)
    with pytest.raises(ValueError, match=r"\[6, 1024, 1, 262144\] float32 = 6\.44 GB"):      # refused before anything is held
        smp.sampling(net, (1024, 1, 262144), smp.calc_diffusion_hyperparams(S, 1e-4, 0.05), seed=1, prior_filter=F,
                     prior_stft=stft)
    dh = smp.calc_diffusion_hyperparams(50, 1e-4, 0.05)
    with pytest.raises(ValueError, match="prior_filter.*guided"):
        smp.sampling_guided(net, size, dh, measurement=known, operator=lambda x: x, scale=1.0, condition=mel, seed=1,
                            prior_filter=F, prior_stft=stft)

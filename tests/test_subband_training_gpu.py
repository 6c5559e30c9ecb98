"""GPU: ``training_loss(..., pqmf=P)`` -- multi-band training on both backbones.

The models are the smallest of their kind that the engine trains, built through tests/cases.py with four channels in
and out: a mel-conditional WaveNet (2 layers, ``mel_upsample = [2, 2]``: hop 16 with K = 4, L = 256) and a SaShiMi
(``d_model = 8``, one layer, ``pool = [4, 4]``, L = 1024, so 256 sub-band positions).  The WaveNet has 32 channels under
``f32`` -- mel-conditional training is built on the MFMA adjoints, channels % 32 == 0; at 16 channels the engine answers
NotImplementedError with or without sub-bands -- and 64 under ``bf16x6`` (``wn_layer_bx6_supported`` starts there)."""
import pytest
import torch
import torch.nn as nn

from diffwave_sashimi_amd.pqmf import PQMF
from tests import cases

pytestmark = pytest.mark.gpu

K = 4
SMALL = ((256, 64, 128), (128, 32, 64))


def _wavenet(channels):
    return cases.wn_cfg(unconditional=False, res_channels=channels, skip_channels=channels, num_res_layers=2,
                        dilation_cycle=2, mel_upsample=[2, 2], in_channels=K, out_channels=K)


MODELS = {      # name -> (cfg, precision, B, L, mel frames)
    "wavenet-f32": (_wavenet(32), "f32", 2, 256, 16),
    "wavenet-bf16x6": (_wavenet(64), "bf16x6", 2, 256, 16),
    "sashimi-f32": (cases.ss_cfg(d_model=8, n_layers=1, pool=[4, 4], L=1024 // K, in_channels=K, out_channels=K,
                                 diffusion_step_embed_dim_mid=64), "f32", 2, 1024, None),
}


def _step(gpu, name, mode, **kw):
    """Loss, ``parts`` and every parameter gradient of one seeded call.  ``mode``: ``pqmf`` hands the waveform and the
    bank, ``bands`` hands ``P.analysis(audio)`` as the audio of a plain call."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    cfg, precision, B, L, frames = MODELS[name]
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    net = cases.build_ours(cfg, 5).to(gpu).train()
    if precision != "f32":
        net.set_option("precision", precision)
    audio = (torch.rand(B, 1, L, generator=torch.Generator().manual_seed(8)) * 0.6 - 0.3).to(gpu)
    mel = None if frames is None else cases.mel_inputs(B, frames, 9).to(gpu)
    P = PQMF(K)
    parts = {}
    gen = torch.Generator().manual_seed(3)
    if mode == "pqmf":
        loss = training_loss(net, nn.MSELoss(), audio, dh, mel_spec=mel, generator=gen, pqmf=P,
                             **(dict(kw, parts=parts) if kw else {}))
    else:
        loss = training_loss(net, nn.MSELoss(), P.analysis(audio), dh, mel_spec=mel, generator=gen)
    loss.backward()
    return loss.detach(), parts, {n: p.grad.detach().clone() for n, p in net.named_parameters()}


@pytest.mark.parametrize("name", list(MODELS))
def test_pqmf_call_is_the_plain_call_on_the_subbands(gpu, name):
    loss, _, grads = _step(gpu, name, "pqmf")
    want, _, want_grads = _step(gpu, name, "bands")
    assert torch.isfinite(loss) and float(loss) > 0
    assert torch.equal(loss, want)
    assert sorted(grads) == sorted(want_grads) and len(grads) > 10
    for n in grads:
        assert torch.equal(grads[n], want_grads[n]), n
    assert grads["final_conv.2.conv.weight"].abs().max() > 0


@pytest.mark.parametrize("name", list(MODELS))
def test_spectral_term_on_the_synthesised_estimate(gpu, name):
    plain, _, plain_grads = _step(gpu, name, "pqmf")
    loss, parts, grads = _step(gpu, name, "pqmf", stft_weight=0.5, stft_resolutions=SMALL)
    print(f"{name}: loss {float(loss):.6f} = eps {float(parts['eps']):.6f} + 0.5 x stft {float(parts['stft']):.6f}")
    assert torch.isfinite(loss) and set(parts) == {"eps", "stft"}
    assert torch.equal(parts["eps"], plain) and float(parts["stft"]) > 0
    assert abs(float(loss) - (float(parts["eps"]) + 0.5 * float(parts["stft"]))) <= 1e-6 * abs(float(loss))
    assert all(torch.isfinite(g).all() for g in grads.values())
    key = "final_conv.2.conv.weight"
    assert not torch.equal(grads[key], plain_grads[key])            # the term reaches eps_theta through the bank's adjoint


def test_prior_std_with_pqmf_is_refused(gpu):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    audio = torch.zeros(2, 1, 256, device=gpu)
    with pytest.raises(ValueError, match="prior_std"):
        training_loss(None, nn.MSELoss(), audio, dh, pqmf=PQMF(K), prior_std=torch.ones(2, 1, 256, device=gpu))

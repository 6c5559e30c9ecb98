"""GPU: the adaptive prior's sigma kernel (``dws_prior_std_from_mel``) against the float64 definitions, and the weighted
training loss on an engine model."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import prior_reference as ref

pytestmark = pytest.mark.gpu

E_MAX, E_MIN, STD_MIN = 8.0, 0.25, 0.1


def _mel():
    """[3, 80, 3] in the log-mel range U(-11.5, 2) (frame energies 6 .. 7: unclamped at E_MAX = 8), but clip 0's frame 0
    silent (the clip floor log 1e-5 in every band: the lower clamp) and clip 1's frame 1 loud (2 in every band: energy 24,
    the upper clamp)."""
    mel = cases.mel_inputs(3, 3, 91).clone()
    mel[0, :, 0] = float(np.log(1e-5))
    mel[1, :, 1] = 2.0
    return mel


def _yardstick(mel):
    """Worst relative error of torch's own fp32 evaluation of the formula against float64 on the SAME inputs: the mel of
    the case, [B, 80, frames].  (Every case of the parametrised test holds clip 0's silent frame, where fp32(0.1) stands
    1.49e-08 off 0.1: no case has a zero yardstick.)"""
    e = torch.sqrt(torch.exp(mel).sum(dim=1))
    sf = ((e - np.float32(E_MIN)) / (np.float32(E_MAX) - np.float32(E_MIN))).clamp(STD_MIN, 1.0)
    want = ref.prior_std(mel, 1, energy_max=E_MAX, energy_min=E_MIN, std_min=STD_MIN)[:, 0]
    return float(np.abs(sf.double().numpy() / want - 1).max())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("cut", [0, 3])
@pytest.mark.parametrize("hop", [256, 6])
@pytest.mark.parametrize("frames", [1, 3])
def test_sigma_kernel_against_float64(gpu, frames, hop, cut, B):
    """The kernel may err at most 4 x what torch's fp32 evaluation errs on the case's own mel (another summation order,
    the device exp).
    Rows of B = 3 start at b L: with L = frames hop - 3 they are not 16-byte aligned, so the single-float head and tail
    of the store run; hop = 6 puts frame borders inside a float4."""
    from diffwave_sashimi_amd.mel import prior_std_from_mel
    mel = _mel()[:B, :, :frames].contiguous()
    L = frames * hop - cut
    kw = dict(energy_max=E_MAX, energy_min=E_MIN, std_min=STD_MIN)
    got = prior_std_from_mel(mel.to(gpu), hop, L, **kw)
    assert got.shape == (B, 1, L) and got.device.type == "cuda" and got.dtype == torch.float32
    want = ref.prior_std(mel, hop, L, **kw)
    err = float(np.abs(got.double().cpu().numpy() / want - 1).max())
    torch_err = _yardstick(mel)
    bound = 4 * torch_err
    print(f"sigma kernel frames={frames} hop={hop} L={L} B={B}: worst relative error {err:.3e} "
          f"(torch fp32: {torch_err:.3e}, bound {bound:.3e})")
    assert err <= bound
    # whole frames repeat one value; both clamps are hit exactly
    g = got.cpu()
    for f in range(frames):
        seg = g[:, 0, f * hop:min((f + 1) * hop, L)]
        assert torch.equal(seg, seg[:, :1].expand_as(seg))
    assert float(g[0, 0, 0]) == np.float32(STD_MIN)
    if B > 1 and frames > 1:
        assert float(g[1, 0, hop]) == 1.0
    # a clip's row is its B = 1 evaluation, bit for bit
    for b in range(B):
        assert torch.equal(prior_std_from_mel(mel[b:b + 1].to(gpu), hop, L, **kw), got[b:b + 1])


def test_sigma_kernel_beyond_one_block_and_its_refusals(gpu):
    """70 frames: two workgroups of 64 frames per clip, the second partly filled; L ends inside a frame."""
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.mel import prior_std_from_mel
    mel = cases.mel_inputs(2, 70, 93)
    hop, L = 5, 70 * 5 - 2
    kw = dict(energy_max=E_MAX, energy_min=E_MIN, std_min=STD_MIN)
    got = prior_std_from_mel(mel.to(gpu), hop, L, **kw)
    want = ref.prior_std(mel, hop, L, **kw)
    err, torch_err = float(np.abs(got.double().cpu().numpy() / want - 1).max()), _yardstick(mel)
    print(f"sigma kernel, 70 frames: worst relative error {err:.3e} (torch fp32: {torch_err:.3e})")
    assert err <= 4 * torch_err
    # the entry's own checks (the Python surface refuses the same before it calls)
    lib, st = _lib.load(), _lib.current_stream()
    m, out = mel.to(gpu), torch.zeros(2, 1, L, device=gpu)
    call = lambda L_=L, e0=E_MIN, e1=E_MAX, s=STD_MIN: lib.dws_prior_std_from_mel(m.data_ptr(), 2, 80, 70, hop, L_, e0, e1, s,
                                                                                    out.data_ptr(), st)
    assert call() == 0
    for bad in (dict(L_=70 * hop + 1), dict(L_=0), dict(e0=8.0), dict(e1=float("inf")), dict(s=0.0), dict(s=1.5)):
        assert call(**bad) == _lib.DWS_ERR_INVALID, bad
    torch.cuda.synchronize()
    assert torch.equal(out, got)


# ---------------------------------------------------------------------------------------------------------- training
def test_training_loss_with_a_prior_on_an_engine_model(gpu):
    """wn_cond_c64, the smallest mel-conditional WaveNet the engine trains (mel-conditional training needs the MFMA adjoints,
    channels % 32 == 0: wn_cond_tiny, 16 channels, is refused with or without a prior).  sigma from the batch's own mel."""
    from diffwave_sashimi_amd.mel import prior_std_from_mel
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    cfg, B, L, Tmel, wseed, iseed, _ = cases.WAVENET_COND_CASES["wn_cond_c64"]
    net = cases.build_ours(cfg, wseed).to(gpu).train()
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    audio = (torch.rand(B, 1, L, generator=torch.Generator().manual_seed(iseed)) * 0.6 - 0.3).to(gpu)
    mel = cases.mel_inputs(B, Tmel, iseed).to(gpu)
    sigma = prior_std_from_mel(mel, 256, L, energy_max=7.0)
    assert float(sigma.min()) >= 0.1 and float(sigma.max()) <= 1.0 and float(sigma.std()) > 0
    seen = []
    hook = net.register_forward_hook(lambda mod, args, out: seen.append(out.detach()))
    loss = training_loss(net, None, audio, dh, mel_spec=mel, generator=torch.Generator().manual_seed(29), prior_std=sigma)
    hook.remove()
    gen = torch.Generator().manual_seed(29)
    torch.randint(50, size=(B, 1, 1), generator=gen)
    z = torch.normal(0, 1, size=audio.shape, generator=gen)
    want = ref.loss(seen[0], z, sigma)
    print(f"engine loss with a prior {float(loss.detach()):.6f}, float64 from the engine's eps {want:.6f}")
    assert abs(float(loss.detach()) - want) <= 1e-5 * abs(want)
    loss.backward()
    for name, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert any(float(p.grad.abs().max()) > 0 for p in net.parameters())
    # what training refuses stays refused
    with pytest.raises(NotImplementedError):
        net((audio, torch.zeros(B, 1, device=gpu)), mel_spec=mel, lengths=[L, L - 256])

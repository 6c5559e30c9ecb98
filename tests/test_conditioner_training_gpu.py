"""GPU: the adjoint of the mel conditioner (`csrc/conditioner_train.hip`: `mel_upsample_bwd_input_kernel`,
`mel_upsample_bwd_weight_kernel`, `conditioner_backward`) at strides that are no power of two, with the rule of
tests/gradcheck.py (`compare` with `kink=`: the conditioner's LeakyReLU is bracketed by `_shifted_gates`).  The other
conditional gradient tests run `mel_upsample=[16, 16]` (WaveNet C = 64 / 128, SaShiMi d_model = 32) and `[32, 64]` (SaShiMi).

Every case also asserts that each `upsample_conv2d.{0,1}.{weight_g, weight_v, bias}` and `mel_conv.conv.*` tensor of every
layer has a non-zero oracle gradient, and that the conditioner tensors alone meet the plain 1e-3 (`weight_v` of the
1-input-channel upsamplers: what `compare` grants for that family, no more).

Not covered: position-resolved cotangents, gradients with respect to the mel (not computed by the engine), the grid-stride
loops of the adjoint kernels (T0 > 262144).  The `O % 32 != 0` plain-FMA branch of `conditioner_backward` is reached by the
SaShiMi d_model = 8 case (H = 8, 16) only: WaveNet refuses mel-conditional training at every width with `2C % 32 != 0`
(C = 8, 24, 40 tried: `forward_train` needs the MFMA adjoints, channels % 32 == 0), which
`test_wavenet_refuses_conditional_training_below_the_mfma_widths` pins instead of a gradient case."""
import pytest
import torch
import torch.nn as nn

from tests import cases, gradcheck
from tests.test_conditioner_gpu import lengths, ss_blocks, ss_cond_cfg, wn_cond_cfg, wn_prefixes
from tests.test_sashimi_training_gpu import _engine_and_oracle as sashimi_engine_and_oracle
from tests.test_wavenet_training_gpu import _engine_and_oracle as wavenet_engine_and_oracle

pytestmark = pytest.mark.gpu

COND_SUFFIXES = tuple(f"upsample_conv2d.{i}.{t}" for i in (0, 1) for t in ("weight_g", "weight_v", "bias")) + \
    tuple(f"mel_conv.conv.{t}" for t in ("weight_g", "weight_v", "bias"))


def check_conditioner_gradients(label, prefixes, got, o32, truth, kink):
    worst, k = gradcheck.compare(got, o32, truth, label=label, kink=kink)       # every tensor, the shared rule
    names = [f"{p}.{s}" for p in prefixes for s in COND_SUFFIXES]
    assert len(names) == 9 * len(prefixes) and all(n in o32 for n in names)
    dead = [n for n in names if not float(o32[n].abs().max()) > 0]
    assert not dead, dead                                                        # every conditioner tensor carries gradient
    gmax = max(float(v.abs().max()) for v in truth.values())
    err = {n: float((got[n].double() - o32[n].double()).abs().max()) / gradcheck._scale(truth[n], gmax) for n in names}
    plain = {n: e for n, e in err.items() if not n.endswith(("upsample_conv2d.0.weight_v", "upsample_conv2d.1.weight_v"))}
    wn, wp = max(err, key=err.get), max(plain, key=plain.get)
    print(f"{label}: worst gradient {worst:.3e} ({k}); conditioner: worst {err[wn]:.3e} ({wn}), "
          f"worst outside the upsamplers' weight_v {plain[wp]:.3e} ({wp})")
    assert plain[wp] < gradcheck.TOL, (wp, plain[wp])


WN_CASES = {
    # generic forward recompute inside conditioner_backward (odd strides), dvalid = L < T1 = 606, MFMA branch (O = 128)
    "c64_3x5_ragged": ([3, 5], 40, 500, 2, 2),
    # one mel shared by the batch ([1, 80, Tmel], expanded by the module), even strides that are no power of two / a power of two, L = T1
    "c64_6x4_shared_mel": ([6, 4], 20, 480, 2, 1),
}


@pytest.mark.parametrize("name", list(WN_CASES))
def test_wavenet_conditioner_gradients_match_autograd(gpu, name):
    strides, Tmel, L, B, Bm = WN_CASES[name]
    cfg = wn_cond_cfg(strides, C=64)
    assert lengths(Tmel, strides)[1] == {"c64_3x5_ragged": 606, "c64_6x4_shared_mel": 480}[name] >= L
    mel = torch.cat([cases.mel_inputs(1, Tmel, 51 + i) for i in range(Bm)])
    got, o32, truth, loss, ref_loss, kink = wavenet_engine_and_oracle(cfg, B, L, gpu, 45, 49, 53, mel=mel)
    assert abs(loss - ref_loss) < 1e-5 * max(1.0, abs(ref_loss))
    check_conditioner_gradients(name, wn_prefixes(cfg), got, o32, truth, kink)


@pytest.mark.parametrize("C", [8, 24, 40])
def test_wavenet_refuses_conditional_training_below_the_mfma_widths(gpu, C):
    """The narrowest trainable conditional WaveNet has C % 32 == 0 (2C % 32 == 0): no WaveNet reaches the plain-FMA branch of
    `conditioner_backward`.  The refusal is loud (DWS_ERR_UNSUPPORTED -> NotImplementedError), and sampling still works."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    strides, Tmel, L, B = [5, 3], 3, 40, 2                  # T1 = 49
    net = cases.build_ours(wn_cond_cfg(strides, C=C), 46).to(gpu).train()
    audio = (torch.randn(B, 1, L, generator=torch.Generator().manual_seed(1)) * 0.3).to(gpu)
    mel = cases.mel_inputs(B, Tmel, 52).to(gpu)
    with pytest.raises(NotImplementedError, match="MFMA adjoints"):
        training_loss(net, nn.MSELoss(), audio, calc_diffusion_hyperparams(50, 1e-4, 0.05), mel_spec=mel,
                      generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        assert torch.isfinite(net.eval()((audio, torch.zeros(B, 1, device=gpu)), mel_spec=mel)).all()


@pytest.mark.parametrize("d_model", [8, 32])
def test_sashimi_conditioner_gradients_match_autograd(gpu, d_model):
    """Strides [3, 5], Tmel = 36: T1 = 546 frames of which the stages keep the first 512 / 128 / 32, so most of u1 gets a zero
    cotangent at the pooled stages.  d_model = 8: H = 8, 16 take the plain-FMA GEMM of `conditioner_backward` (`O % 32 != 0`),
    H = 32 the MFMA one; d_model = 32: MFMA at every stage."""
    strides, Tmel, L, B = [3, 5], 36, 512, 2
    cfg = ss_cond_cfg(strides, L, d_model=d_model)
    assert lengths(Tmel, strides)[1] == 546
    mel = torch.cat([cases.mel_inputs(1, Tmel, 61 + i) for i in range(B)])
    net, got, o32, truth, loss, ref_loss, kink = sashimi_engine_and_oracle(cfg, B, gpu, 55, 59, 63, mel=mel, start=0, tries=1)
    assert abs(loss - ref_loss) < 1e-4 * max(1.0, abs(ref_loss))
    check_conditioner_gradients(f"d{d_model}", [p for p, _, _ in ss_blocks(cfg)], got, o32, truth, kink)

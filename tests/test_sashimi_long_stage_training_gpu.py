"""GPU: SaShiMi training on stages the fused in-LDS FFT convolution does not hold -- odd stage lengths and stages longer
than 16384 samples (`configs/experiment/ljspeech_harder.yaml`: segment_length 44000, hop 2048, mel_upsample [32, 64]).
Such blocks run the rocFFT convolution (R2C / spectrum multiply / C2R over 2L-padded rows) and its adjoint
(`sashimi_train_long.hip`); every parameter gradient against the oracle's autograd (fp32, with float64 as the yardstick)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import cases
from tests.conftest import rel_err
from tests.test_sashimi_training_gpu import _engine_and_oracle

pytestmark = pytest.mark.gpu

LONG_CASES = {
    # stages 2000 / 500 on the fused convolution, 125 (odd, H = 128) on rocFFT
    "odd_bottom": (cases.ss_cfg(d_model=32, n_layers=1, L=2000, diffusion_step_embed_dim_mid=64), 2),
    # 16400 (> 16384) and 1025 (odd) on rocFFT, 4100 fused: a mixed model, the fused stage's kernels generated stacked
    "long_top": (cases.ss_cfg(d_model=16, n_layers=1, L=16400), 1),
}

# the S4 parameters of a block whose gradients come out of the rocFFT-stage adjoint
_S4 = (".layer.kernel.kernel.C", ".layer.kernel.kernel.B", ".layer.kernel.kernel.P", ".layer.kernel.kernel.inv_w_real",
       ".layer.kernel.kernel.w_imag", ".layer.kernel.kernel.log_dt", ".layer.D", ".fc_t.weight")


def _long_blocks(cfg):
    """Prefixes of the blocks whose stage runs on rocFFT (odd length or > 16384 samples)."""
    L, H, pool, n = cfg["L"], cfg["d_model"], cfg["pool"], cfg["n_layers"]
    lengths, idx, out = [], 0, []
    for p in pool:
        lengths += [(f"d_layers.{idx + i}", L) for i in range(n)]
        idx += n + 1
        L //= p
    lengths += [(f"c_layers.{i}", L) for i in range(n)]
    idx = 0
    for p in reversed(pool):
        L *= p
        lengths += [(f"u_layers.{idx + 1 + i}", L) for i in range(n)]
        idx += n + 1
    return [pre for pre, Ls in lengths if Ls % 2 or Ls > 16384]


# Weight norm of a conv with ONE input tap (init_conv: [D][1][1]) normalises every output channel's single weight: W = g sign(v),
# so d loss / d v is zero in exact arithmetic and what any fp32 evaluation returns for it is rounding of |dW| g / |v|.  Measured
# against the 1e-5 gmax floor of gradcheck's scale that rounding alone reaches 1.1e-3 on long_top (the oracle's own fp32: 1.4e-4).
# Checked here as what it is -- rounding-sized next to the largest gradient -- and left out of the per-tensor comparison.
_ZERO_BY_CONSTRUCTION = ("init_conv.0.conv.weight_v",)


def _split_zero(got, o32, truth):
    gmax = max(float(v.abs().max()) for v in truth.values())
    for k in _ZERO_BY_CONSTRUCTION:
        assert float(truth[k].abs().max()) <= 1e-9 * gmax, k
        assert float(got[k].abs().max()) <= 1e-6 * gmax, (k, float(got[k].abs().max()) / gmax)
    keep = lambda d: {k: v for k, v in d.items() if k not in _ZERO_BY_CONSTRUCTION}
    return keep(got), keep(o32), keep(truth)


def _check_case(gpu, name, precision="f32", also=()):
    from tests import gradcheck
    cfg, B = LONG_CASES[name]
    net, got, o32, truth, loss, ref_loss, kink = _engine_and_oracle(cfg, B, gpu, 15, 19, 23, start=0, tries=1,
                                                                    precision=precision, also=also)
    assert abs(loss - ref_loss) < 1e-4 * max(1.0, abs(ref_loss))
    got, o32, truth = _split_zero(got, o32, truth)
    long_blocks = _long_blocks(cfg)
    assert long_blocks
    for pre in long_blocks:                     # the rocFFT-stage blocks' S4 gradients are really there
        for suf in _S4:
            assert float(got[pre + suf].abs().max()) > 0, pre + suf
    worst, worst_k = gradcheck.compare(got, o32, truth, label=f"{name} {precision}", kink=kink)
    e64 = gradcheck.errors(got, truth)
    k64 = max(e64, key=e64.get)
    print(f"{name} {precision}: worst vs oracle fp32 {worst:.3e} ({worst_k}); vs float64 {e64[k64]:.3e} ({k64})")
    return net, got, truth


@pytest.mark.parametrize("name", list(LONG_CASES))
def test_long_stage_parameter_gradients_match_autograd(gpu, name):
    _check_case(gpu, name)


def test_long_stage_bf16x6_gradients_are_those_of_the_f32_path(gpu):
    """precision="bf16x6" on the mixed model: against float64 no further than 2x the f32 path's worst tensor (the yardstick
    of test_sashimi_training_gpu.py::test_sashimi_bf16x6_training_gradients_are_those_of_the_f32_path)."""
    from tests import gradcheck
    net, got, truth = _check_case(gpu, "long_top", precision="bf16x6", also=("f32",))
    f32 = {k: v for k, v in net.extra_grads["f32"].items() if k in got}
    e6, e32 = gradcheck.errors(got, truth), gradcheck.errors(f32, truth)
    k6, k32 = max(e6, key=e6.get), max(e32, key=e32.get)
    print(f"long_top: worst gradient error vs float64: bf16x6 {e6[k6]:.3e} ({k6}) | f32 {e32[k32]:.3e} ({k32})")
    assert e6[k6] <= 2.0 * e32[k32]


def test_harder_geometry_gradients_match_autograd(gpu):
    """ljspeech_harder's geometry at d_model 16: stages 44000 / 11000 / 2750 (44000 on rocFFT), the mel conditioner at hop
    2048 (upsamplers of 2 x 32 and 2 x 64 taps), one mel per clip."""
    from tests import gradcheck
    cfg = cases.ss_cfg(d_model=16, n_layers=1, L=44000, pool=[4, 4], unconditional=False, mel_upsample=[32, 64])
    B, Tmel = 2, 22
    mel = torch.cat([cases.mel_inputs(1, Tmel, 51 + i) for i in range(B)])
    net, got, o32, truth, loss, ref_loss, kink = _engine_and_oracle(cfg, B, gpu, 45, 49, 53, mel=mel, start=0, tries=1)
    assert abs(loss - ref_loss) < 1e-4 * max(1.0, abs(ref_loss))
    got, o32, truth = _split_zero(got, o32, truth)
    for pre in ("d_layers.0", "u_layers.3"):
        for suf in _S4 + (".upsample_conv2d.1.weight_v", ".mel_conv.conv.weight_v"):
            assert float(got[pre + suf].abs().max()) > 0, pre + suf
    worst, worst_k = gradcheck.compare(got, o32, truth, label="harder", kink=kink)
    print(f"harder: worst parameter-gradient rel err {worst:.3e} ({worst_k})")


def _loss_and_grads(net, gpu, cfg, B, seed=5):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    audio = (torch.rand(B, 1, cfg["L"], generator=torch.Generator().manual_seed(3)) * 2 - 1) * 0.3
    net.zero_grad(set_to_none=True)
    loss = training_loss(net, nn.MSELoss(), audio.to(gpu), dh, generator=torch.Generator().manual_seed(seed))
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def test_long_stage_backward_is_deterministic(gpu):
    """The batch reduction of the kernel gradient (sum_b conj(U_b) dA_b) runs in a fixed order without atomics: two
    backward passes on the same inputs give the same bits."""
    cfg, _ = LONG_CASES["long_top"]
    net = cases.build_ours(cfg, 15).to(gpu).train()
    l1, g1 = _loss_and_grads(net, gpu, cfg, 2)
    l2, g2 = _loss_and_grads(net, gpu, cfg, 2)
    assert l1 == l2
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_long_stage_training_forward_is_the_sampling_forward(gpu):
    """forward_train (rocFFT stages: padded copy of u, s4_post_train) computes what the eval forward computes."""
    cfg, B = LONG_CASES["long_top"]
    net = cases.build_ours(cfg, 15).to(gpu)
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(B, 1, cfg["L"], generator=g) * 0.5).to(gpu)
    steps = torch.tensor([[17.0]] * B, device=gpu)
    net.train()
    with torch.enable_grad():
        out_train = net((x, steps)).detach().clone()
    net.eval()
    with torch.no_grad():
        out_eval = net((x, steps)).clone()
    err = rel_err(out_train, out_eval)
    print(f"long_top: forward_train vs forward rel err {err:.2e}")
    assert err < 1e-6


def test_long_stage_layernorm_fusion_into_a_rocfft_block(gpu):
    """At H = 128 the previous block's last GEMM writes the next block's LN1(out) + fc_t(e) into its unpadded input rows
    (`ln1_done`); a rocFFT-stage block copies them into the padded transform rows.  Same loss and gradients as with the
    separate LayerNorm passes: 2e-4 as in test_sashimi_training_gpu.py, except for the cancelling sums of gradcheck's
    WIDEN_FAMILIES (log_dt, the LayerNorm scalars), which move with any change of rounding -- at a 16400-sample stage the
    oracle's own fp32 log_dt gradients sit up to 2.5e-3 from float64 (long_top) -- and are held to 5e-3."""
    from tests import gradcheck
    cfg = cases.ss_cfg(d_model=128, n_layers=2, L=16400)
    net = cases.build_ours(cfg, 15).to(gpu).train()
    net.set_option("train_ln_fusion", "1")
    l1, g1 = _loss_and_grads(net, gpu, cfg, 1)
    net.set_option("train_ln_fusion", "0")
    l0, g0 = _loss_and_grads(net, gpu, cfg, 1)
    assert abs(l1 - l0) <= 2e-6 * abs(l0)
    gmax = max(float(v.abs().max()) for v in g0.values())
    diff = {k: float((g1[k] - g0[k]).abs().max()) / max(float(g0[k].abs().max()), 1e-4 * gmax) for k in g0}
    fam = {k: d for k, d in diff.items() if k.endswith(gradcheck.WIDEN_FAMILIES)}
    rest = {k: d for k, d in diff.items() if k not in fam}
    wf, wr = max(fam.items(), key=lambda kv: kv[1]), max(rest.items(), key=lambda kv: kv[1])
    print(f"worst gradient difference fused vs separate: {wr[1]:.2e} ({wr[0]}); cancelling sums {wf[1]:.2e} ({wf[0]})")
    assert wr[1] < 2e-4, wr
    assert wf[1] < 5e-3, wf


def test_train_ljspeech_harder_from_wavs(tmp_path, gpu):
    """`experiment=ljspeech_harder` end to end at d_model 16: 2 s crops of 22050 Hz wavs -> mel at hop 2048 -> conditional
    training steps on a 44000-sample top stage -> checkpoint, finite losses."""
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import local_path_name
    from diffwave_sashimi_amd.train import train
    rng = np.random.default_rng(4)
    data = tmp_path / "wavs"
    os.makedirs(data)
    for i in range(4):
        wavfile.write(str(data / f"LJ00{i}.wav"), 22050, (rng.standard_normal(50000 + 1000 * i) * 2500).astype(np.int16))
    model = dict(cases.ss_cfg(d_model=16, n_layers=2, L=44000, unconditional=False, mel_upsample=[32, 64]))
    ds = dict(_name_="ljspeech", data_path=str(data), segment_length=44000, sampling_rate=22050, filter_length=1024,
              hop_length=2048, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0, valid=False)
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05)
    exp = str(tmp_path / "exp")
    train(0, 1, diff, model, ds, {}, ckpt_iter=-1, n_iters=3, iters_per_ckpt=2, iters_per_logging=1, learning_rate=2e-4,
          batch_size_per_gpu=2, exp_root=exp, num_workers=0)
    run = local_path_name(None, model, diff, ds)
    assert sorted(os.listdir(os.path.join(exp, run, "checkpoint"))) == ["0.pkl", "2.pkl"]
    log = [json.loads(l) for l in open(os.path.join(exp, run, "train_log.jsonl"))]
    losses = [r["train/loss"] for r in log if "train/loss" in r]
    assert len(losses) >= 3 and all(np.isfinite(losses)), losses

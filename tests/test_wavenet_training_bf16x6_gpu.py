"""GPU: WaveNet training under precision="bf16x6" -- forward_train on the split layer kernel (`wn_layer_bx6_kernel`, the
instance that saves the gate pre-activations), the gate adjoint and dskip = Wf^T dy on `tapconv_mfma_kernel<.., SPLIT=1>`,
the res / skip / final_conv.0 weight gradients on `wgrad_dma4_kernel<1>`, the dilated conv's data and weight gradients on
`tapwino_bx6_kernel` and `wgrad_wino_kernel<1>`.  The gradients are held to the rule of the
f32 path (tests/gradcheck.py) and, against FLOAT64, to the f32 path's own error."""
import ctypes

import pytest
import torch
import torch.nn as nn

from tests import cases

pytestmark = pytest.mark.gpu

GRAD_CASES = {
    # MFMA forward (C = 64) + adjoints, 1 M-tile per wave, L % 4 == 0
    "c64": (cases.wn_cfg(res_channels=64, skip_channels=64, num_res_layers=3, dilation_cycle=3), 2, 200, 0),
    # different res / skip widths (gate adjoint K = 256 + 128 at MT = 1, skip weight gradient O = 256, C = 128), L % 4 == 0
    "c128_s256": (cases.wn_cfg(res_channels=128, skip_channels=256, num_res_layers=2, dilation_cycle=2), 1, 132, 4),
    # the same at a ragged L: the 16-byte-only split adjoints fall back to f32, the layer kernel and the Winograd adjoints stay split
    "c128_s256_ragged": (cases.wn_cfg(res_channels=128, skip_channels=256, num_res_layers=2, dilation_cycle=2), 1, 130, 4),
    # 2 M-tiles per wave, dilations up to 64, B > 1, L % 4 == 0: every split instance runs
    "c256": (cases.wn_cfg(res_channels=256, skip_channels=256, num_res_layers=7, dilation_cycle=7), 2, 336, 1),
}


def _loss_and_grads(net, audio, dh, gseed, gpu, precision, mel=None):
    from diffwave_sashimi_amd.training import training_loss
    net.set_option("precision", precision)
    net.zero_grad(set_to_none=True)
    loss = training_loss(net, nn.MSELoss(), audio.to(gpu), dh, mel_spec=None if mel is None else mel.to(gpu),
                         generator=torch.Generator().manual_seed(gseed))
    loss.backward()
    return float(loss.detach()), {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}


def _engine_and_oracle(cfg, B, L, gpu, wseed, aseed, gseed, mel=None, start=0, tries=1):
    """bf16x6 and f32 engine gradients on the same weights / inputs, the oracle's fp32 autograd and its FLOAT64 autograd."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from tests import gradcheck
    net = cases.build_ours(cfg, wseed)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    audio, gseed, loss_of, truth, kink, tried = gradcheck.smooth_case(cfg, sd, dh, B, L, mel, aseed, gseed, start=start, tries=tries)
    net = net.to(gpu).train()
    _, g32 = _loss_and_grads(net, audio, dh, gseed, gpu, "f32", mel)
    loss6, g6 = _loss_and_grads(net, audio, dh, gseed, gpu, "bf16x6", mel)
    loss32, o32 = gradcheck.oracle_grads(cfg, sd, loss_of, torch.float32)
    return g6, g32, {k: o32[k] for k in g6}, {k: truth[k] for k in g6}, loss6, loss32, kink


def _check_bf16x6(label, g6, g32, o32, truth, kink):
    """The rule of test_sashimi_bf16x6_training_gradients_are_those_of_the_f32_path: gradcheck.compare at 1e-3, and against
    float64 the worst tensor within 2x the f32 path's worst, the median tensor within 1.5x, a single tensor beyond 2x its f32
    error only inside 30 % of the 1e-3 bound or inside the f32 path's worst."""
    from tests import gradcheck
    for k, v in g6.items():
        assert torch.isfinite(v).all(), k
    gradcheck.compare(g6, o32, truth, label=label, kink=kink)
    e6, e32 = gradcheck.errors(g6, truth), gradcheck.errors(g32, truth)
    k6, k32 = max(e6, key=e6.get), max(e32, key=e32.get)
    bad = {k: (e6[k], e32[k]) for k in e6 if e6[k] > max(2.0 * e32[k], 0.3 * gradcheck.TOL, e32[k32])}
    med = sorted(e6[k] / max(e32[k], 1e-12) for k in e6)[len(e6) // 2]
    print(f"{label}: worst gradient error vs float64: bf16x6 {e6[k6]:.3e} ({k6}) | f32 {e32[k32]:.3e} ({k32}); "
          f"median ratio bf16x6/f32 {med:.2f}")
    assert any(not torch.equal(g6[k], g32[k]) for k in g6)          # the split kernels really ran
    assert not bad, bad
    assert e6[k6] <= 2.0 * e32[k32] and med <= 1.5


@pytest.mark.parametrize("name", list(GRAD_CASES))
def test_wavenet_bf16x6_training_gradients_are_those_of_the_f32_path(gpu, name):
    cfg, B, L, start = GRAD_CASES[name]
    g6, g32, o32, truth, loss, ref_loss, kink = _engine_and_oracle(cfg, B, L, gpu, 5, 9, 21, start=start)
    assert abs(loss - ref_loss) < 1e-5 * max(1.0, abs(ref_loss))
    _check_bf16x6(name, g6, g32, o32, truth, kink)


def _split_launches(fn):
    """Launches whose ProfileScope name contains "bx6" (the split instances) while fn() runs."""
    from diffwave_sashimi_amd import _lib
    lib = _lib.load()
    _lib.check(lib.dws_profile_enable(b"bx6"))
    try:
        out = fn()
        torch.cuda.synchronize()
        n, ms = ctypes.c_int64(), ctypes.c_double()
        _lib.check(lib.dws_profile_query(ctypes.byref(n), ctypes.byref(ms)))
    finally:
        lib.dws_profile_disable()
    return out, n.value


@pytest.mark.parametrize("L", [336, 333])
def test_which_kernels_run_split_in_a_bf16x6_training_step(gpu, L):
    """Forward: NL split layer launches (`wn_layer_bx6`, any L).  Backward, at any L: per layer the dilated conv's data and
    weight gradients in Winograd form (`tapwino_bx6`, `wgrad_wino_bx6`: 2 NL).  With L % 4 == 0 also dskip = Wf^T dy and the
    final_conv.0 weight gradient (2), per layer the gate adjoint and the skip weight gradient (2 NL) and the res weight
    gradient of every layer but the last (NL - 1): 3 NL + 1 more.  Those stage 16-byte rows: at a ragged L they run f32, and
    the gradients still agree with the f32 path."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    from tests.conftest import rel_err
    cfg, B, _, _ = GRAD_CASES["c256"]
    NL = cfg["num_res_layers"]
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    audio = (torch.randn(B, 1, L, generator=torch.Generator().manual_seed(77)) * 0.3).to(gpu)
    net = cases.build_ours(cfg, 5).to(gpu).train()
    _, g32 = _loss_and_grads(net, audio, dh, 3, gpu, "f32")
    net.set_option("precision", "bf16x6")
    net.zero_grad(set_to_none=True)
    loss, n_fwd = _split_launches(lambda: training_loss(net, nn.MSELoss(), audio, dh, generator=torch.Generator().manual_seed(3)))
    _, n_bwd = _split_launches(lambda: loss.backward())
    g6 = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    print(f"L={L}: split launches forward {n_fwd}, backward {n_bwd}")
    assert n_fwd == NL
    assert n_bwd == 2 * NL + (3 * NL + 1 if L % 4 == 0 else 0)
    top = max(float(g.abs().max()) for g in g32.values())
    worst = max((rel_err(g6[k], g32[k]), k) for k in g32 if float(g32[k].abs().max()) > 1e-6 * top)
    print(f"L={L}: largest bf16x6-vs-f32 gradient difference {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < 2e-4, worst
    assert any(not torch.equal(g6[k], g32[k]) for k in g32)


def test_conditional_wavenet_bf16x6_training_gradients(gpu):
    """Mel-conditional training: the split layer kernel's EXTRA instance adds the mel term and saves H in the same pass."""
    cfg = cases.wn_cfg(unconditional=False, res_channels=64, skip_channels=64, num_res_layers=3, dilation_cycle=3,
                       mel_upsample=[16, 16])
    B, L, Tmel = 2, 500, 2
    mel = torch.cat([cases.mel_inputs(1, Tmel, 31 + i) for i in range(B)])
    g6, g32, o32, truth, loss, ref_loss, kink = _engine_and_oracle(cfg, B, L, gpu, 25, 29, 33, mel=mel, start=4)
    assert abs(loss - ref_loss) < 1e-5 * max(1.0, abs(ref_loss))
    _check_bf16x6("cond_c64", g6, g32, o32, truth, kink)
    seen_cond = sum(("upsample_conv2d" in k or "mel_conv" in k) and float(v.abs().max()) > 0 for k, v in g6.items())
    assert seen_cond >= 9 * cfg["num_res_layers"]


def test_bf16x6_training_gradients_are_deterministic(gpu):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    cfg, B, L, _ = GRAD_CASES["c256"]
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    audio = torch.randn(B, 1, L, generator=torch.Generator().manual_seed(12)) * 0.3
    net = cases.build_ours(cfg, 5).to(gpu).train()
    l1, g1 = _loss_and_grads(net, audio, dh, 4, gpu, "bf16x6")
    l2, g2 = _loss_and_grads(net, audio, dh, 4, gpu, "bf16x6")
    assert l1 == l2
    assert all(torch.equal(g1[k], g2[k]) for k in g1), [k for k in g1 if not torch.equal(g1[k], g2[k])][:5]


def test_full_size_bf16x6_training_step(gpu):
    """BASELINE config 2's network (C = S = 256, 36 layers, cycle 12), B = 2, L = 16000.  Yardstick measured here: the f32
    gradients of the direct convolution against those of the Winograd form.  Per tensor the bf16x6 gradient sits within 2x
    that distance of the f32 (Winograd) one, or within 1e-5 of the tensor's largest value."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    cfg = cases.wn_cfg(res_channels=256, skip_channels=256, num_res_layers=36, dilation_cycle=12)
    B, L = 2, 16000
    dh = calc_diffusion_hyperparams(200, 1e-4, 0.02)
    audio = torch.randn(B, 1, L, generator=torch.Generator().manual_seed(8)) * 0.3
    net = cases.build_ours(cfg, 41).to(gpu).train()
    _, gw = _loss_and_grads(net, audio, dh, 6, gpu, "f32")
    net.set_option("conv_algo", "direct")
    _, gd = _loss_and_grads(net, audio, dh, 6, gpu, "f32")
    net.set_option("conv_algo", "winograd")
    _, g6 = _loss_and_grads(net, audio, dh, 6, gpu, "bf16x6")
    bad, ratios = [], []
    for k in gw:
        assert torch.isfinite(g6[k]).all(), k
        yard = float((gd[k].double() - gw[k].double()).abs().max())
        err = float((g6[k].double() - gw[k].double()).abs().max())
        floor = 1e-5 * float(gw[k].abs().max())
        ratios.append((err / max(yard, 1e-30), k))
        if not (err <= 2.0 * yard or err <= floor):
            bad.append(f"{k}: |bf16x6 - f32| {err:.2e}, |direct - winograd| {yard:.2e}, 1e-5 of max {floor:.2e}")
    ratios.sort(reverse=True)
    print("largest (bf16x6 - f32) / (direct - winograd): " + "; ".join(f"{k} {r:.2f}" for r, k in ratios[:5]))
    assert not bad, "\n".join(bad[:20])


def test_bf16x6_training_reduces_the_loss_and_eval_path_still_works(gpu):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    cfg, B, L, _ = GRAD_CASES["c64"]
    net = cases.build_ours(cfg, 6).to(gpu).train()
    net.set_option("precision", "bf16x6")
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    audio = (torch.randn(B, 1, L, generator=torch.Generator().manual_seed(1)) * 0.3).to(gpu)
    losses = []
    for it in range(8):
        opt.zero_grad()
        loss = training_loss(net, nn.MSELoss(), audio, dh, generator=torch.Generator().manual_seed(3))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0] * 0.9, losses
    net.eval()
    with torch.no_grad():
        out = net((audio, torch.zeros(B, 1, device=gpu)))
    assert torch.isfinite(out).all()


def test_train_cli_wavenet_bf16x6(tmp_path, gpu):
    """`train.py model=wavenet +engine.precision=bf16x6` on synthetic data: four iterations and a checkpoint."""
    import json
    import os

    import numpy as np
    from diffwave_sashimi_amd.generate import load_config, local_path_name
    from diffwave_sashimi_amd.train import train
    from tests.test_train_cli import _tree
    d = _tree(tmp_path / "configs")
    cfg = load_config(d, ["model=wavenet", "model.res_channels=64", "model.skip_channels=64", "model.num_res_layers=4",
                          "model.dilation_cycle=4", "model.in_channels=1", "model.out_channels=1",
                          "model.diffusion_step_embed_dim_in=128", "model.diffusion_step_embed_dim_mid=512",
                          "model.diffusion_step_embed_dim_out=512",
                          "dataset._name_=synthetic", "dataset.segment_length=2048", "dataset.n_items=8",
                          "diffusion.T=20"])
    exp = str(tmp_path / "exp")
    torch.manual_seed(0)
    train(0, 1, diffusion_cfg={k: v for k, v in cfg["diffusion"].items() if k != "beta"}, model_cfg=cfg["model"],
          dataset_cfg=cfg["dataset"], generate_cfg={}, ckpt_iter=-1, n_iters=4, iters_per_ckpt=3, iters_per_logging=1,
          learning_rate=2e-3, batch_size_per_gpu=4, exp_root=exp, num_workers=0, precision="bf16x6")
    run = local_path_name(None, cfg["model"], cfg["diffusion"], cfg["dataset"])
    ck = os.path.join(exp, run, "checkpoint")
    assert sorted(os.listdir(ck)) == ["0.pkl", "3.pkl"]
    saved = torch.load(os.path.join(ck, "3.pkl"), map_location="cpu")
    assert set(saved) == {"model_state_dict", "optimizer_state_dict"}
    log = [json.loads(l) for l in open(os.path.join(exp, run, "train_log.jsonl"))]
    losses = [r["train/loss"] for r in log if "train/loss" in r]
    assert len(losses) == 5 and all(np.isfinite(losses))


@pytest.mark.parametrize("precision", ["bf16x3", "f16x3"])
def test_wavenet_training_refuses_the_other_splits(gpu, precision):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    cfg, B, L, _ = GRAD_CASES["c64"]
    net = cases.build_ours(cfg, 6).to(gpu).train()
    net.set_option("precision", precision)
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    audio = (torch.randn(B, 1, L, generator=torch.Generator().manual_seed(1)) * 0.3).to(gpu)
    with pytest.raises(NotImplementedError):
        training_loss(net, nn.MSELoss(), audio, dh, generator=torch.Generator().manual_seed(3))

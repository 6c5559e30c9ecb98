"""GPU: the gradient w.r.t. the AUDIO input (`dws_model_backward_input`, `audio.requires_grad` through the autograd
wrapper) and the data-only backward that produces nothing else.

`audio.grad` of the `train.py:198-222` MSE loss is held to the project's rule, max|a-b| / max|ref| <= 1e-3, against torch
autograd through the CPU oracle in FLOAT64 on the same state dict, x_t, steps and noise (drawn as
`gradcheck.mse_training_loss` draws them).  The oracle's own fp32 input gradient sits 3e-7 (WaveNet) to 2.6e-6 (SaShiMi)
from float64, so the bound leaves > 300x room for the reference.  The cotangent is dense (2 (eps - z) / n)."""
import ctypes

import pytest
import torch
import torch.nn as nn

from oracle import sashimi as osa
from oracle import wavenet as own
from tests import cases
from tests.conftest import REL_TOL, rel_err
from tests.test_sashimi_training_gpu import TRAIN_CASES as SS_TRAIN
from tests.test_wavenet_training_gpu import COND_TRAIN_CASES as WN_COND, TRAIN_CASES as WN_TRAIN

pytestmark = pytest.mark.gpu

_SS_COND = cases.SASHIMI_COND_CASES["ss_cond_d32"]
# name -> (cfg, B, L, Tmel or None, precisions): bf16x6 where the training tests run the case under it (WaveNet: the MFMA
# adjoints, C % 32 == 0) and on the d32 SaShiMi the guided sampler is tested with
CASES = {
    "wn_tiny": (WN_TRAIN["tiny"][0], 3, 50, None, ("f32",)),
    "wn_c64": (WN_TRAIN["c64"][0], 2, 200, None, ("f32", "bf16x6")),
    "wn_c256": (WN_TRAIN["c256"][0], 2, 333, None, ("f32", "bf16x6")),        # L % 4 != 0
    "wn_cond_c64": (WN_COND["cond_c64"][0], 2, 500, 2, ("f32", "bf16x6")),
    "ss_d32": (SS_TRAIN["d32"][0], 2, 1024, None, ("f32", "bf16x6")),
    "ss_snet": (SS_TRAIN["snet"][0], 3, 512, None, ("f32",)),
    # odd stage lengths (250 / 125: the rocFFT stages), channel counts on the plain-FMA GEMM
    "ss_knobs": (cases.SASHIMI_CASES["ss_knobs"][0], 3, 250, None, ("f32",)),
    "ss_cond_d32": (_SS_COND[0], _SS_COND[1], _SS_COND[0]["L"], _SS_COND[2], ("f32",)),
    # two input / output channels (the data adjoint's Cin = 2 instance)
    "wn_c64_cin2": (dict(WN_TRAIN["c64"][0], in_channels=2, out_channels=2), 2, 200, None, ("f32",)),
    "ss_d32_cin2": (dict(SS_TRAIN["d32"][0], in_channels=2, out_channels=2), 2, 1024, None, ("f32",)),
}
DATA_ONLY_CASES = ["wn_tiny", "wn_c64", "wn_cond_c64", "ss_d32", "ss_knobs", "ss_cond_d32"]


def _build(name, wseed=5):
    cfg, B, L, Tmel, precisions = CASES[name]
    net = cases.build_ours(cfg, wseed)
    if cfg["_name_"] == "sashimi":
        net._setup_C()
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    mel = None if Tmel is None else torch.cat([cases.mel_inputs(1, Tmel, 31 + i) for i in range(B)])
    return cfg, B, L, mel, precisions, net, sd


def _draw(cfg, B, L, aseed=9, gseed=21):
    """x_t, steps, z of the training loss, drawn as `gradcheck.mse_training_loss` draws them."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import q_sample
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    C = cfg["in_channels"]
    audio = torch.randn(B, C, L, generator=torch.Generator().manual_seed(aseed)) * 0.3
    g = torch.Generator().manual_seed(gseed)
    steps = torch.randint(dh["T"], size=(B, 1, 1), generator=g)
    z = torch.normal(0, 1, size=audio.shape, generator=g)
    return q_sample(audio, steps, dh["Alpha_bar"], z), steps.view(B, 1), z


def _oracle_input_grad(cfg, sd, x_t, steps, z, mel):
    def make():
        fwd = own.wavenet_forward if cfg["_name_"] == "wavenet" else osa.sashimi_forward
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        x = x_t.double().requires_grad_(True)
        eps = fwd(sd64, cfg, x, steps, mel_spec=None if mel is None else mel.double())
        loss = nn.MSELoss()(eps, z.double())
        (g,) = torch.autograd.grad(loss, x)
        return float(loss.detach()), g
    return make()


@pytest.fixture(scope="module")
def truth():
    """name -> (inputs, float64 loss and input gradient of the oracle), computed once per case."""
    memo = {}

    def get(name):
        if name not in memo:
            cfg, B, L, mel, precisions, net, sd = _build(name)
            x_t, steps, z = _draw(cfg, B, L)
            memo[name] = (x_t, steps, z, mel, _oracle_input_grad(cfg, sd, x_t, steps, z, mel))
        return memo[name]
    return get


def _engine_input_grad(net, gpu, x_t, steps, z, mel):
    x = x_t.to(gpu).requires_grad_(True)
    eps = net((x, steps.to(gpu)), mel_spec=None if mel is None else mel.to(gpu))
    loss = nn.MSELoss()(eps, z.to(gpu))
    loss.backward()
    return float(loss), x.grad.detach().cpu()


@pytest.mark.parametrize("name,precision", [(n, p) for n, c in CASES.items() for p in c[4]])
def test_audio_gradient_matches_the_float64_oracle(gpu, truth, name, precision):
    cfg, B, L, mel, _, net, sd = _build(name)
    x_t, steps, z, mel, (loss64, g64) = truth(name)
    net = net.to(gpu).eval()
    net.set_option("precision", precision)
    loss, got = _engine_input_grad(net, gpu, x_t, steps, z, mel)
    assert got.shape == x_t.shape and torch.isfinite(got).all()
    err = rel_err(got, g64)
    print(f"{name} {precision}: loss {loss:.7f} / {loss64:.7f}, audio.grad rel err vs float64 {err:.3e} "
          f"(max|grad| {float(g64.abs().max()):.3e})")
    assert abs(loss - loss64) < 1e-4 * max(1.0, abs(loss64))
    assert float(g64.abs().max()) > 0
    assert err < REL_TOL
    assert all(p.grad is None for p in net.parameters())          # eval(): the backward was data-only
    # the same in train() mode, where the parameters take part: the full backward with the input gradient filled
    net.train()
    loss_t, got_t = _engine_input_grad(net, gpu, x_t, steps, z, mel)
    assert all(p.grad is not None for p in net.parameters())
    assert torch.equal(got_t, got)


# ---------------------------------------------------------------------------------------------------------- C ABI
def _abi(net, gpu, x, steps, mel):
    """Bring the engine of `net` to the state before a forward_train of (x, steps, mel)."""
    B, _, L = x.shape
    net._sync_params(L)
    net._prepare(B, L)
    net._set_condition(mel)


def _forward_train(net, x, steps):
    from diffwave_sashimi_amd import _lib
    out = torch.empty(x.shape[0], net.out_channels, x.shape[2], device=x.device)
    _lib.check(_lib.load().dws_model_forward_train(net._handle, x.data_ptr(), steps.data_ptr(), out.data_ptr(),
                                                   _lib.current_stream()))
    return out


def _backward_input(net, dout, param_grads, want=True):
    from diffwave_sashimi_amd import _lib
    da = torch.full((dout.shape[0], net.in_channels, dout.shape[2]), float("nan"), device=dout.device) if want else None
    st = _lib.load().dws_model_backward_input(net._handle, dout.data_ptr(), None if da is None else da.data_ptr(),
                                              param_grads, _lib.current_stream())
    return st, da


def _all_grads(net, gpu):
    from diffwave_sashimi_amd import _lib
    meta = [(k, p) for k, p in net.named_parameters()]
    n = len(meta)
    outs = [torch.empty(p.shape, device=gpu) for _, p in meta]
    names = (ctypes.c_char_p * n)(*[k.encode() for k, _ in meta])
    dsts = (ctypes.c_void_p * n)(*[g.data_ptr() for g in outs])
    numels = (ctypes.c_int64 * n)(*[g.numel() for g in outs])
    _lib.check(_lib.load().dws_model_get_grads(net._handle, n, names, dsts, numels, _lib.current_stream()))
    torch.cuda.synchronize()
    return {k: g for (k, _), g in zip(meta, outs)}


def _abi_inputs(name, gpu, seed):
    cfg, B, L, mel, precisions, net, sd = _build(name)
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, cfg["in_channels"], L, generator=g) * 0.5).to(gpu)
    steps = torch.randint(0, 50, (B,), generator=g).float().to(gpu)
    dout = torch.randn(B, cfg["out_channels"], L, generator=g).to(gpu)
    return net, x, steps, dout, None if mel is None else mel.to(gpu), precisions


@pytest.mark.parametrize("name", DATA_ONLY_CASES)
def test_data_only_and_full_backward_give_the_same_bits(gpu, name):
    from diffwave_sashimi_amd import _lib
    net, x, steps, dout, mel, precisions = _abi_inputs(name, gpu, 77)
    net = net.to(gpu)
    for precision in precisions:
        net.set_option("precision", precision)
        _abi(net, gpu, x, steps, mel)
        _forward_train(net, x, steps)
        st0, da0 = _backward_input(net, dout, 0)
        _forward_train(net, x, steps)
        st1, da1 = _backward_input(net, dout, 1)
        _lib.check(st0), _lib.check(st1)
        torch.cuda.synchronize()
        assert torch.isfinite(da0).all() and float(da0.abs().max()) > 0
        assert torch.equal(da0, da1), f"{name} {precision}: {float((da0 - da1).abs().max()):.3e}"


@pytest.mark.parametrize("name", ["wn_c64", "wn_cond_c64", "ss_d32", "ss_knobs"])
def test_data_only_backward_writes_no_parameter_gradient(gpu, name):
    from diffwave_sashimi_amd import _lib
    net, x, steps, dout, mel, _ = _abi_inputs(name, gpu, 78)
    net = net.to(gpu)
    _abi(net, gpu, x, steps, mel)
    _forward_train(net, x, steps)
    _lib.check(_lib.load().dws_model_backward(net._handle, dout.data_ptr(), _lib.current_stream()))
    before = _all_grads(net, gpu)
    assert any(float(g.abs().max()) > 0 for g in before.values())
    _, x2, steps2, dout2, _, _ = _abi_inputs(name, gpu, 79)            # a different input and cotangent
    _forward_train(net, x2, steps2)
    st, da = _backward_input(net, dout2, 0)
    _lib.check(st)
    after = _all_grads(net, gpu)
    assert all(torch.equal(before[k], after[k]) for k in before)
    # data-only needs a destination
    _forward_train(net, x2, steps2)
    st, _ = _backward_input(net, dout2, 0, want=False)
    assert st == _lib.DWS_ERR_INVALID and b"daudio" in _lib.load().dws_last_error()


@pytest.mark.parametrize("name", ["wn_c64", "ss_d32"])
def test_python_data_only_backward_leaves_every_parameter_gradient_unset(gpu, name):
    net, x, steps, dout, mel, _ = _abi_inputs(name, gpu, 80)
    net = net.to(gpu).eval()
    audio = x.clone().requires_grad_(True)
    out = net((audio, steps.view(-1, 1)), mel_spec=mel)
    (g,) = torch.autograd.grad(out.sum(), audio)
    assert g.shape == audio.shape and float(g.abs().max()) > 0
    assert all(p.grad is None for p in net.parameters())
    assert audio.grad is None          # autograd.grad does not accumulate


@pytest.mark.parametrize("name", ["wn_c64", "ss_d32"])
def test_data_only_backward_delivers_nothing_to_installed_sinks(gpu, name):
    from diffwave_sashimi_amd import _lib
    lib = _lib.load()
    net, x, steps, dout, mel, _ = _abi_inputs(name, gpu, 81)
    net = net.to(gpu)
    _abi(net, gpu, x, steps, mel)
    meta = [(k, p) for k, p in net.named_parameters()]
    n = len(meta)
    sentinel = -12345.5
    dsts = [torch.full(p.shape, sentinel, device=gpu) for _, p in meta]
    names = (ctypes.c_char_p * n)(*[k.encode() for k, _ in meta])
    ptrs = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dsts])
    numels = (ctypes.c_int64 * n)(*[d.numel() for d in dsts])
    groups = (ctypes.c_int32 * n)(*[i % 2 for i in range(n)])
    _lib.check(lib.dws_model_set_grad_sinks(net._handle, n, names, ptrs, numels, groups, 2))
    try:
        _forward_train(net, x, steps)
        st, da = _backward_input(net, dout, 0)
        _lib.check(st)
        torch.cuda.synchronize()
        assert all(bool((d == sentinel).all()) for d in dsts)
        # (the sinks do work: a full backward fills them)
        _forward_train(net, x, steps)
        st, da1 = _backward_input(net, dout, 1)
        _lib.check(st)
        torch.cuda.synchronize()
        assert all(not bool((d == sentinel).any()) for d in dsts)
        assert torch.equal(da, da1)
    finally:
        _lib.check(lib.dws_model_set_grad_sinks(net._handle, 0, None, None, None, None, 0))


@pytest.mark.parametrize("name", ["wn_c64", "wn_cond_c64", "ss_d32"])
def test_parameter_gradients_do_not_depend_on_asking_for_the_input_gradient(gpu, name):
    net, x, steps, dout, mel, _ = _abi_inputs(name, gpu, 82)
    net = net.to(gpu).train()
    grads = []
    for want in (False, True):
        net.zero_grad(set_to_none=True)
        audio = x.clone().requires_grad_(want)
        out = net((audio, steps.view(-1, 1)), mel_spec=mel)
        (out * dout).sum().backward()
        grads.append({k: p.grad.detach().clone() for k, p in net.named_parameters()})
        assert (audio.grad is not None) == want
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in grads[0])


@pytest.mark.parametrize("name", ["wn_c64", "ss_d32"])
def test_input_gradient_refusals(gpu, name):
    net, x, steps, dout, mel, _ = _abi_inputs(name, gpu, 83)
    net = net.to(gpu).eval()
    st = steps.view(-1, 1)
    # under no_grad the eval path runs (no graph, same values as a plain call)
    with torch.no_grad():
        a = net((x.clone().requires_grad_(True), st))
        b = net((x, st))
    assert not a.requires_grad and torch.equal(a, b)
    # ONE pending forward: a backward after another forward is refused
    a1 = x.clone().requires_grad_(True)
    o1 = net((a1, st))
    a2 = x.clone().requires_grad_(True)
    o2 = net((a2, st))
    with pytest.raises(RuntimeError, match="ONE training forward"):
        o1.sum().backward()
    o2.sum().backward()
    assert a2.grad is not None and a1.grad is None
    # the fp16 split has no training forward: the engine's own message, no fallback
    net.set_option("precision", "f16x3")
    with pytest.raises(NotImplementedError, match="training runs with precision"):
        net((x.clone().requires_grad_(True), st))

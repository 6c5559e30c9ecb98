"""GPU: `audio.grad` of a SaShiMi model at a run length OTHER than its kernels' own (`dws_model_forward_input` + the
data-only `dws_model_backward_input`), against torch autograd through the CPU oracle in FLOAT64 -- the form of
tests/test_input_gradient_gpu.py::test_audio_gradient_matches_the_float64_oracle: the MSE training loss on inputs drawn as
`_draw` draws them, max|a - b| / max|ref| <= REL_TOL = 1e-3, eval() mode.

  model (configured length)           run lengths       what it exercises
  SS_TRAIN["d32"] (1024, pool [4, 4]) 512, 2048, 1008   truncated and clamped taps at every stage; at 1008 the stages are
                                                        1008 / 252 / 63: the last an odd rocFFT stage with Lt = 63
                                                        (f32; bf16x6 at 512 and 2048)
  ss_knobs (250, pool [2])            126, 500          channel counts on the plain-FMA GEMM; stages 126 / 63, 500 / 250
  ss_cond_d32 (1024, hop 256)         512, 1536         the mel-conditional route, one mel per clip of frames -+ 2
  d8, one block per level (4096,      66000, B = 1      stages 66000 and 16500 on the segmented convolution (4096 and 1024
  pool [4, 4])                                          taps), 4125 on rocFFT

The oracle's own fp32 gradient lies <= 1.3e-6 from float64 on the unconditional cases.  Also: the launch profile of the
big case; at the kernels' own length the Python path has the bits of `dws_model_forward_train` + `backward_input(0)`; the
refusals that stay; an eval forward is bit-equal before and after such a pair.  Every gradient here raised
NotImplementedError before `dws_model_forward_input` existed."""
import ctypes

import pytest
import torch
import torch.nn as nn

from diffwave_sashimi_amd import _lib
from tests import cases
from tests.conftest import REL_TOL, rel_err
from tests.test_input_gradient_gpu import (_abi, _backward_input, _draw, _engine_input_grad, _forward_train,
                                           _oracle_input_grad)
from tests.test_sashimi_training_gpu import TRAIN_CASES as SS_TRAIN

pytestmark = pytest.mark.gpu

_SS_COND = cases.SASHIMI_COND_CASES["ss_cond_d32"]
HOP = 256
BIG = cases.ss_cfg(d_model=8, n_layers=1, L=4096, pool=[4, 4], diffusion_step_embed_dim_mid=64)
# name -> (cfg, B, conditional)
MODELS = {"d32": (SS_TRAIN["d32"][0], 2, False), "knobs": (cases.SASHIMI_CASES["ss_knobs"][0], 3, False),
          "cond_d32": (_SS_COND[0], _SS_COND[1], True), "big": (BIG, 1, False)}
# (model, run length, precision)
CASES = ([("d32", L, "f32") for L in (512, 2048, 1008)] + [("d32", L, "bf16x6") for L in (512, 2048)]
         + [("knobs", L, "f32") for L in (126, 500)]
         + [("cond_d32", HOP * (_SS_COND[2] + d), "f32") for d in (-2, 2)]
         + [("big", 66000, "f32")])


def _build(model, wseed=5):
    cfg, B, cond = MODELS[model]
    net = cases.build_ours(cfg, wseed)
    net._setup_C()
    return cfg, B, cond, net, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


@pytest.fixture(scope="module")
def truth():
    """(model, L) -> (x_t, steps, z, mel, (float64 loss, float64 input gradient of the oracle)), once per shape."""
    memo = {}

    def get(model, L):
        if (model, L) not in memo:
            cfg, B, cond, net, sd = _build(model)
            assert L != cfg["L"]
            x_t, steps, z = _draw(cfg, B, L)
            mel = torch.cat([cases.mel_inputs(1, L // HOP, 31 + i) for i in range(B)]) if cond else None
            memo[(model, L)] = (x_t, steps, z, mel, _oracle_input_grad(cfg, sd, x_t, steps, z, mel))
        return memo[(model, L)]
    return get


def _profiled(fn, name):
    lib = _lib.load()
    _lib.check(lib.dws_profile_enable(name))
    try:
        out = fn()
        torch.cuda.synchronize()
        n, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
        _lib.check(lib.dws_profile_query(ctypes.byref(n), ctypes.byref(ms)))
    finally:
        lib.dws_profile_disable()
    return out, int(n.value)


@pytest.mark.parametrize("model,L,precision", CASES)
def test_audio_gradient_at_another_run_length_matches_the_float64_oracle(gpu, truth, model, L, precision):
    cfg, B, cond, net, sd = _build(model)
    x_t, steps, z, mel, (loss64, g64) = truth(model, L)
    net = net.to(gpu).eval()
    net.set_option("precision", precision)
    with torch.no_grad():
        before = net((x_t.to(gpu), steps.to(gpu)), mel_spec=None if mel is None else mel.to(gpu))
    loss, got = _engine_input_grad(net, gpu, x_t, steps, z, mel)
    assert got.shape == x_t.shape == (B, 1, L) and torch.isfinite(got).all()
    err = rel_err(got, g64)
    print(f"{model} L={L} (configured {cfg['L']}) {precision}: loss {loss:.7f} / {loss64:.7f}, audio.grad rel err vs float64 "
          f"{err:.3e} (max|grad| {float(g64.abs().max()):.3e})")
    assert abs(loss - loss64) < 1e-4 * max(1.0, abs(loss64))
    assert float(g64.abs().max()) > 0
    assert err < REL_TOL
    assert all(p.grad is None for p in net.parameters())          # the backward was data-only
    # the eval path is untouched by the pair: same bits as before it
    with torch.no_grad():
        after = net((x_t.to(gpu), steps.to(gpu)), mel_spec=None if mel is None else mel.to(gpu))
    assert torch.equal(before, after)
    # train() mode asks for parameter gradients: refused from the forward, as before
    net.train()
    with pytest.raises(NotImplementedError, match="kernels' own length|segmented convolution"):
        net((x_t.to(gpu).requires_grad_(True), steps.to(gpu)), mel_spec=None if mel is None else mel.to(gpu))


def test_big_case_runs_the_segmented_pair(gpu, truth):
    """Stages 66000 and 16500 (two blocks each: down and up) on `fftconv_seg` forward and backward, 4125 on rocFFT."""
    cfg, B, cond, net, sd = _build("big")
    x_t, steps, z, mel, _ = truth("big", 66000)
    net = net.to(gpu).eval()
    counts = {}
    for name in (b"fftconv_seg", b"fftconv", b"long_stage_fwd", b"long_stage_bwd", b"fftcorr"):
        x = x_t.to(gpu).requires_grad_(True)
        eps, nf = _profiled(lambda: net((x, steps.to(gpu))), name)
        _, nb = _profiled(lambda: nn.MSELoss()(eps, z.to(gpu)).backward(), name)
        counts[name.decode()] = (nf, nb)
    print(f"big case launches (forward, backward): {counts}")
    assert counts == {"fftconv_seg": (4, 4), "fftconv": (4, 4), "long_stage_fwd": (1, 0), "long_stage_bwd": (0, 1),
                      "fftcorr": (0, 0)}


@pytest.mark.parametrize("precision", ["f32", "bf16x6"])
def test_at_the_kernels_own_length_the_new_entry_is_forward_train(gpu, precision):
    cfg, B, cond, net, sd = _build("d32")
    L = cfg["L"]
    g = torch.Generator().manual_seed(77)
    x = (torch.randn(B, 1, L, generator=g) * 0.5).to(gpu)
    steps = torch.randint(0, 50, (B,), generator=g).float().to(gpu)
    dout = torch.randn(B, 1, L, generator=g).to(gpu)
    net = net.to(gpu).eval()
    net.set_option("precision", precision)
    audio = x.clone().requires_grad_(True)
    out = net((audio, steps.view(-1, 1)))          # dws_model_forward_input: no parameter in the graph
    out.backward(dout)
    _abi(net, gpu, x, steps, None)
    out_abi = _forward_train(net, x, steps)
    st, da = _backward_input(net, dout, 0)
    _lib.check(st)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), out_abi) and torch.equal(audio.grad, da)


def _forward_input(net, x, steps):
    out = torch.empty(x.shape[0], net.out_channels, x.shape[2], device=x.device)
    return _lib.load().dws_model_forward_input(net._handle, x.data_ptr(), steps.data_ptr(), out.data_ptr(),
                                               _lib.current_stream()), out


@pytest.mark.parametrize("L", [1024, 512])
def test_parameter_gradients_after_the_new_entry_are_a_state_error(gpu, L):
    lib = _lib.load()
    cfg, B, cond, net, sd = _build("d32")
    g = torch.Generator().manual_seed(78)
    x = (torch.randn(B, 1, L, generator=g) * 0.5).to(gpu)
    steps = torch.randint(0, 50, (B,), generator=g).float().to(gpu)
    dout = torch.randn(B, 1, L, generator=g).to(gpu)
    net = net.to(gpu)
    _abi(net, gpu, x, steps, None)
    st, _ = _forward_input(net, x, steps)
    _lib.check(st)
    st, _ = _backward_input(net, dout, 1)
    assert st == _lib.DWS_ERR_STATE and b"dws_model_forward_input" in lib.dws_last_error()
    assert lib.dws_model_backward(net._handle, dout.data_ptr(), _lib.current_stream()) == _lib.DWS_ERR_STATE
    st, da = _backward_input(net, dout, 0)         # the pending forward is still good for what it was made for
    _lib.check(st)
    torch.cuda.synchronize()
    assert torch.isfinite(da).all() and float(da.abs().max()) > 0
    # dws_model_forward_train keeps its refusal at another length
    out = torch.empty_like(x)
    st = lib.dws_model_forward_train(net._handle, x.data_ptr(), steps.data_ptr(), out.data_ptr(), _lib.current_stream())
    assert st == (_lib.DWS_OK if L == cfg["L"] else _lib.DWS_ERR_UNSUPPORTED)
    # f16x3 has no training forward of either kind
    net.set_option("precision", "f16x3")
    st, _ = _forward_input(net, x, steps)
    assert st == _lib.DWS_ERR_UNSUPPORTED and b"training runs with precision" in lib.dws_last_error()


def test_per_clip_lengths_stay_refused(gpu):
    cfg, B, cond, net, sd = _build("d32")
    net = net.to(gpu).eval()
    x = torch.randn(B, 1, 512, generator=torch.Generator().manual_seed(3)).to(gpu)
    steps = torch.zeros(B, 1, device=gpu)
    with pytest.raises(NotImplementedError, match="evaluation calls"):
        net((x.clone().requires_grad_(True), steps), lengths=[512, 256])
    # the engine's own check: lengths installed, then the new entry
    with torch.no_grad():
        net((x, steps), lengths=[512, 256])
    st, _ = _forward_input(net, x, steps.view(-1))
    assert st == _lib.DWS_ERR_UNSUPPORTED and b"per-clip lengths" in _lib.load().dws_last_error()

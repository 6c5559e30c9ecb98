"""GPU: the chunk pipeline of the split WaveNet layer kernel (`csrc/wavenet_bx6.hip`): which waves stage a raw chunk
(all of them, or alternating halves of an eight-wave workgroup), the wait counts that go with either form, the transform
units dealt out among a step's MFMAs, and the one wave's residual copy -- for every instance of the template that a model
reaches, under the 3-term bf16 split (precision="bf16x6") and the 2-term fp16 split ("f16x3").

A wrong wait count or a unit placed before its data shows as a race: results that differ between two runs, or between a
clip run alone and the same clip inside a batch (the tile numbers of its workgroups then differ).  A wrong staging
address or transform shows against the exact-f32 Winograd path, which shares the tile geometry; the bound is the one
tests/test_bf16x6_gpu.py and tests/test_f16x3_gpu.py hold the same pairs to.

Instances: wn_c64 = (C 64, S 64): 2 waves, 16-channel chunks, 4 of them; wn_c128 = (C 128, S 256): 4 waves, 8 chunks, the
skip tiles fetched in the epilogue (no preload); c128_s128 (no case of tests/cases.py has these widths: built here) = the
preloading C = 128 instance; wn_h256_d36 = (C 256, S 256): 8 waves, 32-channel chunks, 8 of them, staged by halves under bf16x6."""
import pytest
import torch

from tests import cases
from tests.conftest import REL_TOL, load_golden, rel_err

pytestmark = pytest.mark.gpu

SPLITS = ("bf16x6", "f16x3")
# 1 / 63 / 1001: rows not 16-byte aligned (dword staging, per-lane epilogue); 600 / 4096 / 4100: 16-byte pieces, the
# contiguous-row form for d <= 16, positions past L in the last pair block; 2052: a multiple of 4 just past the largest
# dilation of a 12-cycle, whose halo tiles then read shifts that lie outside the clip on either side
LENGTHS = (1, 63, 600, 1001, 4096, 4100, 2052)
B = 3

NETS = {
    "wn_c64": lambda: cases.WAVENET_CASES["wn_c64"][0],
    "wn_c128": lambda: cases.WAVENET_CASES["wn_c128"][0],
    "c128_s128": lambda: cases.wn_cfg(res_channels=128, skip_channels=128, num_res_layers=10, dilation_cycle=10),
    "wn_h256_d36": lambda: cases.WAVENET_CASES["wn_h256_d36"][0],
}


def _forward(net, prec, audio, steps):
    net.set_option("precision", prec)
    return net((audio, steps))


@pytest.mark.parametrize("name", list(NETS))
def test_every_instance_at_every_staging_form_is_race_free_and_agrees_with_f32(gpu, name):
    cfg = NETS[name]()
    net = cases.build_ours(cfg, 77).to(gpu)
    for L in LENGTHS:
        audio, steps = cases.wavenet_inputs(B, L, 1, 500 + L)
        audio, steps = audio.to(gpu), steps.to(gpu)
        with torch.no_grad():
            w = _forward(net, "f32", audio, steps)
            for prec in SPLITS:
                s = _forward(net, prec, audio, steps)
                s2 = _forward(net, prec, audio, steps)
                alone = [_forward(net, prec, audio[b:b + 1].contiguous(), steps[b:b + 1].contiguous()) for b in range(B)]
                err = rel_err(s, w)
                print(f"{name} {prec} L={L}: rel err vs the f32 Winograd path {err:.3e}")
                assert torch.equal(s, s2), (name, prec, L)
                for b in range(B):
                    assert torch.equal(alone[b][0], s[b]), (name, prec, L, b)
                assert err < 1e-5, (name, prec, L, err)


LAST_LAYER_NETS = {
    # the last layer has the largest dilation of the cycle (2048): its residual row tile is the one that is never stored
    "c256_d12": dict(res_channels=256, skip_channels=256, num_res_layers=12, dilation_cycle=12),
    # one layer: first and last at once -- the running skip is not read and x is not written
    "c256_d1": dict(res_channels=256, skip_channels=256, num_res_layers=1, dilation_cycle=1),
    "c64_d1": dict(res_channels=64, skip_channels=64, num_res_layers=1, dilation_cycle=1),
    "c128_s256_d1": dict(res_channels=128, skip_channels=256, num_res_layers=1, dilation_cycle=1),
}


@pytest.mark.parametrize("name", list(LAST_LAYER_NETS))
def test_last_layer_skip_output_and_eps(gpu, name):
    cfg = cases.wn_cfg(**LAST_LAYER_NETS[name])
    S = cfg["skip_channels"]
    net = cases.build_ours(cfg, 78).to(gpu)
    for L in (4100, 1001):
        audio, steps = cases.wavenet_inputs(B, L, 1, 600 + L)
        audio, steps = audio.to(gpu), steps.to(gpu)
        with torch.no_grad():
            net.set_option("precision", "f32")
            w = net((audio, steps))
            wp = net.read_tap("pre_final", (B, S, L))
            for prec in SPLITS:
                net.set_option("precision", prec)
                s = net((audio, steps))
                sp = net.read_tap("pre_final", (B, S, L))
                s2 = net((audio, steps))
                e, ep = rel_err(s, w), rel_err(sp, wp)
                print(f"{name} {prec} L={L}: rel err vs f32 eps {e:.3e} pre_final {ep:.3e}")
                assert torch.equal(s, s2), (name, prec, L)
                assert e < 1e-5 and ep < 1e-5, (name, prec, L, e, ep)


def test_conditional_instance_matches_the_reference(gpu):
    """The EXTRA instance (mel term added in the gate stage), as test_bf16x6_conditional_matches_reference holds it."""
    name = "wn_cond_c64"
    cfg, Bc, L, Tmel, wseed, iseed, store = cases.WAVENET_COND_CASES[name]
    g = load_golden("wavenet_cond")
    net = cases.build_ours(cfg, wseed).to(gpu)
    net.set_option("precision", "bf16x6")
    audio, steps = cases.wavenet_inputs(Bc, L, 1, iseed)
    with torch.no_grad():
        for Bm in (1, Bc):
            mel = cases.mel_inputs(Bm, Tmel, iseed).to(gpu)
            eps = net((audio.to(gpu), steps.to(gpu)), mel_spec=mel)
            err = rel_err(eps, g[f"{name}/eps_bm{Bm}"])
            assert err < REL_TOL / 100, f"{name} Bm={Bm}: {err:.3e}"
        eps = net((audio.to(gpu), steps.to(gpu)))
        assert rel_err(eps, g[f"{name}/eps_nomel"]) < REL_TOL / 100


def test_training_instance_saves_the_same_pre_activations_twice(gpu):
    """forward_train under bf16x6 (the EXTRA instance with the H store): eps and the saved gate pre-activations of every
    layer are those of a second run bit for bit, and finite."""
    from diffwave_sashimi_amd import _lib
    cfg, Bt, L, wseed, iseed, _ = cases.WAVENET_CASES["wn_c64"]
    net = cases.build_ours(cfg, wseed).to(gpu).train()
    net.set_option("precision", "bf16x6")
    audio, steps = cases.wavenet_inputs(Bt, L, 1, iseed)
    x, st = audio.to(gpu).contiguous(), steps.to(gpu).float().reshape(-1).contiguous()
    net._sync_params(L)
    net._prepare(Bt, L)
    net._set_condition(None)
    NL, C = cfg["num_res_layers"], cfg["res_channels"]
    runs = []
    for _ in range(2):
        out = torch.empty(Bt, net.out_channels, L, device=gpu)
        _lib.check(_lib.load().dws_model_forward_train(net._handle, x.data_ptr(), st.data_ptr(), out.data_ptr(),
                                                       _lib.current_stream()))
        runs.append((out, net.read_tap("hsave", (NL, Bt, 2 * C, L))))
    torch.cuda.synchronize()
    assert torch.isfinite(runs[0][1]).all() and float(runs[0][1].abs().max()) > 0
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])

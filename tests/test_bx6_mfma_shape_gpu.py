"""GPU: the MFMA shape option of the bf16x6 WaveNet layer kernel at C = S = 256 (`csrc/wavenet_bx6.hip`, set_option
"bx6_mfma"): "16x16x32" runs both GEMMs, the gate stage and the epilogue on v_mfma_f32_16x16x32_bf16 through another
lane -> item map of the same operand bytes (weight fragments, transformed chunks, gate tile, transpose slot);
"gemm2-16x16x32" only GEMM2 and the epilogue.

A wrong map shows against the exact-f32 Winograd path (same tile geometry; the 1e-5 bound of tests/test_bx6_pipeline_gpu.py)
and against the 32x32x16 kernel: both shapes evaluate the same sums in the same order, only that one instruction adds 32
channels where two added 16 + 16, so they differ by one more rounding of the size the 32x32x16 kernel already carries
against f32 -- rel_err(new, old) <= 2 x rel_err(old, f32 path), and the outputs are NOT equal (the option switches kernels).
A race shows as bits that differ between two runs or between a clip alone and the clip inside a batch.
"""
import pytest
import torch

from tests import cases
from tests.conftest import REL_TOL, load_golden, rel_err

pytestmark = pytest.mark.gpu

OLD = "32x32x16"
SHAPES = ("16x16x32", "gemm2-16x16x32")
B = 3
D12 = dict(res_channels=256, skip_channels=256, num_res_layers=12, dilation_cycle=12)
D1 = dict(res_channels=256, skip_channels=256, num_res_layers=1, dilation_cycle=1)


def _net(kw, seed, gpu):
    return cases.cached(("bx6_mfma_net", tuple(sorted(kw.items())), seed), lambda: cases.build_ours(cases.wn_cfg(**kw), seed).to(gpu))


def _run(net, prec, shape, audio, steps, S):
    net.set_option("precision", prec)
    net.set_option("bx6_mfma", shape)
    eps = net((audio, steps))
    return eps, net.read_tap("pre_final", (audio.shape[0], S, audio.shape[2]))


def _check_case(net, L, seed, tag, gpu, NEW):
    S = 256
    audio, steps = cases.wavenet_inputs(B, L, 1, seed)
    audio, steps = audio.to(gpu), steps.to(gpu)
    with torch.no_grad():
        w, wp = _run(net, "f32", OLD, audio, steps, S)
        o, op = _run(net, "bf16x6", OLD, audio, steps, S)
        n, np_ = _run(net, "bf16x6", NEW, audio, steps, S)
        n2, _ = _run(net, "bf16x6", NEW, audio, steps, S)
        alone = [_run(net, "bf16x6", NEW, audio[b:b + 1].contiguous(), steps[b:b + 1].contiguous(), S)[0] for b in range(B)]
    e_new, e_new_p = rel_err(n, w), rel_err(np_, wp)
    e_old, e_old_p = rel_err(o, w), rel_err(op, wp)
    e_no, e_no_p = rel_err(n, o), rel_err(np_, op)
    print(f"{tag} {NEW} L={L}: eps / pre_final rel err  new vs f32 {e_new:.3e} {e_new_p:.3e} | old vs f32 {e_old:.3e} {e_old_p:.3e} | "
          f"new vs old {e_no:.3e} {e_no_p:.3e}")
    assert torch.equal(n, n2), (tag, L)
    for b in range(B):
        assert torch.equal(alone[b][0], n[b]), (tag, L, b)
    assert e_new < 1e-5 and e_new_p < 1e-5, (tag, L, e_new, e_new_p)
    assert not torch.equal(n, o) and not torch.equal(np_, op), (tag, L)
    assert e_no <= 2.0 * e_old and e_no_p <= 2.0 * e_old_p, (tag, L, e_no, e_old, e_no_p, e_old_p)


# 63 / 1001: rows not 16-byte aligned (dword staging, per-lane epilogue); 2052 / 4100: 16-byte pieces, positions past L in
# the last pair block, tiles in block-fastest order for d >= 64, halos outside the clip
@pytest.mark.parametrize("L", [63, 1001, 2052, 4100])
@pytest.mark.parametrize("NEW", SHAPES)
def test_new_shape_at_every_staging_form_and_edge(gpu, NEW, L):
    _check_case(_net(D12, 81, gpu), L, 700 + L, "c256_d12", gpu, NEW)


@pytest.mark.parametrize("L", [4100, 1001])
@pytest.mark.parametrize("NEW", SHAPES)
def test_new_shape_one_layer_network(gpu, NEW, L):
    """First and last layer at once: no skip read, no x written, no residual row tile."""
    _check_case(_net(D1, 82, gpu), L, 800 + L, "c256_d1", gpu, NEW)


@pytest.mark.parametrize("NEW", SHAPES)
def test_new_shape_error_against_float64_is_that_of_the_f32_path(gpu, NEW):
    """The form and bound of test_bf16x6_error_against_float64_is_that_of_the_f32_path, on its C = 256 case."""
    from tests.test_bf16x6_gpu import _f64_oracle
    name = "wn_h256_d36"
    cfg, Bc, L, wseed, iseed, _ = cases.WAVENET_CASES[name]
    net = cases.build_ours(cfg, wseed).to(gpu)
    audio, steps = cases.wavenet_inputs(Bc, L, cfg["in_channels"], iseed)
    ref, ref_pre = cases.cached(("wavenet_f64", name), lambda: _f64_oracle(net, cfg, audio, steps))
    out = {}
    with torch.no_grad():
        for key, prec, shape in (("f32", "f32", OLD), ("old", "bf16x6", OLD), ("new", "bf16x6", NEW)):
            eps, pre = _run(net, prec, shape, audio.to(gpu), steps.to(gpu), cfg["skip_channels"])
            out[key] = (eps.cpu(), pre.cpu())
    e = {p: (rel_err(out[p][0], ref), rel_err(out[p][1], ref_pre)) for p in out}
    rms = {p: float(((out[p][1].double() - ref_pre) ** 2).mean().sqrt() / (ref_pre ** 2).mean().sqrt()) for p in out}
    print(f"{name}: max-rel error vs float64 (eps, pre_final) f32 {e['f32'][0]:.3e} {e['f32'][1]:.3e} | 32x32x16 {e['old'][0]:.3e} "
          f"{e['old'][1]:.3e} | {NEW} {e['new'][0]:.3e} {e['new'][1]:.3e}; rms-rel pre_final f32 {rms['f32']:.3e} "
          f"32x32x16 {rms['old']:.3e} {NEW} {rms['new']:.3e}")
    assert not torch.equal(out["new"][0], out["old"][0])
    for k in (0, 1):
        assert e["new"][k] <= 2.0 * e["f32"][k], (k, e)
    assert rms["new"] <= 2.0 * rms["f32"], rms
    assert rel_err(out["new"][0], load_golden("wavenet")[f"{name}/eps"]) < REL_TOL / 100


@pytest.mark.parametrize("NEW", SHAPES)
def test_new_shape_conditional_instance_agrees_with_f32(gpu, NEW):
    """The EXTRA instance at C = 256 (mel term added in the gate stage), mel batch 1 and B."""
    cfg = cases.wn_cfg(unconditional=False, res_channels=256, skip_channels=256, num_res_layers=3, dilation_cycle=3,
                       mel_upsample=[16, 16])
    L, Tmel = 512, 2
    net = cases.build_ours(cfg, 83).to(gpu)
    audio, steps = cases.wavenet_inputs(B, L, 1, 84)
    audio, steps = audio.to(gpu), steps.to(gpu)
    with torch.no_grad():
        for Bm in (1, B):
            mel = cases.mel_inputs(Bm, Tmel, 85).to(gpu)
            net.set_option("precision", "f32")
            w = net((audio, steps), mel_spec=mel)
            net.set_option("precision", "bf16x6")
            net.set_option("bx6_mfma", OLD)
            o = net((audio, steps), mel_spec=mel)
            net.set_option("bx6_mfma", NEW)
            n = net((audio, steps), mel_spec=mel)
            n2 = net((audio, steps), mel_spec=mel)
            e, eo = rel_err(n, w), rel_err(o, w)
            print(f"conditional c256 {NEW} Bm={Bm}: rel err vs f32  new {e:.3e} old {eo:.3e}  new vs old {rel_err(n, o):.3e}")
            assert torch.equal(n, n2), Bm
            assert not torch.equal(n, o), Bm
            assert e < 1e-5, (Bm, e)


def _forward_train(net, x, st, shape, gpu):
    from diffwave_sashimi_amd import _lib
    out = torch.empty(shape[1], net.out_channels, shape[3], device=gpu)
    _lib.check(_lib.load().dws_model_forward_train(net._handle, x.data_ptr(), st.data_ptr(), out.data_ptr(), _lib.current_stream()))
    return out, net.read_tap("hsave", shape)


@pytest.mark.parametrize("NEW", SHAPES)
def test_new_shape_training_instance(gpu, NEW):
    """forward_train under bf16x6 (the EXTRA instance with the H store) at C = 256: eps and the saved gate pre-activations
    are those of a second run bit for bit, finite, and within 1e-5 of the f32 path's."""
    kw = dict(res_channels=256, skip_channels=256, num_res_layers=3, dilation_cycle=3)
    L, NL, C = 600, 3, 256
    net = cases.build_ours(cases.wn_cfg(**kw), 86).to(gpu).train()
    audio, steps = cases.wavenet_inputs(B, L, 1, 87)
    x, st = audio.to(gpu).contiguous(), steps.to(gpu).float().reshape(-1).contiguous()
    runs = {}
    for key, prec, shape in (("f32", "f32", OLD), ("new", "bf16x6", NEW), ("new2", "bf16x6", NEW)):
        net.set_option("precision", prec)
        net.set_option("bx6_mfma", shape)
        net._sync_params(L)
        net._prepare(B, L)
        net._set_condition(None)
        runs[key] = _forward_train(net, x, st, (NL, B, 2 * C, L), gpu)
    torch.cuda.synchronize()
    assert torch.isfinite(runs["new"][1]).all() and float(runs["new"][1].abs().max()) > 0
    assert torch.equal(runs["new"][0], runs["new2"][0])
    assert torch.equal(runs["new"][1], runs["new2"][1])
    e, eh = rel_err(runs["new"][0], runs["f32"][0]), rel_err(runs["new"][1], runs["f32"][1])
    print(f"forward_train c256 {NEW}: rel err vs f32  eps {e:.3e} hsave {eh:.3e}")
    assert e < 1e-5 and eh < 1e-5, (e, eh)


@pytest.mark.parametrize("NEW", SHAPES)
def test_new_shape_captured_sampler_gives_the_eager_bits(gpu, NEW):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling
    net = _net(D12, 81, gpu)
    net.set_option("precision", "bf16x6")
    net.set_option("bx6_mfma", NEW)
    L, T = 2052, 6
    dh = calc_diffusion_hyperparams(T, 1e-4, 0.05)
    g = torch.Generator().manual_seed(88)
    x_T = torch.randn(B, 1, L, generator=g)
    noise = torch.randn(T, B, 1, L, generator=g)
    a = sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise, use_graph=True)
    b = sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise, use_graph=False)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


def test_option_values(gpu):
    net = _net(D1, 82, gpu)
    with pytest.raises(Exception):
        net.set_option("bx6_mfma", "8x8x8")
    for v in (OLD,) + SHAPES:
        net.set_option("bx6_mfma", v)
    net.set_option("bx6_mfma", OLD)

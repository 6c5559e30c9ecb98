"""GPU: the A-fragment ring option of GEMM1 in the both-GEMM 16x16x32 bf16x6 WaveNet layer kernel at C = S = 256
(`csrc/wavenet_bx6.hip`, set_option "bx6_a_ring"): "half-step" requests the six fragments of a half-step (product, row tile)
one half-step ahead; "quarter-step" runs the half-step as its two row halves and requests three fragments three quarter-steps
ahead, in the same registers.

The rings schedule the same MFMAs: every accumulator receives its start value, the chunks in rotated order and the products in
P::ia / P::ib order under both; only the interleaving between DIFFERENT accumulators moves.  So the one property is bit equality --
a wrong set index, a wrong address of a quarter-step's fragments, a request that overwrites a set still in use or a wait count
that lets a chunk be read before it has landed shows as outputs that differ between the rings, between two runs, or between a
clip alone and the clip inside a batch.  Accuracy (float64, golden, full size, trajectory) is what the existing tests check
for whichever ring is the default.
"""
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu

HALF, QUARTER = "half-step", "quarter-step"
B = 3
D12 = dict(res_channels=256, skip_channels=256, num_res_layers=12, dilation_cycle=12)
D1 = dict(res_channels=256, skip_channels=256, num_res_layers=1, dilation_cycle=1)


def _net(kw, seed, gpu):
    return cases.cached(("bx6_a_ring_net", tuple(sorted(kw.items())), seed), lambda: cases.build_ours(cases.wn_cfg(**kw), seed).to(gpu))


def _run(net, ring, audio, steps, S=256, mfma="16x16x32"):
    net.set_option("precision", "bf16x6")
    net.set_option("bx6_mfma", mfma)
    net.set_option("bx6_a_ring", ring)
    eps = net((audio, steps))
    return eps, net.read_tap("pre_final", (audio.shape[0], S, audio.shape[2]))


def _check_case(net, L, seed, tag, gpu):
    audio, steps = cases.wavenet_inputs(B, L, 1, seed)
    audio, steps = audio.to(gpu), steps.to(gpu)
    with torch.no_grad():
        h, hp = _run(net, HALF, audio, steps)
        q, qp = _run(net, QUARTER, audio, steps)
        q2, qp2 = _run(net, QUARTER, audio, steps)
        alone = [_run(net, QUARTER, audio[b:b + 1].contiguous(), steps[b:b + 1].contiguous()) for b in range(B)]
    assert torch.isfinite(h).all() and float(h.abs().max()) > 0, (tag, L)
    print(f"{tag} L={L}: max |eps| {float(h.abs().max()):.3e}; differing elements quarter vs half: eps {int((q != h).sum())} "
          f"pre_final {int((qp != hp).sum())}")
    assert torch.equal(q, h) and torch.equal(qp, hp), (tag, L)
    assert torch.equal(q2, q) and torch.equal(qp2, qp), (tag, L)
    for b in range(B):
        assert torch.equal(alone[b][0][0], q[b]) and torch.equal(alone[b][1][0], qp[b]), (tag, L, b)


# 63 / 1001: rows not 16-byte aligned (dword staging, per-lane epilogue); 2052 / 4100: 16-byte pieces, positions past L in
# the last pair block, tiles in block-fastest order for d >= 64, halos outside the clip
@pytest.mark.parametrize("L", [63, 1001, 2052, 4100])
def test_rings_give_equal_bits_at_every_staging_form_and_edge(gpu, L):
    _check_case(_net(D12, 91, gpu), L, 900 + L, "c256_d12", gpu)


@pytest.mark.parametrize("L", [63, 1001, 2052, 4100])
def test_rings_give_equal_bits_one_layer_network(gpu, L):
    """First and last layer at once: no skip read, no x written, no residual row tile."""
    _check_case(_net(D1, 92, gpu), L, 1000 + L, "c256_d1", gpu)


def test_rings_give_equal_bits_conditional_instance(gpu):
    """The EXTRA instance at C = 256 (mel term added in the gate stage), mel batch 1 and B."""
    cfg = cases.wn_cfg(unconditional=False, res_channels=256, skip_channels=256, num_res_layers=3, dilation_cycle=3,
                       mel_upsample=[16, 16])
    L, Tmel = 512, 2
    net = cases.build_ours(cfg, 93).to(gpu)
    audio, steps = cases.wavenet_inputs(B, L, 1, 94)
    audio, steps = audio.to(gpu), steps.to(gpu)
    net.set_option("precision", "bf16x6")
    net.set_option("bx6_mfma", "16x16x32")
    with torch.no_grad():
        for Bm in (1, B):
            mel = cases.mel_inputs(Bm, Tmel, 95).to(gpu)
            net.set_option("bx6_a_ring", HALF)
            h = net((audio, steps), mel_spec=mel)
            net.set_option("bx6_a_ring", QUARTER)
            q = net((audio, steps), mel_spec=mel)
            q2 = net((audio, steps), mel_spec=mel)
            assert torch.isfinite(h).all() and float(h.abs().max()) > 0, Bm
            assert torch.equal(q, h), Bm
            assert torch.equal(q2, q), Bm


def _forward_train(net, x, st, shape, gpu):
    from diffwave_sashimi_amd import _lib
    out = torch.empty(shape[1], net.out_channels, shape[3], device=gpu)
    _lib.check(_lib.load().dws_model_forward_train(net._handle, x.data_ptr(), st.data_ptr(), out.data_ptr(), _lib.current_stream()))
    return out, net.read_tap("hsave", shape)


def test_rings_give_equal_bits_training_instance(gpu):
    """forward_train under bf16x6 (the EXTRA instance with the H store) at C = 256: eps and the saved gate pre-activations."""
    kw = dict(res_channels=256, skip_channels=256, num_res_layers=3, dilation_cycle=3)
    L, NL, C = 600, 3, 256
    net = cases.build_ours(cases.wn_cfg(**kw), 96).to(gpu).train()
    audio, steps = cases.wavenet_inputs(B, L, 1, 97)
    x, st = audio.to(gpu).contiguous(), steps.to(gpu).float().reshape(-1).contiguous()
    runs = {}
    net.set_option("precision", "bf16x6")
    net.set_option("bx6_mfma", "16x16x32")
    for key, ring in (("half", HALF), ("quarter", QUARTER), ("quarter2", QUARTER)):
        net.set_option("bx6_a_ring", ring)
        net._sync_params(L)
        net._prepare(B, L)
        net._set_condition(None)
        eps, hs = _forward_train(net, x, st, (NL, B, 2 * C, L), gpu)
        runs[key] = (eps.clone(), hs.clone())
    torch.cuda.synchronize()
    assert torch.isfinite(runs["half"][1]).all() and float(runs["half"][1].abs().max()) > 0
    for k in (0, 1):
        assert torch.equal(runs["quarter"][k], runs["half"][k]), k
        assert torch.equal(runs["quarter2"][k], runs["quarter"][k]), k


def test_captured_sampler_gives_the_eager_bits_under_both_rings(gpu):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling
    net = _net(D12, 91, gpu)
    net.set_option("precision", "bf16x6")
    net.set_option("bx6_mfma", "16x16x32")
    L, T = 2052, 6
    dh = calc_diffusion_hyperparams(T, 1e-4, 0.05)
    g = torch.Generator().manual_seed(98)
    x_T = torch.randn(B, 1, L, generator=g)
    noise = torch.randn(T, B, 1, L, generator=g)
    net.set_option("bx6_a_ring", QUARTER)
    a = sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise, use_graph=True).clone()
    b = sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise, use_graph=False).clone()
    net.set_option("bx6_a_ring", HALF)
    h = sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise, use_graph=False).clone()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert torch.equal(a, h) and torch.equal(b, h)


def test_option_values(gpu):
    net = _net(D1, 92, gpu)
    with pytest.raises(Exception):
        net.set_option("bx6_a_ring", "eighth-step")
    for v in (HALF, QUARTER):
        net.set_option("bx6_a_ring", v)


def test_ring_is_a_no_op_on_the_32x32x16_kernel(gpu):
    """The ring belongs to the 16x16x32 GEMM1: under bx6_mfma = "32x32x16" either value runs the one 32x32x16 kernel."""
    net = _net(D1, 92, gpu)
    audio, steps = cases.wavenet_inputs(B, 1001, 1, 1101)
    audio, steps = audio.to(gpu), steps.to(gpu)
    with torch.no_grad():
        h, hp = _run(net, HALF, audio, steps, mfma="32x32x16")
        q, qp = _run(net, QUARTER, audio, steps, mfma="32x32x16")
        n, _ = _run(net, QUARTER, audio, steps, mfma="16x16x32")
    assert torch.equal(q, h) and torch.equal(qp, hp)
    assert not torch.equal(n, h)   # (the MFMA shape option itself still switches kernels)
    net.set_option("bx6_a_ring", HALF)

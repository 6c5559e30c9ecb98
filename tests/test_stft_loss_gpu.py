"""GPU: ``metrics.mr_stft_loss`` (``dws_spectral_distance`` forwards, ``dws_spectral_loss_backward`` backwards) against
the float64 CPU reference of tests/stft_loss_reference.py, and ``training_loss(stft_weight=)`` on both backbones."""
import pytest
import torch
import torch.nn as nn

from diffwave_sashimi_amd.metrics import mr_stft_loss, spectral_metrics
from tests import cases
from tests import stft_loss_reference as ref
from tests.spectral_reference import KINDS, LENGTHS, RESOLUTIONS, RTOL, signal_pair

pytestmark = pytest.mark.gpu

T_MAX = 4000
CUSTOM = ((64, 16, 48), (128, 200, 128))            # hop > n_fft in the second: samples no frame covers
SC_TOL = RTOL                                       # 1e-5: spectral convergence alone (well conditioned)
FULL_TOL = 2e-3                                     # with the log-magnitude term (1 / |X|^2 at weak bins)
SMALL = ((256, 64, 128), (128, 32, 64))             # the training tests' resolutions


def _batch(kind, fill=0.0):
    """[4, 4000] x and y holding ``signal_pair(kind, n)`` for the four lengths, ``fill`` behind each clip's end."""
    x = torch.full((len(LENGTHS), T_MAX), fill)
    y = torch.full((len(LENGTHS), T_MAX), fill)
    for b, n in enumerate(LENGTHS):
        x[b, :n], y[b, :n] = signal_pair(kind, n)
    return x, y


def _grad(x, y, lengths=None, cot=None, **kw):
    x = x.clone().requires_grad_(True)
    out = mr_stft_loss(x, y, lengths, **kw)
    assert out.dtype == torch.float32 and out.shape == (x.shape[0],) and out.device == x.device
    out.backward(torch.ones_like(out) if cot is None else cot)
    return x.grad, out.detach()


@pytest.mark.parametrize("kind", KINDS)
def test_value_is_spectral_metrics_mr_stft(gpu, kind):
    """Every kind and length (one ragged batch per kind: a clip's number does not depend on the batch): the float32 loss
    is the float64 ``mr_stft`` of ``spectral_metrics`` to one float32 rounding (2^-24 relative)."""
    x, y = (t.to(gpu) for t in _batch(kind))
    want = spectral_metrics(x, y, list(LENGTHS))["mr_stft"]
    got = mr_stft_loss(x, y, list(LENGTHS))
    assert got.dtype == torch.float32 and got.device == x.device and not got.requires_grad
    with_grad = mr_stft_loss(x.clone().requires_grad_(True), y, list(LENGTHS))
    assert with_grad.requires_grad and torch.equal(with_grad.detach(), got)
    for b, n in enumerate(LENGTHS):
        err = abs(float(got[b]) - float(want[b])) / abs(float(want[b]))
        print(f"{kind} {n}: loss {float(got[b]):.7f}, mr_stft {float(want[b]):.9f}, rel {err:.1e}")
        assert err <= 2.0 ** -24 * 1.001


@pytest.mark.parametrize("kind", KINDS)
def test_spectral_convergence_gradient_against_float64(gpu, kind):
    """sc_weight = 1, mag_weight = 0, every kind x length: relative L2 per clip and max-abs error over max |g| both <=
    spectral_reference.RTOL = 1e-5.  The sharp test: the term is well conditioned (|Re / |X|| <= 1).  Measured on the CPU
    over kinds x {1025, 1300, 2500}: a float32 emulation of the kernel's sequential arithmetic <= 1.2e-6 (max-abs 1.3e-6),
    float32 torch <= 3.1e-7; the bound is 8 x the emulation.  Measured on an MI355X over every kind x length: rel L2 <=
    1.16e-6, max-abs <= 1.07e-6."""
    x, y = (t.to(gpu) for t in _batch(kind))
    got, _ = _grad(x, y, list(LENGTHS), sc_weight=1.0, mag_weight=0.0)
    assert torch.isfinite(got).all()
    for b, n in enumerate(LENGTHS):
        want = ref.signal_gradient(kind, n, RESOLUTIONS, 1.0, 0.0)
        assert not got[b, n:].any()
        if kind == "xsilent":
            assert not want.any() and not got[b].any()
            continue
        l2, mx = ref.rel_l2(got[b, :n], want), ref.rel_max(got[b, :n], want)
        print(f"sc only, {kind} {n}: rel L2 {l2:.2e}, max-abs / max|g| {mx:.2e}")
        assert l2 <= SC_TOL and mx <= SC_TOL


@pytest.mark.parametrize("kind", KINDS)
def test_default_weights_gradient_against_float64(gpu, kind):
    """Default weights, every kind x length: relative L2 per clip <= 2e-3.  The 1 / |X|^2 factor of the log-magnitude
    term at weak bins is ill-conditioned in ANY float32 evaluation: measured on the CPU, a float32 emulation of the
    kernel's arithmetic gives <= 7.3e-4 and float32 torch autograd <= 4.7e-4; 2e-3 leaves 2.7 x over the emulation, while
    a wrong reflection, a missing window or a dropped term is O(1e-1).  len = 1025 at n_fft = 2048 reflects every frame
    at both ends; (512, 50, 240) has K = 257 bins (thread 0's second bin).  Measured on an MI355X: <= 5.46e-4 (gain,
    2500); 1.3e-5 .. 2.2e-4 elsewhere."""
    x, y = (t.to(gpu) for t in _batch(kind))
    got, _ = _grad(x, y, list(LENGTHS))
    assert torch.isfinite(got).all()
    for b, n in enumerate(LENGTHS):
        want = ref.signal_gradient(kind, n)
        assert not got[b, n:].any()
        if kind == "xsilent":
            assert not want.any() and not got[b].any()
            continue
        l2 = ref.rel_l2(got[b, :n], want)
        print(f"default weights, {kind} {n}: rel L2 {l2:.2e}")
        assert l2 <= FULL_TOL


def test_exact_zeros(gpu):
    """x = 0: every bin below the floor, the gradient is exactly 0.  x is y: the spectral-convergence numerator and every
    log difference are 0; torch autograd gives NaN (sqrt at 0), the kernel exactly 0."""
    for n in (1025, 2500):
        x, y = (t[None].to(gpu) for t in signal_pair("xsilent", n))
        g, v = _grad(x, y)
        assert torch.isfinite(g).all() and not g.any() and torch.isfinite(v).all()
        g, v = _grad(y, y)
        assert torch.isfinite(g).all() and not g.any() and float(v) == 0.0


def test_ragged_batch_rows_are_their_own_calls(gpu):
    """[4, 4000] of the four lengths with NaN in every padded position of x and y, a random cotangent per clip: a row is
    bit-equal to its own B = 1, T = len call and to its row in the reversed batch, padded positions are exactly 0, and
    two calls give the same bits."""
    x, y = (t.to(gpu) for t in _batch("noise", float("nan")))
    cot = (torch.rand(4, generator=torch.Generator().manual_seed(2)) + 0.5).to(gpu)
    lengths = list(LENGTHS)
    g, v = _grad(x, y, lengths, cot)
    g2, v2 = _grad(x, y, lengths, cot)
    assert torch.equal(g, g2) and torch.equal(v, v2) and torch.isfinite(g).all() and torch.isfinite(v).all()
    gr, vr = _grad(x.flip(0), y.flip(0), lengths[::-1], cot.flip(0))
    assert torch.equal(gr.flip(0), g) and torch.equal(vr.flip(0), v)
    for b, n in enumerate(lengths):
        assert not g[b, n:].any() and g[b, :n].abs().max() > 0
        own, vo = _grad(x[b:b + 1, :n].contiguous(), y[b:b + 1, :n].contiguous(), None, cot[b:b + 1])
        assert torch.equal(own[0], g[b, :n]) and torch.equal(vo[0], v[b])
        # and the cotangent is what scales it: the reference's gradient times cot[b]
        assert ref.rel_l2(g[b, :n] / cot[b], ref.signal_gradient("noise", n)) <= FULL_TOL


def test_custom_resolutions_and_uncovered_samples(gpu):
    """((64, 16, 48), (128, 200, 128)): hop > n_fft in the second, so with it alone the samples no frame covers get
    exactly 0; the pair against float64 at the two bounds above."""
    x, y = signal_pair("noise", 1300)
    xg, yg = x[None].to(gpu), y[None].to(gpu)
    got, _ = _grad(xg, yg, resolutions=CUSTOM)
    l2 = ref.rel_l2(got[0], ref.gradient(x, y, CUSTOM))
    got_sc, _ = _grad(xg, yg, resolutions=CUSTOM, mag_weight=0.0)
    want_sc = ref.gradient(x, y, CUSTOM, 1.0, 0.0)
    l2_sc, mx_sc = ref.rel_l2(got_sc[0], want_sc), ref.rel_max(got_sc[0], want_sc)
    print(f"custom resolutions: default weights rel L2 {l2:.2e}; sc only rel L2 {l2_sc:.2e}, max-abs {mx_sc:.2e}")
    assert l2 <= FULL_TOL and l2_sc <= SC_TOL and mx_sc <= SC_TOL
    only, _ = _grad(xg, yg, resolutions=CUSTOM[1:])
    covered = torch.zeros(1300, dtype=torch.bool)
    for f in range(1300 // 200 + 1):                # frame f covers samples 200 f - 64 .. 200 f + 63
        covered[max(0, 200 * f - 64):200 * f + 64] = True
    assert not only[0, ~covered].any() and only[0, covered].abs().max() > 0
    assert ref.rel_l2(only[0], ref.gradient(x, y, CUSTOM[1:])) <= FULL_TOL


def test_second_derivative_is_an_error_with_a_name(gpu):
    x, y = (t[None].to(gpu) for t in signal_pair("noise", 1300))
    x.requires_grad_(True)
    (g,) = torch.autograd.grad(mr_stft_loss(x, y, resolutions=SMALL).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="second derivative is not built"):
        g.sum().backward()
    with torch.no_grad():                           # grad mode off: the plain forward
        assert not mr_stft_loss(x, y, resolutions=SMALL).requires_grad


# --------------------------------------------------------------------------------------------------------- training
def _training_grads(gpu, cfg, B, L, precision, reference, **kw):
    """Gradients (parameters and audio) of one seeded ``training_loss`` call; with ``reference`` the spectral term is the
    float64 CPU loss applied to the engine's own x0_hat (autograd crosses the devices)."""
    from diffwave_sashimi_amd import metrics
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    net = cases.build_ours(cfg, 5).to(gpu).train()
    if precision != "f32":
        net.set_option("precision", precision)
    audio = (torch.rand(B, 1, L, generator=torch.Generator().manual_seed(8)) * 0.6 - 0.3).to(gpu).requires_grad_(True)

    def cpu_loss(x, y, lengths=None, *, resolutions):
        return ref.loss(x[:, 0], y[:, 0], None, tuple(tuple(r) for r in resolutions)).to(device=x.device, dtype=torch.float32)
    kept = metrics.mr_stft_loss
    if reference:
        metrics.mr_stft_loss = cpu_loss
    try:
        parts = {}
        loss = training_loss(net, nn.MSELoss(), audio, dh, generator=torch.Generator().manual_seed(3), parts=parts, **kw)
        loss.backward()
    finally:
        metrics.mr_stft_loss = kept
    grads = [p.grad.detach().double().flatten().cpu() for _, p in sorted(net.named_parameters())]
    return torch.cat(grads + [audio.grad.double().flatten().cpu()]), loss.detach(), parts


@pytest.mark.parametrize("name", ["wavenet-f32", "wavenet-bf16x6", "sashimi-f32"])
def test_training_gradients_with_the_spectral_term(gpu, name):
    """stft_weight = 0.5 at ((256, 64, 128), (128, 32, 64)): all parameter gradients and audio.grad against the same call
    whose spectral term is the float64 CPU reference on the engine's own x0_hat: relative L2 over all of them <= 2e-3
    (the bound of the loss's own gradient; the network's backward is the same code in both calls)."""
    if name.startswith("wavenet"):      # the smallest WaveNet of tests/cases.py with channels % 32 == 0
        cfg, B, L = cases.WAVENET_CASES["wn_c64"][0], 3, 2048
    else:
        cfg, B, L = cases.SASHIMI_CASES["ss_tiny"][0], 2, 1024
    kw = dict(stft_weight=0.5, stft_resolutions=SMALL)
    precision = name.split("-")[1]
    got, loss, parts = _training_grads(gpu, cfg, B, L, precision, False, **kw)
    want, loss_ref, parts_ref = _training_grads(gpu, cfg, B, L, precision, True, **kw)
    plain, base, _ = _training_grads(gpu, cfg, B, L, precision, False)
    err = ref.rel_l2(got, want)
    moved = ref.rel_l2(got, plain)
    print(f"{name}: loss {float(loss):.6f} (reference term {float(loss_ref):.6f}, eps {float(parts['eps']):.6f}, "
          f"stft {float(parts['stft']):.6f}); gradients rel L2 {err:.2e}; the term moves them by {moved:.2e}")
    assert torch.isfinite(got).all() and err <= FULL_TOL
    assert moved > 50 * FULL_TOL                    # the term is a visible part of the gradient
    assert set(parts) == {"eps", "stft"} and all(v.device.type == "cuda" and not v.requires_grad for v in parts.values())
    assert torch.equal(parts["eps"], base) and float(parts["stft"]) > 0
    assert abs(float(loss) - (float(parts["eps"]) + 0.5 * float(parts["stft"]))) <= 1e-6 * abs(float(loss))
    assert abs(float(parts["stft"]) - float(parts_ref["stft"])) <= 1e-5 * float(parts_ref["stft"])


def test_training_loss_without_the_term_and_with_an_empty_mask(gpu):
    cfg, B, L = cases.WAVENET_CASES["wn_c64"][0], 3, 2048
    a, base, _ = _training_grads(gpu, cfg, B, L, "f32", False)
    b, base2, parts = _training_grads(gpu, cfg, B, L, "f32", False, stft_weight=None)
    assert torch.equal(a, b) and torch.equal(base, base2) and parts == {}
    c, masked, parts = _training_grads(gpu, cfg, B, L, "f32", False, stft_weight=0.5, stft_max_step=0, stft_resolutions=SMALL)
    assert torch.equal(masked, base) and float(parts["stft"]) == 0.0 and torch.equal(parts["eps"], base)
    assert torch.isfinite(c).all()
    # a mask that lets every step through is the call without one
    d, full, _ = _training_grads(gpu, cfg, B, L, "f32", False, stft_weight=0.5, stft_max_step=50, stft_resolutions=SMALL)
    e, nomask, _ = _training_grads(gpu, cfg, B, L, "f32", False, stft_weight=0.5, stft_resolutions=SMALL)
    assert torch.equal(full, nomask) and torch.equal(d, e) and float(full) > float(base)

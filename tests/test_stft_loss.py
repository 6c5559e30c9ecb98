"""CPU: the spectral training loss (``metrics.mr_stft_loss``, ``training_loss(stft_weight=)``, the ``train.stft_*``
keys): every argument error in its order, and the float64 reference of the GPU tests against the hand-written float64
adjoint of the kernel's formula (include/dws.h, ``dws_spectral_loss_backward``)."""
import pytest
import torch

from diffwave_sashimi_amd.metrics import mr_stft_loss
from tests import stft_loss_reference as ref
from tests.spectral_reference import KINDS, RESOLUTIONS, signal_pair

CUSTOM = ((64, 16, 48), (128, 200, 128))            # hop > n_fft in the second: samples no frame covers
# float64 against float64: two evaluation orders of the same sums (an FFT and a matrix product; autograd's and the
# formula's).  Unit roundoff 1.1e-16 over 2048-term sums, amplified at the weak bins of the log-magnitude term by up to
# max|X| / sqrt(floor) ~ 1e5: 1e-8 leaves two decades (measured: 3e-10 at the worst signal).
F64_TOL = 1e-8


# ------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("length", (1025, 1300, 2500))
@pytest.mark.parametrize("weights", ((1.0, 1.0), (1.0, 0.0), (0.0, 2.0)))
def test_reference_autograd_equals_the_handwritten_adjoint(kind, length, weights):
    x, y = signal_pair(kind, length)
    auto = ref.gradient(x, y, RESOLUTIONS, *weights)
    hand = ref.adjoint_gradient(x, y, RESOLUTIONS, *weights)
    assert torch.isfinite(auto).all() and torch.isfinite(hand).all()
    if kind == "xsilent":                           # every bin of X below the floor: no gradient at all
        assert not auto.any() and not hand.any()
        return
    err = ref.rel_l2(hand, auto)
    print(f"{kind} {length} {weights}: adjoint vs autograd rel L2 {err:.2e}")
    assert err <= F64_TOL


def test_reference_adjoint_on_uncovered_samples_and_an_exact_match():
    x, y = signal_pair("noise", 1300)
    auto = ref.gradient(x, y, CUSTOM)
    hand = ref.adjoint_gradient(x, y, CUSTOM)
    assert ref.rel_l2(hand, auto) <= F64_TOL
    # with (128, 200, 128) alone, frame f covers samples 200 f - 64 .. 200 f + 63: the others get exactly 0
    only = ref.adjoint_gradient(x, y, CUSTOM[1:])
    covered = torch.zeros(1300, dtype=torch.bool)
    for f in range(1300 // 200 + 1):
        covered[max(0, 200 * f - 64):200 * f + 64] = True
    assert not only[~covered].any() and only[covered].abs().max() > 0
    assert torch.equal(ref.gradient(x, y, CUSTOM[1:])[~covered], only[~covered])
    # x == y: autograd through sqrt(0 / den) is NaN; the reference (and the kernel) give exactly 0
    same = ref.gradient(y, y)
    assert torch.isfinite(same).all() and not same.any()
    assert not ref.adjoint_gradient(y, y).any()
    assert float(ref.clip_loss(y, y)) == 0.0


# ---------------------------------------------------------------------------------------------------- mr_stft_loss
def test_mr_stft_loss_argument_errors_in_their_order():
    x, y = (t[None] for t in signal_pair("noise", 1300))
    with pytest.raises(ValueError, match="expected a float tensor"):
        mr_stft_loss(x[0], y)
    with pytest.raises(ValueError, match="two equal non-empty batches"):
        mr_stft_loss(x, y[:, :-1])
    with pytest.raises(ValueError, match="lengths"):
        mr_stft_loss(x, y, [1301])
    with pytest.raises(ValueError, match="clip 0 has 1000 samples"):            # n_fft = 2048 needs 1025
        mr_stft_loss(x, y, [1000])
    with pytest.raises(ValueError, match="n_fft must be a power of two"):
        mr_stft_loss(x, y, resolutions=((2048, 240, 1200), (4096, 240, 1200)))
    for bad in ((), ((512, 50),), 7, ((500, 50, 240),), ((512, 0, 240),), ((512, 50, 600),)):
        with pytest.raises(ValueError):
            mr_stft_loss(x, y, resolutions=bad)
    for kw in (dict(sc_weight=-1.0), dict(mag_weight=float("nan")), dict(sc_weight=float("inf")),
               dict(sc_weight=0.0, mag_weight=0), dict(mag_weight="1"), dict(sc_weight=True)):
        with pytest.raises(ValueError, match="weight"):
            mr_stft_loss(x, y, **kw)
    with pytest.raises(ValueError, match="y requires grad"):
        mr_stft_loss(x, y.clone().requires_grad_(True))
    # every argument in order: the device is what is left (a ValueError wins over it, see above: all of those were CPU)
    with pytest.raises(RuntimeError, match="GPU only"):
        mr_stft_loss(x, y)
    with pytest.raises(RuntimeError, match="GPU only"):
        mr_stft_loss(x.clone().requires_grad_(True), y, sc_weight=0.0)


# --------------------------------------------------------------------------------------------------- training_loss
class _StandIn(torch.nn.Module):
    """A differentiable network of the reference surface: eps = conv(x) + t / 100."""

    def __init__(self, channels=1):
        super().__init__()
        torch.manual_seed(3)
        self.conv = torch.nn.Conv1d(channels, channels, 5, padding=2)
        self.calls = 0

    def forward(self, inp, mel_spec=None, labels=None):
        x, t = inp
        self.calls += 1
        return self.conv(x) + t.reshape(-1, 1, 1) / 100.0


def test_training_loss_argument_errors_and_an_unchanged_plain_call():
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    mse = torch.nn.MSELoss()
    audio = torch.rand(2, 1, 600, generator=torch.Generator().manual_seed(5)) * 0.6 - 0.3
    net = _StandIn()
    small = ((256, 64, 128), (128, 32, 64))
    gen = torch.Generator().manual_seed(9)
    state = gen.get_state()
    bad = [dict(stft_weight=0.0), dict(stft_weight=-0.5), dict(stft_weight=float("nan")), dict(stft_weight="0.5"),
           dict(stft_weight=True), dict(stft_max_step=10), dict(stft_resolutions=small),
           dict(stft_weight=0.5, stft_max_step=-1), dict(stft_weight=0.5, stft_max_step=51),
           dict(stft_weight=0.5, stft_max_step=2.5), dict(stft_weight=0.5, stft_resolutions=((100, 10, 50),)),
           dict(stft_weight=0.5, stft_resolutions=())]
    for kw in bad:
        with pytest.raises(ValueError, match="stft_|resolution"):
            training_loss(net, mse, audio, dh, generator=gen, **kw)
    with pytest.raises(ValueError, match="clip 0 has 600 samples"):          # the default n_fft = 2048 needs 1025
        training_loss(net, mse, audio, dh, generator=gen, stft_weight=0.5)
    with pytest.raises(ValueError, match="one audio channel"):
        training_loss(_StandIn(2), mse, audio.expand(2, 2, 600), dh, generator=gen, stft_weight=0.5, stft_resolutions=small)
    with pytest.raises(ValueError, match="parts"):
        training_loss(net, mse, audio, dh, generator=gen, stft_weight=0.5, stft_resolutions=small, parts=[])
    assert net.calls == 0 and torch.equal(gen.get_state(), state)        # nothing was drawn, nothing ran
    # good arguments on the CPU: the value errors are through, the device error is what is left (there is no CPU path)
    with pytest.raises(RuntimeError, match="GPU only"):
        training_loss(net, mse, audio, dh, generator=gen, stft_weight=0.5, stft_resolutions=small, stft_max_step=50)
    # without stft_weight: the call of before, bit for bit, with the draws of before
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    a = training_loss(net, mse, audio, dh, generator=g1)
    b = training_loss(net, mse, audio, dh, generator=g2, stft_weight=None, stft_max_step=None, stft_resolutions=None,
                      parts=None)
    steps = torch.randint(50, size=(2, 1, 1), generator=torch.Generator().manual_seed(9))
    assert torch.equal(a, b) and torch.equal(g1.get_state(), g2.get_state())
    g3 = torch.Generator().manual_seed(9)
    torch.randint(50, size=(2, 1, 1), generator=g3)
    torch.normal(0, 1, size=audio.shape, generator=g3)
    assert torch.equal(g1.get_state(), g3.get_state()) and steps.shape == (2, 1, 1)


# ------------------------------------------------------------------------------------------------------- train keys
def test_stft_loss_options_and_the_train_keys():
    from diffwave_sashimi_amd.metrics import MR_STFT_RESOLUTIONS
    from diffwave_sashimi_amd.train import train
    from diffwave_sashimi_amd.training import stft_loss_options
    assert stft_loss_options() is None
    assert stft_loss_options(0.1, T=200) == dict(weight=0.1, max_step=None,
                                                 resolutions=[list(r) for r in MR_STFT_RESOLUTIONS])
    assert stft_loss_options(2, 40, [[256, 64, 128]], T=50) == dict(weight=2.0, max_step=40, resolutions=[[256, 64, 128]])

    class NeverBuilt(dict):        # a model config that fails the test if anything reads past the checked key
        def __getitem__(self, k):
            raise AssertionError(f"train read model.{k} before it had checked the stft keys")

    tr = dict(diffusion_cfg=dict(T=50, beta_0=1e-4, beta_T=0.05), dataset_cfg={}, generate_cfg={}, ckpt_iter=-1, n_iters=1,
              iters_per_ckpt=1, iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=2)
    for kw in (dict(stft_weight=0), dict(stft_weight=-1.0), dict(stft_weight="x"), dict(stft_max_step=3),
               dict(stft_resolutions=[[256, 64, 128]]), dict(stft_weight=0.1, stft_max_step=51),
               dict(stft_weight=0.1, stft_max_step=-2), dict(stft_weight=0.1, stft_resolutions=[[256, 64]]),
               dict(stft_weight=0.1, stft_resolutions=[[300, 64, 128]]), dict(stft_weight=0.1, stft_resolutions="all")):
        with pytest.raises(ValueError, match="train|resolution"):
            train(0, 1, model_cfg=NeverBuilt(in_channels=1), **tr, **kw)
    with pytest.raises(ValueError, match="in_channels"):
        train(0, 1, model_cfg=NeverBuilt(in_channels=2), **tr, stft_weight=0.1)

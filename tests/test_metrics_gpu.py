"""GPU: ``metrics.spectral_metrics`` / ``spectral_sums`` (``dws_spectral_distance``) against the float64 reference of
tests/spectral_reference.py, and the properties the kernel states: a clip's sums depend on its own samples alone (bit for
bit: batch size, place, padded length and the content of the padding do not enter), two calls give the same bits, digital
silence gives exact zeros, and no length is clamped.

Tolerance (spectral_reference.RTOL / ATOL / ATOL_MCD): relative 1e-5 plus absolute 1e-6 (1e-5 dB for mcd): about a
hundred float32 roundings, where a metric is a mean over 10^4 .. 10^6 terms whose single errors are a few roundings of
random sign.  As a check of the bound itself, all-float32 evaluations of exactly these inputs on a CPU -- the FFT form
and the direct DFT as a float32 matmul, logarithms and cepstra in float32 too -- use at most 0.43 of it (the widest: mcd
of nearly equal signals, 4e-6 dB off); the kernel, with its band logarithms in double, at most 0.37."""
import pytest
import torch

from tests import spectral_reference as ref

pytestmark = pytest.mark.gpu

_REFERENCE = {}


def _reference(kind, length):
    """The float64 metrics of one (kind, length): computed once, shared, never changed."""
    if (kind, length) not in _REFERENCE:
        _REFERENCE[kind, length] = ref.metrics(*ref.signal_pair(kind, length))
    return dict(_REFERENCE[kind, length])


def _passes():
    """The four launches of a ``spectral_metrics`` call as ``spectral_sums`` keywords."""
    out = [dict(n_fft=r[0], hop=r[1], win=r[2]) for r in ref.RESOLUTIONS]
    n_fft, hop, win = ref.MEL_RESOLUTION
    return out + [dict(n_fft=n_fft, hop=hop, win=win, mel_basis=ref.default_basis(), n_cep=13)]


@pytest.mark.parametrize("length", ref.LENGTHS)
@pytest.mark.parametrize("kind", ref.KINDS)
def test_every_metric_matches_float64(gpu, kind, length):
    from diffwave_sashimi_amd.metrics import spectral_metrics
    x, y = ref.signal_pair(kind, length)
    got = spectral_metrics(x[None].to(gpu), y[None, None].to(gpu))         # [B, T] and [B, 1, T] are both taken
    want = _reference(kind, length)
    assert sorted(got) == sorted(want) and len(want) == 2 * len(ref.RESOLUTIONS) + 4
    bad = []
    for key in sorted(want):
        assert got[key].dtype == torch.float64 and got[key].device.type == "cpu" and tuple(got[key].shape) == (1,)
        err = abs(float(got[key]) - want[key])
        print(f"{kind} {length} {key}: got {float(got[key]):.9g} want {want[key]:.9g} |diff| {err:.3g}")
        if not ref.close(got[key], want[key], key):
            bad.append((key, float(got[key]), want[key]))
    assert not bad, bad


def test_ragged_batch_rows_are_each_clips_own_bits(gpu):
    """Four lengths in one [4, 4000] batch with NaN in every padded position of both inputs: each clip's six sums equal, bit
    for bit, its own B = 1, T = len call and the same batch in reverse order."""
    from diffwave_sashimi_amd.metrics import spectral_sums
    pairs = [ref.signal_pair("noise", n) for n in ref.LENGTHS]
    T = max(ref.LENGTHS)
    x = torch.full((len(pairs), T), float("nan"))
    y = torch.full((len(pairs), T), float("nan"))
    for b, (xb, yb) in enumerate(pairs):
        x[b, :xb.shape[0]], y[b, :yb.shape[0]] = xb, yb
    lens = list(ref.LENGTHS)
    for kw in _passes():
        batch = spectral_sums(x.to(gpu), y.to(gpu), lens, **kw)
        assert batch.dtype == torch.float64 and tuple(batch.shape) == (4, 6) and torch.isfinite(batch).all()
        back = spectral_sums(x.flip(0).to(gpu), y.flip(0).to(gpu), lens[::-1], **kw)
        assert torch.equal(back.flip(0), batch), kw
        for b, (xb, yb) in enumerate(pairs):
            alone = spectral_sums(xb[None].to(gpu), yb[None].to(gpu), **kw)
            assert torch.equal(alone[0], batch[b]), (kw["n_fft"], lens[b], alone[0], batch[b])
        assert (batch[:, :4] > 0).all() and ((batch[:, 4:] > 0).all() if "mel_basis" in kw else (batch[:, 4:] == 0).all())


def test_two_calls_give_the_same_bits(gpu):
    from diffwave_sashimi_amd.metrics import spectral_metrics
    x, y = ref.signal_pair("noise", 4000)
    x, y = x[None].repeat(3, 1).to(gpu), y[None].repeat(3, 1).to(gpu)
    a, b = spectral_metrics(x, y), spectral_metrics(x, y)
    for key in a:
        assert torch.equal(a[key], b[key]), key
        assert torch.equal(a[key], a[key][:1].expand(3)), key              # and equal clips equal numbers


def test_digital_silence_is_exactly_zero(gpu):
    from diffwave_sashimi_amd.metrics import spectral_metrics
    z = torch.zeros(2, 2500, device=gpu)
    for key, v in spectral_metrics(z, z, [2500, 1300]).items():
        assert torch.equal(v, torch.zeros(2, dtype=torch.float64)), key


def test_a_clip_one_sample_too_short_is_refused_not_clamped(gpu):
    from diffwave_sashimi_amd.metrics import spectral_metrics, spectral_sums
    x = torch.zeros(2, 4000, device=gpu)
    with pytest.raises(ValueError, match=r"n_fft=2048.*clip 1 has 1024 samples"):
        spectral_metrics(x, x, [4000, 1024])
    with pytest.raises(ValueError, match=r"n_fft=512.*clip 0 has 256 samples"):
        spectral_sums(x[:, :256], x[:, :256], n_fft=512, hop=50, win=240)
    assert torch.isfinite(spectral_sums(x[:, :257], x[:, :257], n_fft=512, hop=50, win=240)).all()

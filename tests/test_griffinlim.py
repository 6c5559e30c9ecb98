"""CPU: the float64 restatement of the inversion kernels (tests/griffinlim_reference.py) against torch's own transforms
and against the reference's recorded results, and the pseudo-inverse table of ``mel_to_magnitude``."""
import numpy as np
import pytest
import torch

from tests import griffinlim_reference as glr
from tests.conftest import load_golden

# (n_fft, hop, win)
RESOLUTIONS = [(64, 16, 64), (1024, 256, 1024), (1024, 256, 800), (64, 32, 64)]


def _torch_window(win):
    return torch.hann_window(win, periodic=True, dtype=torch.float64)


@pytest.mark.parametrize("n_fft,hop,win", RESOLUTIONS)
def test_stft64_is_torch_stft(n_fft, hop, win):
    x = glr.test_signal(2, 8 * max(hop, n_fft // 8))
    want = torch.stft(torch.from_numpy(x.copy()), n_fft, hop_length=hop, win_length=win, window=_torch_window(win),
                      center=True, pad_mode="reflect", return_complex=True).numpy()
    # on torch's float64 window (the engine's table is its float32 rounding)
    got = glr.stft64(x, np.pad(_torch_window(win).numpy(), ((n_fft - win) // 2,) * 2), hop)
    assert got.shape == want.shape
    assert glr.rel_l2(got, want) < 1e-12


@pytest.mark.parametrize("n_fft,hop,win", RESOLUTIONS)
def test_istft64_is_torch_istft(n_fft, hop, win):
    x = glr.test_signal(2, 8 * max(hop, n_fft // 8))
    w = np.pad(_torch_window(win).numpy(), ((n_fft - win) // 2,) * 2)
    spec = glr.stft64(x, w, hop)
    want = torch.istft(torch.from_numpy(spec), n_fft, hop_length=hop, win_length=win, window=_torch_window(win),
                       center=True).numpy()
    got = glr.istft64(spec, w, hop)
    assert got.shape == want.shape == x.shape
    assert glr.rel_l2(got, want) < 1e-12
    assert glr.rel_l2(got, x) < 1e-12          # and the pair is a perfect reconstruction


@pytest.mark.parametrize("name,n_fft,hop", [("n64", 64, 16), ("n1024", 1024, 256)])
def test_restatement_reproduces_the_reference(name, n_fft, hop):
    """``STFT.inverse`` and ``griffin_lim(n_iters=4)`` of the reference's ``dataloaders/stft.py`` (float32, recorded by
    tests/golden/make_golden_griffinlim.py) against ``istft64`` / ``griffin_lim64`` on the recorded magnitudes and angles.
    The tolerance is the float32 reference's distance from float64.  Measured relative l2 differences: inverse 1.9e-7
    (64/16) and 3.6e-7 (1024/256); griffin_lim at 4 iterations 3.5e-7 (64/16) and 1.0e-4 (1024/256) -- the last is one
    round's rounding of a nearly silent bin whose phase the next projection keeps: the same run is 1.0e-6, 9.9e-7, 3.8e-6
    at 1, 2, 3 iterations and 1.2e-5 at 8.  Largest 1.0e-4, times 8, rounded up to one digit: 8e-4."""
    d = load_golden("griffinlim")
    mag, ang = d[name + "_magnitude"], d[name + "_angles"]
    w = glr.hann_window(n_fft, n_fft)
    inv = glr.rel_l2(glr.istft64(mag * np.exp(1j * ang.astype(np.float64)), w, hop), d[name + "_inverse"])
    gl = glr.rel_l2(glr.griffin_lim64(mag, ang, w, hop, 4), d[name + "_griffin_lim4"])
    print(f"{name}: inverse {inv:.2e}, griffin_lim4 {gl:.2e}")
    assert inv < 8e-4 and gl < 8e-4


def test_momentum_zero_is_the_plain_loop_and_momentum_changes_it():
    n_fft, hop = 64, 16
    w = glr.hann_window(n_fft, n_fft)
    mag = np.abs(glr.stft64(glr.test_signal(1, 20 * hop), w, hop))
    ph = glr.phases(*mag.shape)
    a = glr.griffin_lim64(mag, ph, w, hop, 3, 0.0)
    x = glr.istft64(mag * np.exp(1j * ph), w, hop)
    for _ in range(3):
        x = glr.istft64(glr.project64(x, mag, w, hop), w, hop)
    assert np.array_equal(a, x)
    assert glr.rel_l2(glr.griffin_lim64(mag, ph, w, hop, 3, 0.99), a) > 1e-3


def test_mel_pinv_table():
    """``P = pinv(basis)`` in float64: ``P basis P == P`` to 1e-10, and magnitudes in the filterbank's row space come back
    from their mel."""
    from diffwave_sashimi_amd.mel import TacotronSTFT
    stft = TacotronSTFT()
    P = stft.mel_pinv()
    basis = stft.mel_basis.numpy().astype(np.float64)
    assert P.dtype == np.float64 and P.shape == (stft.filter_length // 2 + 1, stft.n_mel_channels)
    assert np.abs(P @ basis @ P - P).max() < 1e-10 * np.abs(P).max()
    rng = np.random.RandomState(3)
    mag = basis.T @ rng.rand(stft.n_mel_channels, 7)              # [K, 7] in the row space
    back = P @ (basis @ mag)
    assert np.abs(back - mag).max() < 1e-10 * np.abs(mag).max()
    assert stft.mel_pinv() is P                                    # computed once


def test_argument_errors_need_no_gpu():
    """The refusals that come before anything runs: CPU tensors, ranks, requires_grad, iteration count and momentum."""
    from diffwave_sashimi_amd import mel
    stft = mel.TacotronSTFT(filter_length=64, hop_length=16, win_length=64)
    m = torch.ones(1, 33, 8)
    w = stft.window
    with pytest.raises(ValueError, match="magnitude.*GPU only"):
        mel.istft(m, m, window=w, hop_length=16)
    with pytest.raises(ValueError, match="magnitude.*GPU only"):
        mel.griffin_lim(m, window=w, hop_length=16)
    with pytest.raises(ValueError, match="magnitude has shape"):
        mel.griffin_lim(torch.ones(33, 8), window=w, hop_length=16)
    with pytest.raises(ValueError, match="n_iters"):
        mel.griffin_lim(m, window=w, hop_length=16, n_iters=4097)
    with pytest.raises(ValueError, match="momentum"):
        mel.griffin_lim(m, window=w, hop_length=16, momentum=1.0)
    with pytest.raises(ValueError, match="phase"):
        mel.griffin_lim(m, window=w, hop_length=16, phase="random")
    with pytest.raises(ValueError, match="GPU only"):
        stft.mel_to_audio(torch.zeros(1, 80, 8))
    with pytest.raises(ValueError, match="mel has shape"):
        stft.mel_to_magnitude(torch.zeros(1, 40, 8))
    with pytest.raises(ValueError, match="GPU only"):
        stft.inverse(m, m)

"""GPU: ``mel.istft`` / ``mel.griffin_lim`` (``dws_istft`` / ``dws_griffin_lim``, csrc/griffinlim_kernels.hip) against the
float64 restatement (tests/griffinlim_reference.py) on deterministic signals (a chirp plus a tone plus weak noise), B = 2.

Tolerance of the round trip and of the iteration parity: the relative l2 distance from ``istft64`` / ``griffin_lim64`` on
exactly these inputs, measured on an MI355X.
Round trip (n_fft / hop / win, frames): 64/16/64, 40: 1.38e-7; 1024/256/1024, 6: 5.13e-7; 1024/256/800, 6: 5.78e-7; 64/64/64,
10: 3.02e-6 (frames that do not overlap: a sample next to a window zero is a rounding error divided by a small w^2).
Iteration parity, one number per (n_fft, momentum, n) row:
    64/16, 40 frames      momentum 0:    n = 0: 1.80e-7   1: 2.57e-7   4: 4.43e-7   32: 2.75e-6
                          momentum 0.99: n = 0: 1.80e-7   1: 2.57e-7   4: 9.60e-7
    1024/256, 12 frames   momentum 0:    n = 0: 7.19e-7   1: 1.41e-6   4: 2.26e-5   32: 1.65e-5
                          momentum 0.99: n = 0: 7.19e-7   1: 1.41e-6   4: 6.01e-6
(the step from 1 to 4 iterations at 1024/256 is a nearly silent bin whose phase one rounding turns and the next
projection keeps; the float32 reference itself is 1.0e-4 from float64 at that point, tests/test_griffinlim.py).
The largest, 2.26e-5, times 8 and rounded up to one digit: 2e-4.

Convergence: ``|| |STFT(x_n)| - M || / || M ||`` of the GPU output, evaluated in float64 on the CPU, against the same
number of the float64 run.
Measured at n = 0, 4, 16, 32 (float64 value, relative difference of the GPU's):
    64/16     momentum 0:    0.643167 1.5e-8   0.292914 9.5e-9   0.209986 3.5e-7   0.176343 4.0e-7
              momentum 0.99: 0.643167 1.5e-8   0.257996 1.2e-8   0.146767 2.4e-6   0.095829 6.4e-7
    1024/256  momentum 0:    0.668933 3.0e-10  0.330971 3.8e-8   0.266056 4.4e-8   0.232087 3.8e-7
              momentum 0.99: 0.668933 3.0e-10  0.307578 2.2e-8   0.203757 3.6e-6   0.177341 5.6e-9
The largest relative difference, 3.56e-6, times 8 and rounded up to one digit: 3e-5.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import griffinlim_reference as glr

pytestmark = pytest.mark.gpu

TOL = 2e-4
SC_TOL = 3e-5
# rounding of the inputs where a result is compared with the signal the spectrum was taken from: the magnitudes are
# rounded to float32 (2^-24 relative) and the phases too (pi 2^-24 absolute, the same relative change of a bin)
INPUT_ROUNDING = 2.5e-7

ROUND_TRIP = [(64, 16, 64, 40), (1024, 256, 1024, 6), (1024, 256, 800, 6), (64, 64, 64, 10)]      # n_fft, hop, win, F
PARITY = [(64, 16, 40), (1024, 256, 12)]                                                            # n_fft, hop, F
PARITY_RUNS = [(0.0, 0), (0.0, 1), (0.0, 4), (0.0, 32), (0.99, 0), (0.99, 1), (0.99, 4)]            # momentum, n_iters
SC_ITERS = (0, 4, 16, 32)


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


@functools.lru_cache(maxsize=None)
def _target(n_fft, hop, F):
    """Target magnitudes |STFT| of the test signal and starting phases, as the float32 values both sides read."""
    w = glr.hann_window(n_fft, n_fft)
    mag = np.abs(glr.stft64(glr.test_signal(2, (F - 1) * hop), w, hop)).astype(np.float32)
    return w, mag, glr.phases(*mag.shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _want(n_fft, hop, F, momentum, n):
    w, mag, ph = _target(n_fft, hop, F)
    return glr.griffin_lim64(mag, ph, w, hop, n, momentum)


_got = {}


def _run(gpu, n_fft, hop, F, momentum, n):
    from diffwave_sashimi_amd import mel
    key = (n_fft, hop, F, momentum, n)
    if key not in _got:
        w, mag, ph = _target(n_fft, hop, F)
        _got[key] = mel.griffin_lim(_dev(mag, gpu), window=_dev(w, gpu), hop_length=hop, n_iters=n, momentum=momentum,
                                    phase=_dev(ph, gpu)).cpu().numpy()
    return _got[key]


@pytest.mark.parametrize("n_fft,hop,win,F", ROUND_TRIP)
def test_istft_round_trip(n_fft, hop, win, F, gpu):
    from diffwave_sashimi_amd import mel
    x = glr.test_signal(2, (F - 1) * hop)
    spec = torch.stft(torch.from_numpy(x.copy()), n_fft, hop_length=hop, win_length=win,
                      window=torch.hann_window(win, periodic=True, dtype=torch.float64), center=True, pad_mode="reflect",
                      return_complex=True)
    mag, ph = spec.abs().float(), spec.angle().float()
    w = glr.hann_window(win, n_fft)
    got = mel.istft(mag.to(gpu), ph.to(gpu), window=_dev(w, gpu), hop_length=hop)
    assert got.dtype == torch.float32 and tuple(got.shape) == x.shape
    got = got.cpu().numpy()
    want = glr.istft64(mag.double().numpy() * np.exp(1j * ph.double().numpy()), w, hop)
    err = glr.rel_l2(got, want)
    if hop < n_fft:
        back = glr.rel_l2(got, x)
        print(f"istft {n_fft}/{hop}/{win} F={F}: against istft64 {err:.3e}, against x {back:.3e}")
        assert back <= TOL + INPUT_ROUNDING
    else:
        # hop = n_fft: frames do not overlap and the window's zero leaves wss = 0 at p = f hop: the undivided value, 0
        zero = np.arange(x.shape[1]) % hop == hop - n_fft // 2
        print(f"istft {n_fft}/{hop}/{win} F={F}: against istft64 {err:.3e}, {int(zero.sum())} positions with wss = 0")
        assert zero.sum() == F - 1 and np.all(want[:, zero] == 0.0) and np.all(got[:, zero] == 0.0)
        assert glr.rel_l2(got[:, ~zero], x[:, ~zero]) <= TOL + INPUT_ROUNDING
    assert err <= TOL
    assert np.isfinite(got).all()


@pytest.mark.parametrize("momentum,n", PARITY_RUNS)
@pytest.mark.parametrize("n_fft,hop,F", PARITY)
def test_iteration_parity(n_fft, hop, F, momentum, n, gpu):
    got, want = _run(gpu, n_fft, hop, F, momentum, n), _want(n_fft, hop, F, momentum, n)
    err = glr.rel_l2(got, want)
    print(f"griffin_lim {n_fft}/{hop} F={F} momentum={momentum} n={n}: rel l2 {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("n_fft,hop,F", PARITY)
def test_converges_as_float64_does(n_fft, hop, F, gpu):
    w, mag, _ = _target(n_fft, hop, F)
    for momentum in (0.0, 0.99):
        sc = [glr.spectral_convergence(_run(gpu, n_fft, hop, F, momentum, n), mag, w, hop) for n in SC_ITERS]
        sc64 = [glr.spectral_convergence(_want(n_fft, hop, F, momentum, n), mag, w, hop) for n in SC_ITERS]
        rel = [abs(a - b) / b for a, b in zip(sc, sc64)]
        print(f"convergence {n_fft}/{hop} momentum={momentum}: gpu " + " ".join(f"{v:.6f}" for v in sc) + "  float64 " +
              " ".join(f"{v:.6f}" for v in sc64) + "  relative difference " + " ".join(f"{v:.2e}" for v in rel))
        if momentum == 0.0:
            assert all(a > b for a, b in zip(sc, sc[1:])), sc              # Griffin & Lim's theorem
        assert max(rel) <= SC_TOL, (momentum, rel)


def test_zero_phase_and_zero_magnitude(gpu):
    from diffwave_sashimi_amd import mel
    n_fft, hop, F = 64, 16, 40
    w, mag, _ = _target(n_fft, hop, F)
    wd, md = _dev(w, gpu), _dev(mag, gpu)
    for n, momentum in ((0, 0.0), (3, 0.0), (3, 0.99)):
        a = mel.griffin_lim(md, window=wd, hop_length=hop, n_iters=n, momentum=momentum, phase="zero")
        b = mel.griffin_lim(md, window=wd, hop_length=hop, n_iters=n, momentum=momentum, phase=torch.zeros_like(md))
        assert torch.equal(a, b) and float(a.abs().max()) > 0
        z = mel.griffin_lim(torch.zeros_like(md), window=wd, hop_length=hop, n_iters=n, momentum=momentum, seed=5)
        assert torch.equal(z, torch.zeros_like(z))
    assert torch.equal(mel.istft(torch.zeros_like(md), md, window=wd, hop_length=hop), torch.zeros(2, (F - 1) * hop, device=gpu))


@pytest.mark.parametrize("n_fft,hop,F", PARITY)
def test_ragged_batch(n_fft, hop, F, gpu):
    from diffwave_sashimi_amd import mel
    w, mag, ph = _target(n_fft, hop, F)
    T = (F - 1) * hop
    short = T - 3 * hop
    mag = mag.copy()
    mag[1, :, F - 3:] = np.nan                       # the short clip's unused frames
    wd = _dev(w, gpu)
    for n, momentum in ((0, 0.0), (4, 0.0), (4, 0.99)):
        both = mel.griffin_lim(_dev(mag, gpu), window=wd, hop_length=hop, n_iters=n, momentum=momentum, phase=_dev(ph, gpu),
                               lengths=[T, short])
        alone = mel.griffin_lim(_dev(mag[1:, :, :F - 3], gpu), window=wd, hop_length=hop, n_iters=n, momentum=momentum,
                                phase=_dev(ph[1:, :, :F - 3], gpu))
        assert tuple(both.shape) == (2, T) and tuple(alone.shape) == (1, short)
        assert torch.equal(both[1, :short], alone[0])
        assert torch.equal(both[1, short:], torch.zeros(T - short, device=gpu))
        assert bool(torch.isfinite(both).all())
        assert np.array_equal(both[0].cpu().numpy(), _run(gpu, n_fft, hop, F, momentum, n)[0])      # row 0: the full batch's
    both = mel.istft(_dev(mag, gpu), _dev(ph, gpu), window=wd, hop_length=hop, lengths=torch.tensor([T, short]))
    assert bool(torch.isfinite(both).all()) and float(both[1, short:].abs().max()) == 0.0


def test_reproducible_and_zero_iterations_is_istft(gpu):
    from diffwave_sashimi_amd import mel
    n_fft, hop, F = 1024, 256, 12
    w, mag, ph = _target(n_fft, hop, F)
    wd, md, pd = _dev(w, gpu), _dev(mag, gpu), _dev(ph, gpu)
    a = mel.griffin_lim(md, window=wd, hop_length=hop, n_iters=5, momentum=0.99, seed=3)
    b = mel.griffin_lim(md, window=wd, hop_length=hop, n_iters=5, momentum=0.99, seed=3)
    c = mel.griffin_lim(md, window=wd, hop_length=hop, n_iters=5, momentum=0.99, seed=4)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(mel.griffin_lim(md, window=wd, hop_length=hop, n_iters=0, phase=pd),
                       mel.istft(md, pd, window=wd, hop_length=hop))
    stft = mel.TacotronSTFT(filter_length=n_fft, hop_length=hop, win_length=n_fft)
    assert torch.equal(stft.inverse(md, pd), mel.istft(md, pd, window=wd, hop_length=hop))
    assert torch.equal(stft.griffin_lim(md, n_iters=5, momentum=0.99, seed=3), a)


def test_python_refusals(gpu):
    from diffwave_sashimi_amd import mel
    n_fft, hop, F = 64, 16, 40
    w, mag, ph = _target(n_fft, hop, F)
    wd, md, pd = _dev(w, gpu), _dev(mag, gpu), _dev(ph, gpu)
    T = (F - 1) * hop
    kw = dict(window=wd, hop_length=hop)
    with pytest.raises(ValueError, match="phase.*GPU only"):
        mel.istft(md, pd.cpu(), **kw)
    with pytest.raises(ValueError, match="window"):
        mel.istft(md, pd, window=wd.cpu(), hop_length=hop)
    with pytest.raises(ValueError, match="magnitude has shape"):
        mel.istft(md[0], pd[0], **kw)
    with pytest.raises(ValueError, match="phase has shape"):
        mel.istft(md, pd[:, :, :-1], **kw)
    with pytest.raises(ValueError, match="K = n_fft/2 \\+ 1"):
        mel.griffin_lim(md[:, :-1], **kw)
    with pytest.raises(ValueError, match="magnitude.*float32"):
        mel.griffin_lim(md.double(), **kw)
    with pytest.raises(ValueError, match="magnitude requires grad"):
        mel.griffin_lim(md.clone().requires_grad_(), **kw)
    with pytest.raises(ValueError, match="phase requires grad"):
        mel.istft(md, pd.clone().requires_grad_(), **kw)
    with pytest.raises(ValueError, match="lengths: clip 1 has .* not a multiple of hop_length"):
        mel.griffin_lim(md, lengths=[T, T - 8], **kw)
    with pytest.raises(ValueError, match="lengths: clip 0 has 32 samples"):
        mel.istft(md, pd, lengths=[32, T], **kw)
    with pytest.raises(ValueError, match="lengths has 1 entries"):
        mel.istft(md, pd, lengths=[T], **kw)
    with pytest.raises(ValueError, match="hop_length"):
        mel.istft(md, pd, window=wd, hop_length=0)
    with pytest.raises(ValueError, match="power of two"):
        mel.istft(md, pd, window=wd[:48], hop_length=hop)
    with pytest.raises(ValueError, match="n_iters"):
        mel.griffin_lim(md, n_iters=-1, **kw)
    with pytest.raises(ValueError, match="momentum"):
        mel.griffin_lim(md, momentum=-0.1, **kw)
    with pytest.raises(ValueError, match="seed"):
        mel.griffin_lim(md, seed=-1, **kw)
    stft = mel.TacotronSTFT()
    with pytest.raises(ValueError, match="requires grad"):
        stft.mel_to_audio(torch.zeros(1, 80, 8, device=gpu).requires_grad_())
    with pytest.raises(ValueError, match="mel has shape"):
        stft.mel_to_audio(torch.zeros(80, 8, device=gpu))


def test_abi_refusals(gpu):
    from diffwave_sashimi_amd import _lib
    lib = _lib.load()
    n_fft, hop, F = 64, 16, 40
    w, mag, ph = _target(n_fft, hop, F)
    wd, md = _dev(w, gpu), _dev(mag, gpu)
    T = (F - 1) * hop
    out = torch.empty(2, T, device=gpu)
    ws = torch.empty(lib.dws_griffin_lim_workspace(2, F, n_fft, hop, 1) // 4, device=gpu)
    assert lib.dws_griffin_lim_workspace(2, F, n_fft, hop, 0) == 2 * F * n_fft * 4
    assert lib.dws_griffin_lim_workspace(2, F, n_fft, hop, 1) == (2 * F * n_fft + 2 * T) * 4
    for bad in ((0, F, n_fft, hop), (2, 1, n_fft, hop), (2, F, 48, hop), (2, F, 8192, hop), (2, F, n_fft, 0)):
        assert lib.dws_griffin_lim_workspace(*bad, 0) == 0
    dev_len = torch.tensor([T, T - 8], dtype=torch.int32, device=gpu)

    def gl(mag_ptr=md.data_ptr(), lengths=0, host=None, n_fft=n_fft, n_iters=1, momentum=0.0, F=F):
        return lib.dws_griffin_lim(mag_ptr, 0, 2, F, lengths, host, wd.data_ptr(), n_fft, hop, n_iters, momentum,
                                   out.data_ptr(), ws.data_ptr(), _lib.current_stream())

    def message():
        return lib.dws_last_error().decode()

    assert gl(n_iters=4097) == _lib.DWS_ERR_INVALID and "n_iters = 4097" in message()
    assert gl(n_iters=-1) == _lib.DWS_ERR_INVALID and "n_iters" in message()
    assert gl(momentum=1.0) == _lib.DWS_ERR_INVALID and "momentum = 1" in message()
    assert gl(momentum=float("nan")) == _lib.DWS_ERR_INVALID and "momentum" in message()
    assert gl(mag_ptr=0) == _lib.DWS_ERR_INVALID and "magnitude" in message()
    assert gl(lengths=dev_len.data_ptr(), host=(ctypes.c_int32 * 2)(T, T - 8)) == _lib.DWS_ERR_INVALID
    assert "lengths: clip 1 has %d samples, not a multiple of hop" % (T - 8) in message()
    assert gl(lengths=dev_len.data_ptr(), host=(ctypes.c_int32 * 2)(32, T)) == _lib.DWS_ERR_INVALID and "clip 0 has 32" in message()
    assert gl(lengths=dev_len.data_ptr(), host=(ctypes.c_int32 * 2)(T, T + hop)) == _lib.DWS_ERR_INVALID and "clip 1" in message()
    assert gl(lengths=dev_len.data_ptr()) == _lib.DWS_ERR_INVALID and "lengths_host" in message()
    assert gl(F=1) == _lib.DWS_ERR_INVALID and "f_max = 1" in message()
    assert gl(n_fft=48) == _lib.DWS_ERR_UNSUPPORTED and "n_fft = 48" in message()
    assert gl(n_fft=8192) == _lib.DWS_ERR_UNSUPPORTED and "n_fft = 8192" in message()
    rc = lib.dws_istft(md.data_ptr(), 0, 2, F, 0, None, wd.data_ptr(), n_fft, 0, out.data_ptr(), ws.data_ptr(),
                       _lib.current_stream())
    assert rc == _lib.DWS_ERR_INVALID and "dws_istft: hop = 0" in message()
    rc = lib.dws_istft(md.data_ptr(), 0, 2, F, 0, None, wd.data_ptr(), n_fft, hop, out.data_ptr(), 0, _lib.current_stream())
    assert rc == _lib.DWS_ERR_INVALID and "workspace" in message()


def test_mel_to_audio_moves_towards_the_mel(gpu):
    """A direction check, not a quality claim: the engine's own log-mel of the inversion of a speech-like signal's mel is
    closer to that mel after 32 iterations than after none."""
    from diffwave_sashimi_amd import mel
    from tests import stoi_reference
    stft = mel.TacotronSTFT()
    T = 86 * stft.hop_length                              # about 1 s at 22050 Hz
    y = _dev(stoi_reference.speech_like(T, 22050, 7)[None], gpu)
    m = stft.mel_spectrogram(y)
    dist = []
    for n in (0, 32):
        a = stft.mel_to_audio(m, n_iters=n)
        assert tuple(a.shape) == (1, T) and bool(torch.isfinite(a).all())
        dist.append(float((stft.differentiable_mel(a) - m).abs().mean()))
    print(f"mel_to_audio: mean |delta log-mel| {dist[0]:.4f} at 0 iterations, {dist[1]:.4f} at 32")
    assert dist[1] < dist[0]
    assert torch.equal(stft.mel_to_audio(m, n_iters=4, seed=1), stft.mel_to_audio(m, n_iters=4, seed=1))
    mag = stft.mel_to_magnitude(m)
    assert tuple(mag.shape) == (1, 513, 87) and float(mag.min()) >= 0.0

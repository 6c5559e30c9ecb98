"""GPU: `dws_mel_spectrogram_backward` (csrc/mel_kernels.hip), the adjoint of the mel front-end, against autograd through
the float64 restatement of its formulas (tests/mel_reference.py), and the autograd surface on top of it
(`TacotronSTFT.mel_spectrogram` on a tensor that requires grad, `sampling.mel_operator`).

Bound: the project's REL_TOL (1e-3 of max|reference|).  Float32 autograd through the CPU oracle sits at 3e-7 .. 2.5e-5 of
the float64 helper on these shapes (tests/test_mel_operator.py), so the bound is held by the kernel's arithmetic and
broken by any indexing mistake (a missed reflection changes the edge samples by O(1) of the maximum)."""
import ctypes

import pytest
import torch

from tests import cases
from tests import mel_reference as mref
from tests.conftest import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

IDS = lambda c: "n%d_h%d_w%d_T%d" % c[:4]
C256 = lambda T: (256, 64, 256, T, 80, 16000)


def _stft(case):
    from diffwave_sashimi_amd.mel import TacotronSTFT
    n_fft, hop, win, T, bands, sr = case
    return cases.cached(("mel_backward_stft",) + case[:3] + case[4:], lambda: TacotronSTFT(
        filter_length=n_fft, hop_length=hop, win_length=win, n_mel_channels=bands, sampling_rate=sr, mel_fmin=0.0,
        mel_fmax=min(8000.0, sr / 2.0)))


def _reference(case, x, g, key):
    """Float64 gradient, once per (case, key) in a session."""
    st = _stft(case)
    return cases.cached(("mel_backward_reference", case, key),
                        lambda: mref.mel_gradient(x, g, st.window, st.mel_basis, case[0], case[1]))


def _engine_gradient(st, x, g, gpu):
    xin = x.to(gpu).requires_grad_(True)
    out = st.mel_spectrogram(xin)
    (dx,) = torch.autograd.grad(out, xin, g.to(gpu))
    return dx.cpu()


@pytest.mark.parametrize("case", mref.CASES, ids=IDS)
def test_gradient_matches_the_float64_helper(gpu, case):
    n_fft, hop, win, T, bands, sr = case
    st = _stft(case)
    x, g = mref.case_inputs(case)
    assert x.shape == (3, T)
    smallest = float(mref.mel_energies(x.double(), st.window, st.mel_basis, n_fft, hop).min())
    ref = _reference(case, x, g, "random")
    got = _engine_gradient(st, x, g, gpu)
    err = rel_err(got, ref)
    print(f"{case}: engine vs float64 helper {err:.2e}; smallest mel energy {smallest / mref.CLIP:.1f} x clip")
    assert smallest >= 5 * mref.CLIP          # no clamp decision can flip between float32 and float64
    assert got.shape == ref.shape and torch.isfinite(got).all()
    assert err <= REL_TOL


@pytest.mark.parametrize("T", [1000, 129])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_frame_cotangent_reaches_exactly_its_samples(gpu, T, where):
    case = C256(T)
    st = _stft(case)
    x, _ = mref.case_inputs(case)
    F = T // 64 + 1
    f = {"first": 0, "middle": F // 2, "last": F - 1}[where]
    g = torch.zeros(3, 80, F)
    g[:, 7, f] = 1.0
    g[:, 40, f] = -0.5
    ref = _reference(case, x, g, where)
    got = _engine_gradient(st, x, g, gpu)
    reached = torch.zeros(T, dtype=torch.bool)
    reached[mref.reflect_index(T, 256, 64)[f]] = True
    assert 0 < int(reached.sum()) <= 256
    assert float(ref[:, ~reached].abs().max() if (~reached).any() else 0.0) == 0
    if (~reached).any():
        assert float(got[:, ~reached].abs().max()) == 0          # exactly zero where the frame cannot reach
    worst = float((got.double() - ref).abs().max())
    print(f"T={T} frame {f} of {F}: max |engine - float64| = {worst:.2e} of max|ref| {float(ref.abs().max()):.2e}")
    assert worst <= REL_TOL * float(ref.abs().max())


def test_silent_frames_contribute_exactly_zero(gpu):
    """400 random samples, then 600 exact zeros (torch autograd through the oracle returns NaN there:
    tests/test_mel_operator.py)."""
    case = C256(1000)
    st = _stft(case)
    x, g = mref.case_inputs(case)
    x = x.clone()
    x[:, 400:] = 0
    ref = _reference(case, x, g, "silence")
    got = _engine_gradient(st, x, g, gpu)
    assert torch.isfinite(got).all()
    # frame f covers samples f 64 - 128 .. f 64 + 127: frame 8 (384 .. 639) is the last one that sees a non-zero sample
    assert float(got[:, 640:].abs().max()) == 0 and float(ref[:, 640:].abs().max()) == 0
    err = rel_err(got[:, :640], ref[:, :640])
    print(f"silence: engine vs float64 helper on the reached samples {err:.2e}")
    assert err <= REL_TOL


def test_quiet_clip_under_the_clamp_has_zero_gradient(gpu):
    case = C256(1000)
    st = _stft(case)
    x, g = mref.case_inputs(case)
    x = x / 0.8 * 1e-7
    assert float(mref.mel_energies(x.double(), st.window, st.mel_basis, 256, 64).max()) < mref.CLIP
    got = _engine_gradient(st, x, g, gpu)
    assert float(got.abs().max()) == 0
    out = st.mel_spectrogram(x.to(gpu))
    # every band of every frame sits on the clamp: one value, log(1e-5) to the rounding of the device's logf
    assert float(out.max()) == float(out.min()) and abs(float(out.max()) - float(torch.log(torch.tensor(1e-5)))) < 2e-6


@pytest.mark.parametrize("case", [C256(129), C256(1000), (256, 100, 256, 1000, 80, 16000)], ids=IDS)
def test_gradient_is_bitwise_reproducible_and_independent_of_the_batch(gpu, case):
    st = _stft(case)
    x, g = mref.case_inputs(case)
    a, b = _engine_gradient(st, x, g, gpu), _engine_gradient(st, x, g, gpu)
    assert torch.equal(a, b)
    for i in range(3):
        assert torch.equal(_engine_gradient(st, x[i:i + 1], g[i:i + 1], gpu)[0], a[i]), i


def test_autograd_surface(gpu):
    from diffwave_sashimi_amd.sampling import mel_operator
    case = C256(1000)
    st = _stft(case)
    x, g = mref.case_inputs(case)
    xg = x.to(gpu)
    plain = st.mel_spectrogram(xg)
    assert plain.grad_fn is None and not plain.requires_grad
    y = xg.clone().requires_grad_(True)
    out = st.mel_spectrogram(y)
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)         # the same kernel, the same bits
    (out * g.to(gpu)).sum().backward()
    assert y.grad is not None and y.grad.shape == y.shape
    assert rel_err(y.grad, _reference(case, x, g, "random")) <= REL_TOL
    with torch.no_grad():
        assert st.mel_spectrogram(y).grad_fn is None
    # the operator: [B, 1, L] and [B, L], no range assertion, the same Function
    A = mel_operator(st)
    assert torch.equal(A(xg), plain) and torch.equal(A(xg[:, None]), plain) and A(xg).grad_fn is None
    wide = (xg * 3).requires_grad_(True)
    with pytest.raises(AssertionError):
        st.mel_spectrogram(wide)
    Aw = A(wide[:, None])
    assert Aw.grad_fn is not None and Aw.shape == plain.shape
    (dw,) = torch.autograd.grad(Aw, wide, g.to(gpu))
    assert torch.isfinite(dw).all() and float(dw.abs().max()) > 0
    # second order is refused by name, not answered with zeros
    y2 = xg.clone().requires_grad_(True)
    (d1,) = torch.autograd.grad((st.mel_spectrogram(y2) * g.to(gpu)).sum(), y2, create_graph=True)
    with pytest.raises(RuntimeError, match="second derivative"):
        d1.sum().backward()


def test_c_abi_argument_checks(gpu):
    from diffwave_sashimi_amd import _lib
    lib = _lib.load()
    st = _stft(C256(1000))
    B, T, F = 2, 1000, 1000 // 64 + 1
    x = torch.zeros(B, T, device=gpu)
    win, basis = st.window.to(gpu), st.mel_basis.to(gpu)
    g, dx, ws = torch.zeros(B, 80, F, device=gpu), torch.zeros(B, T, device=gpu), torch.zeros(B, F, 256, device=gpu)
    stream = _lib.current_stream()

    def call(audio=x, B=B, T=T, window=win, basis=basis, n_fft=256, hop=64, n_mels=80, dout=g, daudio=dx, workspace=ws):
        return lib.dws_mel_spectrogram_backward(_lib.ptr(audio), B, T, _lib.ptr(window), _lib.ptr(basis), n_fft, hop, n_mels,
                                                ctypes.c_float(1e-5), _lib.ptr(dout), _lib.ptr(daudio), _lib.ptr(workspace),
                                                stream)
    assert call() == _lib.DWS_OK
    for null in ("audio", "window", "basis", "dout", "daudio", "workspace"):
        assert call(**{null: None}) == _lib.DWS_ERR_INVALID, null
    assert b"workspace" in lib.dws_last_error()
    for bad in (dict(B=0), dict(hop=0), dict(n_mels=0), dict(T=128), dict(T=0)):
        assert call(**bad) == _lib.DWS_ERR_INVALID, bad
    for n_fft in (32, 100, 8192):
        assert call(n_fft=n_fft) == _lib.DWS_ERR_UNSUPPORTED, n_fft
    torch.cuda.synchronize()

"""GPU: ``mel.tv_filter`` (``dws_tv_filter``, csrc/tvfilter_kernels.hip) against the float64 restatement
(tests/tvfilter_reference.py), forwards and as the exact transpose, on standard-normal signals and complex random filters.

Tolerance: not fixed in advance.  On the same inputs a float32 restatement in ``torch.stft`` / ``torch.fft.irfft`` and a
float32 overlap-add (``torch.istft`` refuses the shape whose window sum reaches 0) is measured against float64,
max |difference| / max |float64 result|, and the kernel is held to 8 times that: a direct N-term fp32 sum is expected to be
somewhat worse than an FFT's log N stages, and an indexing error shows at O(1).  The adjoint's float32 restatement is torch
autograd through the forward's.  Every test prints both figures before it asserts; DESIGN.md section 4 ("Spectral prior")
holds the measured values.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import griffinlim_reference as glr
from tests import tvfilter_reference as tvr

pytestmark = pytest.mark.gpu

SHAPES = [(64, 16, 64, 9), (64, 16, 48, 7), (1024, 256, 1024, 6), (1024, 256, 800, 6), (64, 64, 64, 6)]   # n_fft, hop, win, F
OVERLAPPING = [s for s in SHAPES if s[1] <= s[0] // 4]
ROOM = 8.0


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


@functools.lru_cache(maxsize=None)
def _inputs(n_fft, hop, win, F, B=2, real=False):
    """(window, x, g, filt) as the float32 / complex64 values both sides read."""
    rng = np.random.RandomState(n_fft + hop + win + F + 17 * B + int(real))
    T, K = (F - 1) * hop, n_fft // 2 + 1
    x = rng.standard_normal((B, T)).astype(np.float32)
    g = rng.standard_normal((B, T)).astype(np.float32)
    filt = rng.standard_normal((B, K, F)).astype(np.float32)
    if not real:
        filt = (filt + 1j * rng.standard_normal((B, K, F)).astype(np.float32)).astype(np.complex64)
    return glr.hann_window(win, n_fft), x, g, filt


def _min_len(n_fft, hop):
    return -(-(n_fft // 2 + 1) // hop) * hop


def tv_torch(x, filt, w, hop, lengths=None):
    """The forward map in torch at x's dtype, differentiable: ``torch.stft`` (centred, reflect), the product,
    ``irfft``, the window, an overlap-add and the division by the window's sum of squares where that exceeds FLT_MIN."""
    n_fft = w.shape[0]
    rows_out = []
    for b in range(x.shape[0]):
        n = x.shape[1] if lengths is None else int(lengths[b])
        X = torch.stft(x[b:b + 1, :n], n_fft, hop_length=hop, window=w, center=True, pad_mode="reflect", return_complex=True)
        rows = torch.fft.irfft((filt[b:b + 1, :, :X.shape[-1]] * X).transpose(1, 2), n=n_fft, dim=-1)[0] * w    # [F, n_fft]
        F = rows.shape[0]
        s = torch.zeros(n_fft + hop * (F - 1), dtype=x.dtype)
        wss = torch.zeros_like(s)
        for f in range(F):
            s = s + torch.nn.functional.pad(rows[f], (f * hop, hop * (F - 1 - f)))
            wss[f * hop:f * hop + n_fft] += w * w
        s = torch.where(wss > glr.FLT_MIN, s / wss.clamp(min=glr.FLT_MIN), s)
        rows_out.append(torch.nn.functional.pad(s[n_fft // 2:n_fft // 2 + n], (0, x.shape[1] - n)))
    return torch.stack(rows_out)


@functools.lru_cache(maxsize=None)
def _measured(n_fft, hop, win, F, real, adjoint):
    """(float64 result, error of the float32 torch restatement against it relative to max |result|)."""
    w, x, g, filt = _inputs(n_fft, hop, win, F, real=real)
    if not adjoint:
        want = tvr.tv_forward64(x, filt, w, hop)
        got32 = tv_torch(torch.from_numpy(x), torch.from_numpy(filt), torch.from_numpy(w), hop).numpy()
    else:
        want = tvr.tv_adjoint64(g, filt, w, hop)
        x32 = torch.from_numpy(x).clone().requires_grad_()
        tv_torch(x32, torch.from_numpy(filt), torch.from_numpy(w), hop).backward(torch.from_numpy(g))
        got32 = x32.grad.numpy()
    return want, float(np.abs(got32 - want).max() / np.abs(want).max())


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("n_fft,hop,win,F", SHAPES)
def test_against_float64(n_fft, hop, win, F, real, adjoint, gpu):
    from diffwave_sashimi_amd import mel
    w, x, g, filt = _inputs(n_fft, hop, win, F, real=real)
    want, err32 = _measured(n_fft, hop, win, F, real, adjoint)
    got = mel.tv_filter(_dev(g if adjoint else x, gpu), torch.from_numpy(filt).to(gpu), window=_dev(w, gpu), hop_length=hop,
                        adjoint=adjoint)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    err = float(np.abs(got.cpu().numpy() - want).max() / np.abs(want).max())
    print(f"tv_filter {n_fft}/{hop}/{win}, {F} frames, real={real}, adjoint={adjoint}: kernel {err:.3e}, float32 torch {err32:.3e}")
    assert err <= ROOM * err32


@pytest.mark.parametrize("n_fft,hop,win,F", OVERLAPPING)
def test_constant_filter_is_a_gain(n_fft, hop, win, F, gpu):
    """F = 1 returns x and F = 2.5 returns 2.5 x (perfect reconstruction needs overlapping frames: hop <= n_fft/4)."""
    from diffwave_sashimi_amd import mel
    w, x, _, _ = _inputs(n_fft, hop, win, F)
    for gain in (1.0, 2.5):
        filt = torch.full((2, n_fft // 2 + 1, F), gain)
        want = gain * x.astype(np.float64)
        err32 = float(np.abs(tv_torch(torch.from_numpy(x), filt, torch.from_numpy(w), hop).numpy() - want).max() / np.abs(want).max())
        for f in (filt.to(gpu), filt.to(torch.complex64).to(gpu)):
            got = mel.tv_filter(_dev(x, gpu), f, window=_dev(w, gpu), hop_length=hop).cpu().numpy()
            err = float(np.abs(got - want).max() / np.abs(want).max())
            print(f"tv_filter {n_fft}/{hop}/{win}, gain {gain}: kernel {err:.3e}, float32 torch {err32:.3e}")
            assert err <= ROOM * err32


@pytest.mark.parametrize("n_fft,hop,win,F", SHAPES)
def test_adjoint_identity(n_fft, hop, win, F, gpu):
    """<T x, g> = <x, T^T g> with the sums taken in float64.  Each side is an inner product of a float32 result with a
    float32 signal, so the two differ by the inner products of the results' errors with g and with x.  Those errors are
    rounding noise, uncorrelated with the signal they meet, so their inner product grows like the signal's l2 norm (an
    error correlated with it -- a wrong weight at one bin -- grows like the l1 mass and stands out): each result's
    largest error is held to 8 times the float32 restatement's, times that l2 norm."""
    from diffwave_sashimi_amd import mel
    w, x, g, filt = _inputs(n_fft, hop, win, F)
    fd, wd = torch.from_numpy(filt).to(gpu), _dev(w, gpu)
    tx = mel.tv_filter(_dev(x, gpu), fd, window=wd, hop_length=hop).cpu().numpy().astype(np.float64)
    tg = mel.tv_filter(_dev(g, gpu), fd, window=wd, hop_length=hop, adjoint=True).cpu().numpy().astype(np.float64)
    lhs, rhs = float((tx * g).sum()), float((x * tg).sum())
    want_f, e_f = _measured(n_fft, hop, win, F, False, False)
    want_a, e_a = _measured(n_fft, hop, win, F, False, True)
    l2 = lambda a: float(np.sqrt((a.astype(np.float64) ** 2).sum()))
    bound = ROOM * (e_f * np.abs(want_f).max() * l2(g) + e_a * np.abs(want_a).max() * l2(x))
    print(f"tv_filter {n_fft}/{hop}/{win}: <Tx, g> = {lhs!r}, <x, T^T g> = {rhs!r}, difference {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("n_fft,hop,win,F", SHAPES)
def test_autograd(n_fft, hop, win, F, gpu):
    """The gradient of ``mel.tv_filter`` (both directions' backward) against float64 torch autograd through ``torch.stft``
    and ``torch.istft`` -- through the overlap-add of ``tv_torch`` at the shape ``torch.istft`` refuses (its window sum
    reaches 0)."""
    from diffwave_sashimi_amd import mel
    w, x, g, filt = _inputs(n_fft, hop, win, F)
    w64, f64, T = torch.from_numpy(w).double(), torch.from_numpy(filt).to(torch.complex128), x.shape[1]
    x64 = torch.from_numpy(x).double().requires_grad_()
    if hop <= n_fft // 4:
        X = torch.stft(x64, n_fft, hop_length=hop, window=w64, center=True, pad_mode="reflect", return_complex=True)
        y64 = torch.istft(f64 * X, n_fft, hop_length=hop, window=w64, center=True, length=T)
    else:
        y64 = tv_torch(x64, f64, w64, hop)
    y64.backward(torch.from_numpy(g).double())
    want = x64.grad.numpy()
    _, err32 = _measured(n_fft, hop, win, F, False, True)
    xd = _dev(x, gpu).requires_grad_()
    fd, wd = torch.from_numpy(filt).to(gpu), _dev(w, gpu)
    y = mel.tv_filter(xd, fd, window=wd, hop_length=hop)
    assert y.requires_grad
    y.backward(_dev(g, gpu))
    err = float(np.abs(xd.grad.cpu().numpy() - want).max() / np.abs(want).max())
    print(f"tv_filter {n_fft}/{hop}/{win}: autograd {err:.3e}, float32 torch {err32:.3e}")
    assert err <= ROOM * err32
    # the gradient IS the adjoint call, and the adjoint's gradient is the forward call, bit for bit
    assert torch.equal(xd.grad, mel.tv_filter(_dev(g, gpu), fd, window=wd, hop_length=hop, adjoint=True))
    gd = _dev(g, gpu).requires_grad_()
    mel.tv_filter(gd, fd, window=wd, hop_length=hop, adjoint=True).backward(_dev(x, gpu))
    assert torch.equal(gd.grad, y.detach())
    # first order only
    x2 = _dev(x, gpu).requires_grad_()
    (g1,) = torch.autograd.grad((mel.tv_filter(x2, fd, window=wd, hop_length=hop) ** 2).sum(), x2, create_graph=True)
    with pytest.raises(RuntimeError, match="second derivative"):
        g1.sum().backward()
    with pytest.raises(ValueError, match="requires grad"):
        mel.tv_filter(xd, fd.clone().requires_grad_(), window=wd, hop_length=hop)


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("n_fft,hop,win,F", SHAPES)
def test_ragged(n_fft, hop, win, F, adjoint, gpu):
    """B = 3 with lengths T, T - hop (one frame fewer) and the shortest the reflection admits, n_fft/2 + 1 rounded up to the
    hop: float64 parity, row b bit-equal to the B = 1 run on the clip alone, exact zeros behind a clip's length, and NaNs
    planted in the signal and in the filter frames behind a clip's own change nothing."""
    from diffwave_sashimi_amd import mel
    w, x, g, filt = _inputs(n_fft, hop, win, F, B=3)
    src = g if adjoint else x
    T = x.shape[1]
    lengths = [T, T - hop, _min_len(n_fft, hop)]
    assert lengths[2] <= lengths[1] < T
    wd = _dev(w, gpu)
    kw = dict(window=wd, hop_length=hop, adjoint=adjoint)
    got = mel.tv_filter(_dev(src, gpu), torch.from_numpy(filt).to(gpu), lengths=lengths, **kw)
    want = (tvr.tv_adjoint64 if adjoint else tvr.tv_forward64)(src, filt, w, hop, lengths)
    x32 = torch.from_numpy(x if adjoint else src).clone().requires_grad_(adjoint)      # the float32 restatement, same inputs
    y32 = tv_torch(x32, torch.from_numpy(filt), torch.from_numpy(w), hop, lengths)
    if adjoint:
        y32.backward(torch.from_numpy(src))
        y32 = x32.grad
    err32 = float(np.abs(y32.detach().numpy() - want).max() / np.abs(want).max())
    err = float(np.abs(got.cpu().numpy() - want).max() / np.abs(want).max())
    print(f"tv_filter {n_fft}/{hop}/{win}, ragged, adjoint={adjoint}: kernel {err:.3e}, float32 torch {err32:.3e}")
    assert err <= ROOM * err32
    dirty_x, dirty_f = src.copy(), filt.copy()
    for b, n in enumerate(lengths):
        assert not bool(got[b, n:].any())                                           # exactly 0 (and +0) behind the clip
        dirty_x[b, n:] = np.nan
        dirty_f[b, :, n // hop + 1:] = np.nan
        alone = mel.tv_filter(_dev(src[b:b + 1, :n], gpu), torch.from_numpy(filt[b:b + 1, :, :n // hop + 1]).to(gpu), **kw)
        assert torch.equal(got[b, :n], alone[0])
    again = mel.tv_filter(_dev(dirty_x, gpu), torch.from_numpy(dirty_f).to(gpu), lengths=torch.tensor(lengths), **kw)
    assert torch.equal(again, got)


def test_repeatable(gpu):
    from diffwave_sashimi_amd import mel
    w, x, g, filt = _inputs(1024, 256, 800, 6)
    for adjoint in (False, True):
        runs = [mel.tv_filter(_dev(x, gpu), torch.from_numpy(filt).to(gpu), window=_dev(w, gpu), hop_length=256, adjoint=adjoint)
                for _ in range(3)]
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_python_refusals(gpu):
    from diffwave_sashimi_amd import mel
    w, x, _, filt = _inputs(64, 16, 64, 9)
    xd, fd, wd = _dev(x, gpu), torch.from_numpy(filt).to(gpu), _dev(w, gpu)
    with pytest.raises(ValueError, match="complex64 or float32"):
        mel.tv_filter(xd, fd.to(torch.complex128), window=wd, hop_length=16)
    with pytest.raises(ValueError, match="filt"):
        mel.tv_filter(xd, fd[:, :, :-1], window=wd, hop_length=16)
    with pytest.raises(ValueError, match="GPU only"):
        mel.tv_filter(xd.cpu(), fd, window=wd, hop_length=16)
    with pytest.raises(ValueError, match="float32 tensor \\[B, T\\]"):
        mel.tv_filter(xd.double(), fd, window=wd, hop_length=16)
    with pytest.raises(ValueError, match="adjoint"):
        mel.tv_filter(xd, fd, window=wd, hop_length=16, adjoint=1)
    with pytest.raises(ValueError, match="hop_length"):
        mel.tv_filter(xd, fd, window=wd, hop_length=0)
    with pytest.raises(ValueError, match="multiple of hop_length"):
        mel.tv_filter(xd, fd, window=wd, hop_length=16, lengths=[128, 100])


def test_abi_refusals(gpu):
    from diffwave_sashimi_amd import _lib
    lib = _lib.load()
    n_fft, hop, win, F = 64, 16, 64, 9
    w, x, _, filt = _inputs(n_fft, hop, win, F)
    T = (F - 1) * hop
    wd, xd = _dev(w, gpu), _dev(x, gpu)
    fr = _dev(filt.real, gpu)
    out = torch.empty(2, T, device=gpu)
    ws = torch.empty(lib.dws_griffin_lim_workspace(2, F, n_fft, hop, 0) // 4, device=gpu)
    dev_len = torch.tensor([T, T - hop], dtype=torch.int32, device=gpu)

    def tv(x=xd.data_ptr(), fr=fr.data_ptr(), lengths=0, host=None, n_fft=n_fft, hop=hop, adjoint=0, F=F, out=out.data_ptr(),
           ws=ws.data_ptr(), window=wd.data_ptr(), B=2):
        return lib.dws_tv_filter(x, B, F, lengths, host, fr, 0, window, n_fft, hop, adjoint, out, ws, _lib.current_stream())

    def message():
        return lib.dws_last_error().decode()

    assert tv() == _lib.DWS_OK
    assert tv(lengths=dev_len.data_ptr(), host=(ctypes.c_int32 * 2)(T, T - hop)) == _lib.DWS_OK
    assert tv(fr=0) == _lib.DWS_ERR_INVALID and "dws_tv_filter: null filt_re" in message()
    for bad in (2, -1):
        assert tv(adjoint=bad) == _lib.DWS_ERR_INVALID and f"adjoint = {bad}" in message()
    assert tv(x=0) == _lib.DWS_ERR_INVALID and "dws_tv_filter: null x" in message()
    assert tv(window=0) == _lib.DWS_ERR_INVALID and "window" in message()
    assert tv(out=0) == _lib.DWS_ERR_INVALID and "out" in message()
    assert tv(ws=0) == _lib.DWS_ERR_INVALID and "workspace" in message()
    assert tv(B=0) == _lib.DWS_ERR_INVALID and "B = 0" in message()
    assert tv(hop=0) == _lib.DWS_ERR_INVALID and "hop = 0" in message()
    assert tv(F=1) == _lib.DWS_ERR_INVALID and "f_max = 1" in message()
    assert tv(n_fft=48) == _lib.DWS_ERR_UNSUPPORTED and "n_fft = 48" in message()
    assert tv(n_fft=8192) == _lib.DWS_ERR_UNSUPPORTED and "n_fft = 8192" in message()
    assert tv(lengths=dev_len.data_ptr()) == _lib.DWS_ERR_INVALID and "lengths_host" in message()
    assert tv(lengths=dev_len.data_ptr(), host=(ctypes.c_int32 * 2)(T, T - 8)) == _lib.DWS_ERR_INVALID
    assert "not a multiple of hop" in message()
    assert tv(lengths=dev_len.data_ptr(), host=(ctypes.c_int32 * 2)(32, T)) == _lib.DWS_ERR_INVALID and "clip 0 has 32" in message()
    assert tv(lengths=dev_len.data_ptr(), host=(ctypes.c_int32 * 2)(T, T + hop)) == _lib.DWS_ERR_INVALID and "clip 1" in message()
    torch.cuda.synchronize()

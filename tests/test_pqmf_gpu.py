"""GPU: ``dws_pqmf_analysis`` / ``dws_pqmf_synthesis`` through ``pqmf.PQMF`` against the float64 restatement of
tests/pqmf_reference.py.

The bound is derived, not tuned.  An output is ``gain x`` a sum of ``terms`` products accumulated by fp32 fmaf in a fixed
order; with ``A = sum |filt . input|`` and u = 2^-24 the accumulation errs by at most ``terms u A`` (to first order), the
fp32 rounding of the table entries by ``u A``, the product with the gain by ``u A`` (K is a power of two: exact; one more
for a general gain) and nothing else is rounded (the inputs are float32 values on both sides):

    |err| <= (terms + 4) 2^-24 A        per output

where A and terms come from the restatement.  An output with no product (terms = 0) is exactly 0."""
import functools

import numpy as np
import pytest
import torch

from diffwave_sashimi_amd.pqmf import PQMF, TILE
from tests import pqmf_reference as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BANKS = [(4, 62), (2, 62), (4, 6), (2, 6)]


def lengths(K):
    """Full-band lengths: one output per band (the whole clip inside the halo), two, 40 (shorter than the 62-tap filter),
    both sides of the tile, and more than two tiles with a ragged end."""
    return [K, 2 * K, 40, TILE - K, TILE, TILE + K, 2 * TILE + 3 * K]


def bank(K, taps):
    return PQMF(K, taps, cutoff=None if taps == 62 else 0.2)


@functools.lru_cache(maxsize=None)
def clips(T, seed):
    """[3, T] float32: seeded normals, all zeros, and a single 1 at each end (the impulse responses at both edges)."""
    x = torch.zeros(3, T)
    x[0] = torch.randn(T, generator=torch.Generator().manual_seed(seed))
    x[2, 0] = 1.0
    x[2, T - 1] = 1.0
    return x


def check(got, want, A, terms, what):
    got = got.detach().double().cpu().numpy()
    bound = (terms + 4) * U * A
    err = np.abs(got - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max |err| {err.max():.3e}, largest share of the bound {worst:.3f}, max |ref| {np.abs(want).max():.3e}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), what
    assert not got[terms == 0].any()


@pytest.mark.parametrize("K,taps", BANKS)
def test_analysis_against_float64(gpu, K, taps):
    P = bank(K, taps)
    ha, _ = P.filters()
    for T in lengths(K):
        x = clips(T, 11 + T)
        got = P.analysis(x.to(gpu))
        assert got.shape == (3, K, T // K) and got.dtype == torch.float32
        want, A, terms = ref.analysis(x.numpy(), ha)
        check(got, want, A, terms, f"analysis K={K} taps={taps} T={T}")
        assert not got[1].any() and got[0].abs().max() > 0
        # [B, 1, T] is the same call; clip b of the batch is the B = 1 run of that clip; a second run is the first
        assert torch.equal(P.analysis(x[:, None].to(gpu)), got) and torch.equal(P.analysis(x.to(gpu)), got)
        for b in range(3):
            assert torch.equal(P.analysis(x[b:b + 1].to(gpu))[0], got[b])


@pytest.mark.parametrize("K,taps", BANKS)
def test_synthesis_against_float64(gpu, K, taps):
    P = bank(K, taps)
    _, hs = P.filters()
    for T in lengths(K):
        s = clips(T, 23 + T).reshape(3, K, T // K)        # (the impulses land in band 0 and band K - 1)
        got = P.synthesis(s.to(gpu))
        assert got.shape == (3, 1, T) and got.dtype == torch.float32
        want, A, terms = ref.synthesis(s.numpy(), hs, gain=float(K))
        check(got[:, 0], want, A, terms, f"synthesis K={K} taps={taps} T={T}")
        assert not got[1].any() and got[0].abs().max() > 0
        assert torch.equal(P.synthesis(s.to(gpu)), got)
        for b in range(3):
            assert torch.equal(P.synthesis(s[b:b + 1].to(gpu))[0], got[b])
        # zero padding behind the clip's end changes no bit of the clip: a ragged batch synthesises every clip as alone
        for pad in (1, 7, TILE // K + 5):
            padded = torch.cat([s, torch.zeros(3, K, pad)], dim=2)
            assert torch.equal(P.synthesis(padded.to(gpu))[..., :T], got), (T, pad)


@pytest.mark.parametrize("K,taps", BANKS)
def test_adjoints_against_float64(gpu, K, taps):
    P = bank(K, taps)
    ha, hs = P.filters()
    for T in lengths(K):
        g = torch.Generator().manual_seed(31 + T)
        x = torch.randn(3, T, generator=g)
        w = torch.randn(3, K, T // K, generator=g)
        s = torch.randn(3, K, T // K, generator=g)
        v = torch.randn(3, 1, T, generator=g)
        xg = x.to(gpu).requires_grad_(True)
        Ax = P.analysis(xg)
        (Ax * w.to(gpu)).sum().backward()
        want, A, terms = ref.analysis_transpose(w.numpy(), ha)
        check(xg.grad, want, A, terms, f"analysis adjoint K={K} taps={taps} T={T}")
        sg = s.to(gpu).requires_grad_(True)
        Ss = P.synthesis(sg)
        (Ss * v.to(gpu)).sum().backward()
        want, A, terms = ref.synthesis_transpose(v[:, 0].numpy(), hs, K, gain=float(K))
        check(sg.grad, want, A, terms, f"synthesis adjoint K={K} taps={taps} T={T}")
        # <A x, w> = <x, A^T w>, the inner products in float64.  Both sides are fp32 evaluations of one trilinear sum
        # sum f x w: each output errs by at most (terms + 4) u A, so each side by at most (terms_max + 4) u S with
        # S = sum |f| |x| |w| = sum_out A_out |w_out|, and the two differ by at most twice that.
        S_a = float((ref.analysis(x.numpy(), ha)[1] * w.abs().double().numpy()).sum())
        S_s = float((ref.synthesis(s.numpy(), hs, float(K))[1] * v[:, 0].abs().double().numpy()).sum())
        for fwd, cot, inp, grad, S, name in ((Ax, w, x, xg.grad, S_a, "analysis"), (Ss, v, s, sg.grad, S_s, "synthesis")):
            lhs = float((fwd.detach().double().cpu() * cot.double()).sum())
            rhs = float((inp.double() * grad.double().cpu()).sum())
            print(f"{name} K={K} taps={taps} T={T}: <Ax,w> {lhs:.9e}  <x,A'w> {rhs:.9e}  bound {2 * (taps + K + 4) * U * S:.2e}")
            assert abs(lhs - rhs) <= 2 * (taps + K + 4) * U * S


def test_second_derivative_is_an_error(gpu):
    P = PQMF(4)
    x = torch.randn(1, 64, generator=torch.Generator().manual_seed(1)).to(gpu).requires_grad_(True)
    (g,) = torch.autograd.grad(P.analysis(x).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    with torch.no_grad():
        assert not P.analysis(x).requires_grad


@pytest.mark.parametrize("K", (2, 4))
def test_round_trip_on_the_gpu(gpu, K):
    P = PQMF(K)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 1024)).astype(np.float32))
    y = P.synthesis(P.analysis(x.to(gpu)))[:, 0].double().cpu()
    d = (y - x.double())[0, 64:-64]
    err = float(torch.sqrt((d * d).sum() / (x.double()[0, 64:-64] ** 2).sum()))
    print(f"round trip K={K}: interior relative error {err:.3e}")
    assert err <= 1e-3


def test_library_refuses_bad_arguments(gpu):
    from diffwave_sashimi_amd import _lib
    lib = _lib.load()
    x = torch.zeros(2, 64, device=gpu)
    f = torch.zeros(4, 63, device=gpu)
    out = torch.zeros(2, 64, device=gpu)
    st = _lib.current_stream()
    good = (x.data_ptr(), 2, 64, f.data_ptr(), 4, 62, 1.0, out.data_ptr(), st)
    assert lib.dws_pqmf_analysis(*good) == _lib.DWS_OK
    assert lib.dws_pqmf_synthesis(x.data_ptr(), 2, 16, f.data_ptr(), 4, 62, 1.0, out.data_ptr(), st) == _lib.DWS_OK
    for i, bad in ((0, 0), (3, 0), (7, 0), (4, 3), (4, 8), (5, 61), (5, 0), (5, 256), (2, 62), (2, 0), (1, 0)):
        args = list(good)
        args[i] = bad
        assert lib.dws_pqmf_analysis(*args) == _lib.DWS_ERR_INVALID, (i, bad)
        if i != 2:
            args[2] = 16
            assert lib.dws_pqmf_synthesis(*args) == _lib.DWS_ERR_INVALID, (i, bad)
    assert lib.dws_pqmf_synthesis(x.data_ptr(), 2, 0, f.data_ptr(), 4, 62, 1.0, out.data_ptr(), st) == _lib.DWS_ERR_INVALID
    torch.cuda.synchronize()


def test_stft_loss_gradient_through_the_synthesis_bank(gpu):
    """``mr_stft_loss(P.synthesis(s), y)`` differentiated in ``s`` at one resolution (64, 16, 64), K = 4, Ts = 96, against
    float64 torch autograd through tests/stft_loss_reference.py and a ``conv_transpose1d`` restatement of the bank.  The
    tolerance is the one tests/test_stft_loss_gpu.py asserts for the loss at default weights (relative L2 <= 2e-3: the
    log-magnitude term is ill-conditioned at weak bins in any float32 evaluation); the bank adds rounding at the 1e-7
    level."""
    from diffwave_sashimi_amd.metrics import mr_stft_loss
    from tests import stft_loss_reference as sref
    from tests.test_stft_loss_gpu import FULL_TOL
    K, Ts, res = 4, 96, ((64, 16, 64),)
    P = PQMF(K)
    _, hs = P.filters()
    g = torch.Generator().manual_seed(77)
    s = torch.randn(2, K, Ts, generator=g) * 0.1
    y = torch.randn(2, K * Ts, generator=g) * 0.1

    def bank64(t):      # the synthesis bank as a transposed convolution with the tap-reversed filters, in float64
        flt = torch.from_numpy(np.ascontiguousarray(hs[:, ::-1]))[:, None, :]
        full = K * torch.nn.functional.conv_transpose1d(t, flt, stride=K)
        return full[:, 0, P.taps // 2:P.taps // 2 + K * Ts]
    assert np.abs(bank64(s.double()).numpy() - ref.synthesis(s.numpy(), hs, float(K))[0]).max() <= 1e-13
    s64 = s.double().requires_grad_(True)
    sref.loss(bank64(s64), y, None, res).sum().backward()
    sg = s.to(gpu).requires_grad_(True)
    loss = mr_stft_loss(P.synthesis(sg), y.to(gpu), resolutions=res)
    loss.sum().backward()
    err = sref.rel_l2(sg.grad, s64.grad)
    print(f"stft loss through the bank: loss {loss.tolist()}, gradient rel L2 {err:.2e}")
    assert torch.isfinite(sg.grad).all() and err <= FULL_TOL

"""Shared pieces of the any-length adjoint tests of the S4 long convolution (tests/test_s4_convolution_adjoint_any_length_gpu.py,
..._any_length_reference.py): the cases at l_max != L, and a float64 restatement of the SEGMENT scheme of
`fftconv_seg_kernel` (csrc/fftconv_kernels.hip, FftConvSegArgs) with its adjoint.

Segment scheme, S samples per segment, transforms of n = 2 S points.  With K the two-sided kernel (k0[d] at lag d >= 0,
k1[m-1] at lag -m, at most S taps per direction), Kc / Ka its causal / anti-causal half alone and ' a shift by S (bin k
times (-1)^k):

    y_j = first half of IFFT( A_j F(K) + A_{j-1} F(Kc)' + A_{j+1} F(Ka)' )          A_i: spectrum of input segment i

The adjoint du[s] = sum_t K[t - s] da[t] is the convolution with the time-reversed kernel R[d] = K[-d].  Its spectrum is
conj(F(K)); its causal half is the reversed anti-causal half of K (plus lag 0, which no neighbour segment ever reads: a
neighbour's lags are >= 1), its anti-causal half the reversed causal one.  The shift factor is real, so

    du_j = first half of IFFT( dA_j conj(F(K)) + dA_{j-1} conj(F(Ka)') + dA_{j+1} conj(F(Kc)') )

-- the same accumulation on the same three spectra, conjugated, the causal' and anti-causal' ones swapped."""
import torch

from tests import cases, s4conv

# (H, B, l_max, L, weight seed) by stage type
FUSED_CASES = [(8, 2, 4096, 1000, 6),                       # truncated taps
               (8, 2, 1024, 4096, s4conv.WEIGHT_SEED)]      # clamped taps
SEGMENTED_CASES = [(8, 1, 16384, 16386, s4conv.WEIGHT_SEED),    # a 2-sample second segment
                   (8, 2, 16384, 32768, s4conv.WEIGHT_SEED),    # exactly two segments, B > 1
                   (8, 1, 16384, 40000, s4conv.WEIGHT_SEED)]    # two segments and a bit
ROCFFT_CASES = SEGMENTED_CASES[:2]                          # again with every stage on rocFFT
ALL_CASES = FUSED_CASES + SEGMENTED_CASES
SEGMENT = 16384


def prepare_case(H, B, l_max, L, seed):
    """(cfg, net on the host with both ReLUs opened, audio, steps, cotangents, the two ReLU minima): `s4conv.prepare_adjoint_case`
    with the kernels set up for l_max and the run at L."""
    cfg, net = s4conv.build_isolated_block(H, l_max, seed)
    audio, steps = cases.wavenet_inputs(B, L, 1, s4conv.INPUT_SEED)
    minima = s4conv.open_relus(net.state_dict(), cfg, audio, steps)
    net.invalidate()
    return cfg, net, audio, steps, s4conv.edge_cotangents(B, L, s4conv.COTANGENT_SEED), minima


def segment_spectra(k0, k1, S):
    """(F(K), F(Kc)', F(Ka)') [H, S + 1] in float64 for taps k0 / k1 [H, Lt], Lt <= S."""
    Lt, n = k0.shape[-1], 2 * S
    assert Lt <= S and k0.dtype == torch.float64
    kc = torch.zeros(k0.shape[:-1] + (n,), dtype=torch.float64)
    ka = torch.zeros_like(kc)
    kc[..., :Lt] = k0
    ka[..., n - Lt:] = k1.flip(-1)
    sign = 1.0 - 2.0 * (torch.arange(S + 1) % 2).double()
    return torch.fft.rfft(kc + ka, n=n), torch.fft.rfft(kc, n=n) * sign, torch.fft.rfft(ka, n=n) * sign


def segment_accumulate(u, own, left, right, S):
    """Output segment j = first half of IFFT(A_j own + A_{j-1} left + A_{j+1} right), every j; u [..., H, L]."""
    L, n = u.shape[-1], 2 * S
    nseg = -(-L // S)
    A = [torch.fft.rfft(u[..., j * S:min(L, (j + 1) * S)], n=n) for j in range(nseg)]
    out = []
    for j in range(nseg):
        Y = A[j] * own
        if j > 0:
            Y = Y + A[j - 1] * left
        if j + 1 < nseg:
            Y = Y + A[j + 1] * right
        out.append(torch.fft.irfft(Y, n=n)[..., :min(S, L - j * S)])
    return torch.cat(out, -1)


def segmented_conv(u, k0, k1, S=SEGMENT):
    """conv(u, k) by the segment scheme."""
    full, c, a = segment_spectra(k0, k1, S)
    return segment_accumulate(u, full, c, a, S)


def segmented_adjoint(da, k0, k1, S=SEGMENT, swap=True, conj=True):
    """conv^T(da) by the segment scheme on the FORWARD's three spectra.  swap=False: the causal' / anti-causal' spectra in
    the forward's order; conj=False: not conjugated -- the two mistakes the adjoint instance could make."""
    full, c, a = segment_spectra(k0, k1, S)
    f = (lambda z: z.conj()) if conj else (lambda z: z)
    left, right = (a, c) if swap else (c, a)
    return segment_accumulate(da, f(full), f(left), f(right), S)


class ConvWithAdjoint(torch.autograd.Function):
    """The right convolution forward (`s4conv.two_sided_conv_fft`) whose backward towards u is `adjoint(da, k0, k1)`:
    the `conv=` hook of `s4conv.adjoint_reference` with a deliberately wrong (or an independently written) adjoint.  Taps
    are constants."""

    @staticmethod
    def forward(ctx, u, k0, k1, adjoint):
        ctx.k, ctx.adjoint = (k0, k1), adjoint
        return s4conv.two_sided_conv_fft(u, k0, k1)

    @staticmethod
    def backward(ctx, da):
        return ctx.adjoint(da, *ctx.k), None, None, None


def conv_with_adjoint(adjoint):
    return lambda u, k0, k1: ConvWithAdjoint.apply(u, k0, k1, adjoint)

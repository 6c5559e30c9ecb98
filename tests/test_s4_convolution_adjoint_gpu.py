"""Function-level GPU parity of the ADJOINT of the S4 long convolution (SURVEY.md section 8, row a14 backwards: what every
SaShiMi training step and every guided sampling step runs) at every transform plan, on the fused kernels and on rocFFT.

The one-block network of tests/s4conv.py with both ReLUs held open (`open_relus`: every float64 pre-activation >= 0.25) has
everything around the convolution pointwise in time and smooth, so a cotangent of eps reaches the convolution's output with
exactly its own support, and what the test sees is the convolution adjoint and what it feeds:

  audio.grad                   du = conv^T(da) + D da through LN1^T and the init conv: `fftconv_kernel` with conj_k / no_act
                               (RSUM on even plans in a full backward, plain on odd plans and in a data-only backward), or
                               `rocfft_conv_backward`; off the support of a head / tail cotangent it is a read-out of the taps
  layer.D, fc_t.*              the zero lag of `fftcorr`'s summed partial spectra, and the row sums (fused / launch_rowsum_bc /
                               the rocFFT epilogue)
  kernel.*, norm1.*            the spectrum and taps adjoint fed by `fftcorr_kernel` / `fftcorr_blk_kernel`, LN1's scalars

against torch autograd through the CPU oracle in FLOAT64 (`s4conv.adjoint_reference`; the reference side is checked in
tests/test_s4_convolution_adjoint_reference.py, including that four kinds of wrong adjoint move these measures above their
bounds).  Three cotangents per case: dense, and N(0, 1) on the first / last max(2, L // 16) positions with exact zeros
elsewhere.  One train()-mode backward (the full one) and one eval()-mode backward (data-only) per cotangent; the two
audio gradients must be bit-equal.  The launch profile asserts which path ran.

  measure                                                                          bound
  audio.grad: per batch row max_l |got - ref| / max_l |ref_branch|, worst row      2e-5   (ref_branch: the part through the S4 branch)
  audio.grad off the support: per row max |got - ref| / max |ref| over l not in S  2e-5
  layer.D, fc_t.weight, fc_t.bias: max |got - ref| / max |ref|                     2e-5
  kernel.C, B, P, inv_w_real, w_imag, norm1.m, norm1.s: the same                   1e-4
  kernel.log_dt                                                                    gradcheck.compare: 1e-3, or 3x the fp32 oracle's
                                                                                   own distance from float64, capped at MAX_TOL

2e-5 is what tests/test_s4_convolution_gpu.py holds the same transform to, 1e-4 the project's function-level bound of the
kernel generator and the Cauchy operator; the fp32 CPU oracle sits at least 4x below each on every case (asserted on the
CPU).  Every case prints the engine's error, the fp32 oracle's, their ratio and where the engine's worst value lies.

Measured on an MI355X (256 CUs), precision "f32", over the 29 cases (these figures did not exist before this file):
  audio.grad, all positions   engine at most 6.42e-6 (H = 6, B = 3, L = 1024, tail cotangent, b = 0, l = 1017); fp32 oracle at
                              most 4.27e-6 (L = 1022); largest ratio of the two per case 3.1
  audio.grad off the support  7.53e-6 (the same case, l = 718); oracle 3.85e-6 (H = 64, B = 17, L = 1024); ratio at most 3.2
  layer.D, fc_t.*             5.00e-6 (L = 4098, dense, fc_t.weight); oracle 3.97e-6 (H = 64, B = 9, L = 2048); ratio at most 3.2
  kernel.*, norm1.*           3.18e-5 (H = 64, B = 9, L = 8192, tail, norm1.m), 2.68e-5 (L = 8192, tail, norm1.s), 2.07e-5 (L = 18,
                              dense, norm1.m): every case's worst above 1e-5 is norm1.m or norm1.s; where a kernel tensor is a
                              case's worst it is at most 8.88e-6 (H = 64, B = 9, L = 2048, w_imag); oracle 1.79e-5 (the same
                              case); ratio at most 8.5 (L = 250: 1.29e-5 against 1.51e-6)
  kernel.log_dt               at most 9.1e-4 (L = 2048, dense; its bound there 1.7e-3), no case beyond 1e-3
No dependence on the plan, on the row count or on the number of samples a `fftcorr` workgroup walks: the H = 64 batch-chunk
cases (chunks of 2 + 1 and 3 + 2, the parked-U instance at 16384 included) sit at 1.2e-6 .. 3.0e-6 on the audio gradient and
0.7e-6 .. 3.2e-6 on D / fc_t, the rocFFT cases at 0.5e-6 .. 4.2e-6.  Launch counts (fftconv, fftcorr in a full backward;
the same in a data-only one): (1, 1, 1, 0) on every fused case, (0, 0, 0, 0) on every rocFFT case.  The data-only audio
gradient had the full backward's bits in every case.  The largest case takes 13 s, of which the host reference takes 11.
"""
import ctypes

import pytest
import torch

from diffwave_sashimi_amd import _lib
from tests import gradcheck, s4conv
from tests.test_s4_convolution_gpu import PLAN_EDGES

pytestmark = pytest.mark.gpu

FUSED, ROCFFT = "fused", "rocfft"


def _backward(net, gpu, audio, steps, cot, count):
    """One forward / backward of (eps * cot).sum() with the launch profile on for `count` around the backward:
    (audio.grad, {parameter: gradient} or None after a data-only backward, launches whose name contains `count`)."""
    lib = _lib.load()
    net.zero_grad(set_to_none=True)
    a = audio.to(gpu).requires_grad_(True)
    eps = net((a, steps.to(gpu)))
    torch.cuda.synchronize()
    _lib.check(lib.dws_profile_enable(count))
    try:
        eps.backward(cot.to(gpu))
        torch.cuda.synchronize()
        n, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
        _lib.check(lib.dws_profile_query(ctypes.byref(n), ctypes.byref(ms)))
    finally:
        lib.dws_profile_disable()
    grads = {k: p.grad.detach().cpu() for k, p in net.named_parameters() if p.grad is not None}
    return a.grad.detach().cpu(), grads or None, int(n.value)


def _check_case(gpu, H, B, L, path):
    cfg, net, audio, steps, cots, minima = s4conv.prepare_adjoint_case(H, B, L)
    assert min(minima) >= 0.25
    net = net.to(gpu)
    net.invalidate()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    assert s4conv.tail_is_transparent(sd, H)                          # read back from the device
    assert int(sd[s4conv.KERNEL + "L"]) == L
    full, data = {}, {}
    net.train()
    for name, count in zip(s4conv.COTANGENTS, (b"fftconv", b"fftcorr", b"fftconv")):
        full[name] = _backward(net, gpu, audio, steps, cots[name], count)
        assert full[name][1] is not None and len(full[name][1]) == len(list(net.parameters()))
    net.eval()
    for name, count in zip(s4conv.COTANGENTS, (b"fftconv", b"fftcorr", b"fftconv")):
        data[name] = _backward(net, gpu, audio, steps, cots[name], count)
        assert data[name][1] is None                                   # the backward was data-only
    # which path ran: (fftconv, fftcorr) launches of a full backward, of a data-only one
    counts = (full["dense"][2], full["head"][2], data["dense"][2], data["head"][2])
    assert counts == ((1, 1, 1, 0) if path == FUSED else (0, 0, 0, 0)), f"expected the {path} adjoint, launches {counts}"
    k_tap = None
    if (H, B, L) in s4conv.K_TAP_CASES:       # taps as constants: the engine's own
        with torch.no_grad():
            net((audio[:1].to(gpu), steps[:1].to(gpu)))
        k_tap = net.read_tap("k:" + s4conv.BLOCK, (2, H, L)).cpu()
    refs = s4conv.host_references(sd, cfg, audio, steps, cots, k_tap)
    worst, worst_or, failures = {}, {}, []       # per measure: the engine's largest error and where, the fp32 oracle's largest

    def note(measure, bound, err, err_or, where):
        if err > worst.get(measure, (-1.0,))[0]:
            worst[measure] = (err, where)
        worst_or[measure] = max(worst_or.get(measure, 0.0), err_or)
        if not err < bound:
            failures.append(f"{measure} {where}: {err:.2e} >= {bound:g} (fp32 oracle {err_or:.2e})")

    for name in s4conv.COTANGENTS:
        da, grads = refs["ref"][name]
        da32, grads32 = refs["oracle32"][name]
        off = s4conv.off_support(name, L)
        assert torch.isfinite(full[name][0]).all() and full[name][0].shape == (B, 1, L)
        if not torch.equal(data[name][0], full[name][0]):
            failures.append(f"{name}: data-only and full backward differ in audio.grad by "
                            f"{float((data[name][0] - full[name][0]).abs().max()):.2e}")
        every, offs = s4conv.audio_errors(full[name][0], da, refs["branch"][name], off)
        every32, offs32 = s4conv.audio_errors(da32, da, refs["branch"][name], off)
        note("audio", s4conv.AUDIO_BOUND, every[0], every32[0], f"{name} b={every[1]} l={every[2]}")
        if off is not None:
            note("off support", s4conv.AUDIO_BOUND, offs[0], offs32[0], f"{name} b={offs[1]} l={offs[2]}")
        for keys, bound, measure in ((s4conv.READOUT_KEYS, s4conv.READOUT_BOUND, "D / fc_t"),
                                     (s4conv.SPECTRUM_KEYS, s4conv.SPECTRUM_BOUND, "kernel / norm1")):
            for k in keys:
                if k in grads:
                    note(measure, bound, s4conv.tensor_error(full[name][1][k], grads[k]),
                         s4conv.tensor_error(grads32[k], grads[k]), f"{name} {k[len(s4conv.BLOCK) + 1:]}")
    print(f"S4ADJ H={H} B={B} L={L} {path}{' (taps as constants)' if k_tap is not None else ''}, launches {counts}: "
          + " | ".join(f"{m}: engine {e:.2e} ({w}), fp32 oracle {worst_or[m]:.2e}, ratio {e / max(worst_or[m], 1e-300):.1f}"
                       for m, (e, w) in worst.items()))
    assert not failures, "\n".join(failures)
    if k_tap is None:
        for name in s4conv.COTANGENTS:
            one = lambda g: {s4conv.LOG_DT: g[s4conv.LOG_DT]}
            truth = one(refs["ref"][name][1])
            gradcheck.compare(one(full[name][1]), truth, truth, fp32_impls=(one(refs["oracle32"][name][1]),),
                              label=f"S4ADJ H={H} B={B} L={L} {name}", max_widened=1, families=("kernel.log_dt",))


# 1. every plan at its edges (the forward test's list): both fftcorr kernels, RSUM and launch_rowsum_bc, the zero-padded tail
# inside the conjugate product
@pytest.mark.parametrize("L", PLAN_EDGES)
def test_adjoint_at_the_edges_of_every_plan(gpu, L):
    assert PLAN_EDGES == s4conv.ADJOINT_PLAN_EDGES
    _check_case(gpu, 8, 2, L, FUSED)


# 2. the batch-chunk loop of fftcorr: H = 64 gives nbs = 8 partial spectra; B = 9: chunks of 2 and a last chunk of 1, B = 17:
# chunks of 3 and a last chunk of 2.  (64, 9, 16384): the instance that parks the bins of U in its output slab.
@pytest.mark.parametrize("H,B,L", s4conv.ADJOINT_CASES["batch_chunks"])
def test_fftcorr_walks_more_than_one_sample(gpu, H, B, L):
    bchunk, last = s4conv.fftcorr_chunks(B, H)
    assert bchunk > 1 and last < bchunk, (bchunk, last)
    _check_case(gpu, H, B, L, FUSED)


# 3. rows the fused kernels refuse: rocfft_conv_backward, launch_conv_adjoint_spec / _epi, launch_s4_twosided_bwd
@pytest.mark.parametrize("H,B,L", s4conv.ADJOINT_CASES["rocfft"])
def test_rocfft_adjoint(gpu, H, B, L):
    _check_case(gpu, H, B, L, ROCFFT)


# 4. 18 rows: not a multiple of the 8 XCDs `RowSchedule` deals rows over (the adjoint pass goes through the same schedule)
@pytest.mark.parametrize("H,B,L", s4conv.ADJOINT_CASES["row_counts"])
def test_adjoint_with_a_row_count_that_is_no_multiple_of_eight(gpu, H, B, L):
    _check_case(gpu, H, B, L, FUSED)

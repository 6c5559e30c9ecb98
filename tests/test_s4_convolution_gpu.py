"""Function-level GPU parity of the S4 long convolution (`S4.forward`, `s4.py:1376-1437`) at
every transform plan of `fftconv_kernels.hip` / `fft_core.h`, on the segmented kernel and on the rocFFT fallback.

A one-block network whose tail is transparent (tests/s4conv.py: FF = 0, output_linear = [I; 0] with the GLU gate held at
sigmoid(30) = 1.0f) puts the S4 branch on the tap `out:c_layers.0`:  out - 2x = GELU(conv(u, k) + D u).  The reference is
that expression in float64 on the host, with the engine's own taps (`k:c_layers.0`), so the comparison judges the
convolution and not the kernel generator (which has its own test below).  The kernels get long memory
(dt = linspace(0.5, 4, H) / l_max): every case asserts that at least half of its 2H kernels still hold 1 % of their peak
at the last tap and that the convolution term weighs at least half of D u, i.e. that a misplaced anti-causal half,
circular aliasing, a wrong truncation or a wrong neighbour segment would move the output by far more than the bound.

  case group                                       what of a14 it pins down
  plan edges (M = 1024 .. 16384, L = M, M - 2,     even plans with the direct top pass (log2 M = 10, 12, 14), odd plans staged
  smallest L of the plan, L = 2 mod 4)             through LDS (11, 13), fused radix-4 tail (10, 14), zero padding, row alignment
  truncated / clamped taps                         `L_kernel = min(L, l_max)` (`s4.py:1387`)
  segmented rows (16386 .. 40000)                  `fftconv_seg_kernel`: neighbour segments, a 2-sample last segment
  rocFFT dispatch (14, 125, 1025)                  the n = 2L product path of rows the fused kernel refuses
  row-count edges (18 rows; > 2 rows per slot)     `RowSchedule` over 8 XCDs, a workgroup walking a second and third row
  forward_train == forward                         the training forward runs the same convolution
  kernel generator                                 the taps themselves in the long-memory regime, against the oracle

Error measure: per (b, h) row max_l |got - ref| / max_l |ref|, worst row; bound 2e-5, the bound of the same tap and the
same `out - 2x` subtraction in `test_ff_branch_matches_the_oracle`.  Every case also prints the fp32 CPU oracle's error
(`oracle.sashimi.diffwave_block` through the same isolation, against the same float64 expression on the oracle's own
taps) and the ratio of the two.

Measured on an MI355X (256 CUs), precision "f32", over the 32 convolution cases: largest engine error 6.90e-6 (H = 64,
B = 17, L = 8192; 6.85e-6 at H = 64, B = 9, L = 16384), 1.2e-6 .. 3.5e-6 on every H = 8 / H = 6 case -- fused, segmented
and rocFFT alike, no dependence on the plan; largest fp32-oracle error 8.82e-6 (the same H = 64 case; 8.47e-6 at l_max
1024 on a 4096-sample row); largest engine / oracle ratio 2.4 (l_max = 4096 on a 1000-sample row: 1.90e-6 against
7.87e-7), so no case needs an explanation and none comes near the bound.  Both errors have the same floor: the tap holds
2x + s in fp32 (|2x + s| < 16, two roundings, 1e-6 absolute) and the worst row's largest |s| is 0.1.  forward_train
against forward: 1.1e-7 .. 1.7e-7 on the tap.  Kernel generator: 1.7e-6 .. 2.8e-6 of a row's largest tap.
"""
import ctypes
import math

import pytest
import torch

from diffwave_sashimi_amd import _lib
from oracle import sashimi as oss
from tests import cases, s4conv
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

BOUND = 2e-5
TAP = "out:" + s4conv.BLOCK
FUSED, SEGMENTED, ROCFFT = "fused", "segmented", "rocfft"


def _counted_forward(net, gpu, audio, steps, name):
    """One sampling forward with the launch profile on for `name`: (tap, launches whose name contains `name`)."""
    lib = _lib.load()
    B, L, H = audio.shape[0], audio.shape[-1], net.d_model
    _lib.check(lib.dws_profile_enable(name))
    try:
        with torch.no_grad():
            net((audio.to(gpu), steps.to(gpu)))
        torch.cuda.synchronize()
        n, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
        _lib.check(lib.dws_profile_query(ctypes.byref(n), ctypes.byref(ms)))
    finally:
        lib.dws_profile_disable()
    return net.read_tap(TAP, (B, H, L)).cpu(), int(n.value)


def _path_of(net, gpu, audio, steps):
    """(tap of the first run, tap of the second run, which convolution ran).  "fftconv" also matches "fftconv_seg"."""
    tap1, n_seg = _counted_forward(net, gpu, audio, steps, b"fftconv_seg")
    tap2, n_all = _counted_forward(net, gpu, audio, steps, b"fftconv")
    n_fused = n_all - n_seg
    assert (n_fused, n_seg) in ((1, 0), (0, 1), (0, 0)), (n_fused, n_seg)
    return tap1, tap2, FUSED if n_fused else SEGMENTED if n_seg else ROCFFT


def _check_case(gpu, H, B, Lcfg, L, path, weight_seed=s4conv.WEIGHT_SEED):
    cfg, net = s4conv.build_isolated_block(H, Lcfg, weight_seed)
    net = net.to(gpu)
    net.invalidate()
    assert s4conv.tail_is_transparent(net.state_dict(), H)          # read back from the device
    audio, steps = cases.wavenet_inputs(B, L, 1, s4conv.INPUT_SEED)
    tap, tap_again, ran = _path_of(net, gpu, audio, steps)
    assert ran == path, f"expected the {path} convolution, the {ran} one ran"
    assert torch.equal(tap, tap_again)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    assert int(sd[s4conv.BLOCK + ".layer.kernel.kernel.L"]) == Lcfg
    r = s4conv.reference(sd, cfg, audio, steps, net.read_tap("k:" + s4conv.BLOCK, (2, H, Lcfg)))
    Lt = min(L, Lcfg)
    assert r["k0"].shape == (H, Lt)
    # not vacuous: the far taps and the convolution term carry weight (float64 data)
    far, weight = s4conv.far_tap_kernels(r["k0"], r["k1"]), s4conv.rms(r["conv"]) / s4conv.rms(r["du"])
    assert far >= H, f"only {far} of {2 * H} kernels hold 1 % of their peak at tap {Lt - 1}"
    assert weight >= 0.5, f"conv term RMS is {weight:.2f} x the RMS of D u"
    errs = s4conv.row_errors(tap.double() - 2.0 * r["x"], r["ref"])
    err = float(errs.max())
    # the fp32 oracle on the same inputs, against the same float64 expression on ITS taps (the convolution alone, too)
    with torch.no_grad():
        k_or = oss.ss_kernel_nplr(sd, s4conv.BLOCK + ".layer.kernel.kernel", Lt).double()       # what `s4_forward` uses
        ref_or = s4conv.s4_branch(r["u"], k_or[0], k_or[1], sd[s4conv.BLOCK + ".layer.D"].double())[0]
    err_or = float(s4conv.row_errors(s4conv.oracle_fp32_branch(sd, cfg, audio, steps, r["x"]), ref_or).max())
    b, h = divmod(int(errs.argmax()), H)
    pos = int((tap[b, h].double() - 2.0 * r["x"][b, h] - r["ref"][b, h]).abs().argmax())
    print(f"S4CONV H={H} B={B} l_max={Lcfg} L={L} {ran}: engine {err:.2e} (row b={b} h={h}, position {pos}) | fp32 oracle "
          f"{err_or:.2e} | ratio {err / err_or:.1f} | far taps {far}/{2 * H}, conv/Du {weight:.2f}")
    assert err < BOUND, (err, b, h, pos)
    return net, audio, steps, tap


# 1. every plan at its edges: the smallest L of the plan, M - 2 and M (L = 2 mod 4: rows alternate 16-byte alignment)
PLAN_EDGES = [16, 18, 250, 1022, 1024,          # M = 1024 (padded below 512)
              1026, 2046, 2048,                 # M = 2048, odd plan
              2050, 4094, 4096,                 # M = 4096
              4098, 8190, 8192,                 # M = 8192, odd plan, persistent row schedule
              8194, 16382, 16384]               # M = 16384


@pytest.mark.parametrize("L", PLAN_EDGES)
def test_convolution_at_the_edges_of_every_plan(gpu, L):
    _check_case(gpu, 8, 2, L, L, FUSED)


# 2. (l_max, input length, weight seed).  The first runs Lt = 1000 of 4096 taps at M = 1024: a quarter of the kernels'
# memory lies on the row, and with weight seed 5 the convolution term is 0.31 x D u on the float64 reference alone (D is a
# seeded N(0, 1) draw of 8 values); seed 6 is the next seed at which the weight condition holds (0.84).
@pytest.mark.parametrize("Lcfg,L,weight_seed", [(4096, 1000, 6), (1024, 4096, s4conv.WEIGHT_SEED)])
def test_truncated_and_clamped_taps(gpu, Lcfg, L, weight_seed):
    _check_case(gpu, 8, 2, Lcfg, L, FUSED, weight_seed)


# 3. rows beyond one 16384-sample transform: a second segment of 2 samples, exactly two segments, two and a bit, 40000
@pytest.mark.parametrize("B,L", [(1, 16386), (1, 32768), (1, 32770), (1, 40000), (2, 32768)])
def test_segmented_rows(gpu, B, L):
    _check_case(gpu, 8, B, 16384, L, SEGMENTED)


# 4. rows the fused kernel refuses (below 16 samples, odd): the rocFFT n = 2L product path, zero fftconv launches
@pytest.mark.parametrize("L", [14, 125, 1025])
def test_rocfft_dispatch(gpu, L):
    _check_case(gpu, 8, 2, L, L, ROCFFT)


# 5a. 18 rows: not a multiple of the 8 XCDs `RowSchedule` deals rows over
@pytest.mark.parametrize("L", [1024, 8192, 16384])
def test_row_count_that_is_no_multiple_of_eight(gpu, L):
    _check_case(gpu, 6, 3, L, L, FUSED)


# 5b. more rows than twice the resident workgroups.  `launch_fc` starts min(rows, slots) workgroups for log2 M >= 13, with
# slots = CUs x min(160 KiB / LDS, 2048 / threads), LDS = (M + M/16) x 8 bytes and M/16 threads: M = 8192 -> 69632 bytes,
# 512 threads, 2 per CU; M = 16384 -> 139264 bytes, 1024 threads, 1 per CU.  rows > 2 x slots: some workgroup walks three.
@pytest.mark.parametrize("L,per_cu", [(8192, 2), (16384, 1)])
def test_persistent_schedule_walks_three_rows(gpu, L, per_cu):
    H = 64
    slots = per_cu * torch.cuda.get_device_properties(gpu).multi_processor_count
    B = 2 * slots // H + 1                      # 17 and 9 on a 256-CU part
    assert B * H > 2 * slots
    net, audio, steps, tap = _check_case(gpu, H, B, L, L, FUSED)    # (also: a second run of the batch is bit-equal)
    with torch.no_grad():
        net((audio[:1].to(gpu), steps[:1].to(gpu)))
    alone = net.read_tap(TAP, (1, H, L)).cpu()
    assert torch.equal(alone[0], tap[0])        # a row does not depend on which workgroup walked it, or after which row


# 6. the training forward runs the same convolution as the sampling forward
@pytest.mark.parametrize("L", [1024, 2048, 4096, 8192, 16384])
def test_forward_train_is_the_sampling_forward(gpu, L):
    H, B = 8, 2
    cfg, net = s4conv.build_isolated_block(H, L)
    net = net.to(gpu)
    net.invalidate()
    audio, steps = cases.wavenet_inputs(B, L, 1, s4conv.INPUT_SEED)
    net.train()
    with torch.enable_grad():
        eps_t = net((audio.to(gpu), steps.to(gpu)))
    assert eps_t.requires_grad                                     # the differentiable path ran (forward_train)
    tap_t = net.read_tap(TAP, (B, H, L)).cpu()
    net.eval()
    with torch.no_grad():
        eps_e = net((audio.to(gpu), steps.to(gpu)))
    tap_e = net.read_tap(TAP, (B, H, L)).cpu()
    e_tap, e_eps = rel_err(tap_t, tap_e), rel_err(eps_t.detach(), eps_e)
    print(f"S4TRAIN L={L}: forward_train vs forward: tap {e_tap:.2e}, eps {e_eps:.2e}")
    assert float(tap_e.abs().max()) > 1.0
    assert e_tap < 1e-6          # (forward_train fills the tap; eps, printed above, also passes the tails' other GEMM kernels)


# 7. the taps themselves in the long-memory regime (no fixture covers it): per (direction, channel) row against the oracle
# on the float64 state dict, 1e-4 of the row's largest tap as in `test_s4_kernel_generator_matches_reference`
@pytest.mark.parametrize("L", [250, 2048, 8192, 16384])
def test_kernel_generator_with_long_memory(gpu, L):
    H = 8
    cfg, net = s4conv.build_isolated_block(H, L)
    net = net.to(gpu)
    net.invalidate()
    audio, steps = cases.wavenet_inputs(1, L, 1, s4conv.INPUT_SEED)
    with torch.no_grad():
        net((audio.to(gpu), steps.to(gpu)))
    got = net.read_tap("k:" + s4conv.BLOCK, (2, H, L)).cpu().double() / L
    sd64 = s4conv.to_float64(net.state_dict())
    with torch.no_grad():
        ref = oss.ss_kernel_nplr(sd64, s4conv.BLOCK + ".layer.kernel.kernel", L)
    assert ref.dtype == torch.float64 and ref.shape == got.shape
    errs = (got - ref).abs().amax(-1) / ref.abs().amax(-1)
    far = s4conv.far_tap_kernels(ref[0], ref[1])
    print(f"S4KERNEL L={L}: worst row {float(errs.max()):.2e} of its largest tap; far taps {far}/{2 * H}")
    assert far >= H
    assert float(errs.max()) < 1e-4, errs
    assert math.isfinite(float(got.abs().max()))

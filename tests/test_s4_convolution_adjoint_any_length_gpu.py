"""Function-level GPU parity of the ADJOINT of the S4 long convolution at l_max != L: what an `audio.grad` of an eval()
module and every step of a guided run execute when the run is shorter or longer than the kernels, or longer than one
in-LDS transform (`dws_model_forward_input` + the data-only `dws_model_backward_input`).

The one-block network of tests/s4conv.py with both ReLUs held open, the kernels set up for l_max, run at L, against torch
autograd through the CPU oracle in FLOAT64 on the engine's own `k:` taps (`s4conv.adjoint_reference`; its reference side,
the segment identity and two wrong adjoints are checked in tests/test_s4_convolution_adjoint_any_length_reference.py).
Three cotangents per case (dense, head, tail), eval() mode: the backward is data-only and no parameter gets a gradient.

  measure                                                                          bound
  audio.grad: per batch row max_l |got - ref| / max_l |ref_branch|, worst row      2e-5   (`s4conv.AUDIO_BOUND`)
  audio.grad off the support: per row max |got - ref| / max |ref| over l not in S  2e-5

  stage type   (H, B, l_max, L)                       forward              backward               launches asserted
  fused        (8, 2, 4096, 1000)  truncated taps     fftconv + pre        fftconv conj_k/no_act  fftconv 1 + 1
               (8, 2, 1024, 4096)  clamped taps
  segmented    (8, 1, 16384, 16386) 2-sample segment  fftconv_seg_train    fftconv_seg_adjoint    fftconv_seg 1 + 1
               (8, 2, 16384, 32768) two segments
               (8, 1, 16384, 40000) two and a bit
  rocFFT       the 16386 and 32768 cases under DWS_SASHIMI_ROCFFT=1 (a child process each: the variable is read at model
               setup): long_stage_fwd 1, long_stage_bwd 1, no fftconv
  `fftcorr` (the kernel-parameter gradient) runs in none of them.

On the segmented cases the training instance's forward is also held bit-equal to the sampling call's on the same inputs
(the block's output tap and eps; the sampling call with its LayerNorm epilogues off, so that both paths feed the
convolution the same u): the same arithmetic with one more store.

Measured on an MI355X (256 CUs), precision "f32": audio.grad over all positions at most 4.14e-6 (L = 32768 segmented, tail
cotangent; the fp32 CPU oracle 2.96e-6 there, at most 3.22e-6 over the cases), off the support at most 1.42e-6 (oracle
1.17e-6); the rocFFT repeats 3.56e-6 and 1.02e-6; no dependence on the route.

Every case raises NotImplementedError before `dws_model_forward_input` existed."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from diffwave_sashimi_amd import _lib
from tests import s4conv
from tests import s4conv_any_length as anyl

pytestmark = pytest.mark.gpu

FUSED, SEGMENTED, ROCFFT = "fused", "segmented", "rocfft"
COUNTED = (b"fftconv", b"fftconv_seg", b"long_stage_fwd", b"long_stage_bwd", b"fftcorr")
# launches of (forward, backward) whose name contains each of COUNTED ("fftconv" also matches "fftconv_seg...")
EXPECTED = {FUSED: ((1, 0, 0, 0, 0), (1, 0, 0, 0, 0)),
            SEGMENTED: ((1, 1, 0, 0, 0), (1, 1, 0, 0, 0)),
            ROCFFT: ((0, 0, 1, 0, 0), (0, 0, 0, 1, 0))}
IDS = lambda c: "H%d-B%d-lmax%d-L%d-seed%d" % c


def _counted(fn, name):
    lib = _lib.load()
    _lib.check(lib.dws_profile_enable(name))
    try:
        out = fn()
        torch.cuda.synchronize()
        n, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
        _lib.check(lib.dws_profile_query(ctypes.byref(n), ctypes.byref(ms)))
    finally:
        lib.dws_profile_disable()
    return out, int(n.value)


def _pair(net, gpu, audio, steps, cot, name):
    """One eval()-mode forward / backward of (eps * cot).sum(), the launches containing `name` counted in each:
    (audio.grad, eps, forward launches, backward launches)."""
    a = audio.to(gpu).requires_grad_(True)
    eps, nf = _counted(lambda: net((a, steps.to(gpu))), name)
    _, nb = _counted(lambda: eps.backward(cot.to(gpu)), name)
    assert all(p.grad is None for p in net.parameters())           # the backward was data-only
    return a.grad.detach().cpu(), eps.detach(), nf, nb


def _check_case(gpu, case, path):
    H, B, l_max, L, seed = case
    cfg, net, audio, steps, cots, minima = anyl.prepare_case(*case)
    assert min(minima) >= 0.25
    net = net.to(gpu).eval()
    net.invalidate()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    assert s4conv.tail_is_transparent(sd, H) and int(sd[s4conv.KERNEL + "L"]) == l_max != L
    got, eps = {}, None
    fwd, bwd = [], []
    for i, count in enumerate(COUNTED):           # five pairs: each cotangent at least once, every counter once
        name = s4conv.COTANGENTS[i % 3]
        g, eps, nf, nb = _pair(net, gpu, audio, steps, cots[name], count)
        assert name not in got or torch.equal(got[name], g)
        got[name] = g
        fwd.append(nf), bwd.append(nb)
    assert (tuple(fwd), tuple(bwd)) == EXPECTED[path], f"expected the {path} pair, launches {COUNTED}: {fwd} / {bwd}"
    if path == SEGMENTED:      # the training instance's forward is the sampling instance's arithmetic
        tap_train = net.read_tap("out:" + s4conv.BLOCK, (B, H, L))
        os.environ["DWS_SASHIMI_NO_LN_FUSION"] = "1"        # (read per call: the separate LayerNorm launch the training forward runs)
        try:
            with torch.no_grad():
                eps_sample, n_seg = _counted(lambda: net((audio.to(gpu), steps.to(gpu))), b"fftconv_seg")
        finally:
            del os.environ["DWS_SASHIMI_NO_LN_FUSION"]
        assert n_seg == 1
        assert torch.equal(net.read_tap("out:" + s4conv.BLOCK, (B, H, L)), tap_train)
        assert torch.equal(eps_sample, eps)
    k_tap = net.read_tap("k:" + s4conv.BLOCK, (2, H, l_max)).cpu()
    refs = s4conv.host_references(sd, cfg, audio, steps, cots, k_tap)
    failures, report = [], []
    for name in s4conv.COTANGENTS:
        da, da32 = refs["ref"][name][0], refs["oracle32"][name][0]
        off = s4conv.off_support(name, L)
        assert got[name].shape == (B, 1, L) and torch.isfinite(got[name]).all()
        every, offs = s4conv.audio_errors(got[name], da, refs["branch"][name], off)
        every32, offs32 = s4conv.audio_errors(da32, da, refs["branch"][name], off)
        report.append(f"{name}: audio {every[0]:.2e} (b={every[1]} l={every[2]}; fp32 oracle {every32[0]:.2e})"
                      + ("" if offs is None else f", off support {offs[0]:.2e} (l={offs[2]}; oracle {offs32[0]:.2e})"))
        for what, e in (("audio", every), ("off support", offs)):
            if e is not None and not e[0] < s4conv.AUDIO_BOUND:
                failures.append(f"{what} {name} b={e[1]} l={e[2]}: {e[0]:.2e} >= {s4conv.AUDIO_BOUND:g}")
    print(f"S4ADJ-ANY H={H} B={B} l_max={l_max} L={L} {path}, launches {fwd} / {bwd}: " + " | ".join(report))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", anyl.FUSED_CASES, ids=IDS)
def test_fused_adjoint_with_truncated_and_clamped_taps(gpu, case):
    _check_case(gpu, case, FUSED)


@pytest.mark.parametrize("case", anyl.SEGMENTED_CASES, ids=IDS)
def test_segmented_adjoint(gpu, case):
    _check_case(gpu, case, SEGMENTED)


@pytest.mark.parametrize("case", anyl.ROCFFT_CASES, ids=IDS)
def test_rocfft_adjoint_beyond_the_kernels_length(gpu, case):
    """DWS_SASHIMI_ROCFFT=1 is read when the model is set up: a fresh child process per case runs `_check_case`."""
    code = ("import torch; from tests import conftest, test_s4_convolution_adjoint_any_length_gpu as t; "
            "conftest._fit_cpu_threads_to_the_quota(); "
            f"t._check_case(torch.device('cuda:0'), {tuple(case)!r}, t.ROCFFT)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    proc = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, DWS_SASHIMI_ROCFFT="1"),
                          capture_output=True, text=True, timeout=300)
    print(proc.stdout[-2000:])
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    assert "S4ADJ-ANY" in proc.stdout and "rocfft" in proc.stdout

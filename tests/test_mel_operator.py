"""CPU: the float64 restatement of the mel front-end (tests/mel_reference.py) against torch autograd through the oracle's
own formulation (`oracle.mel.mel_spectrogram`: conv1d with the windowed Fourier basis, float32) on non-silent inputs;
`sampling.mel_operator`'s argument validation; and the `generate.guide_op=mel` / `generate.report_mel` key checks, which
run before any GPU work.

Bound of the float32-against-float64 comparison: 2 N eps32 of the largest entry -- a length-N float32 dot product is
within N eps32 of the exact one in the worst case, and the gradient passes through two of them (the DFT and its
adjoint).  7.6e-6 at N = 64, 3.1e-5 at N = 256, 1.2e-4 at N = 1024; float32 autograd through the oracle was measured at
7e-7 .. 2.5e-5 of float64 on these shapes."""
import numpy as np
import pytest
import torch

from oracle import mel as omel
from tests import cases
from tests import mel_reference as mref
from tests.conftest import rel_err

EPS32 = float(np.finfo(np.float32).eps)
WN = cases.wn_cfg(res_channels=64, skip_channels=64, num_res_layers=3, dilation_cycle=3)


def _tables(case):
    from diffwave_sashimi_amd.mel import mel_filterbank, padded_hann
    n_fft, hop, win, T, bands, sr = case
    return (torch.from_numpy(padded_hann(win, n_fft)),
            torch.from_numpy(mel_filterbank(sr, n_fft, bands, 0.0, min(8000.0, sr / 2.0))))


@pytest.mark.parametrize("case", mref.CASES, ids=lambda c: "n%d_h%d_w%d_T%d" % c[:4])
def test_float64_helper_agrees_with_autograd_through_the_oracle(case):
    n_fft, hop, win, T, bands, sr = case
    window, basis = _tables(case)
    x, g = mref.case_inputs(case)
    ref = mref.mel_spectrogram(x, window, basis, n_fft, hop)
    assert ref.shape == (3, bands, T // hop + 1) and ref.dtype == torch.float64
    smallest = float(mref.mel_energies(x.double(), window, basis, n_fft, hop).min())
    assert smallest >= 5 * mref.CLIP, smallest                # non-silent: no clamp decision near its edge
    xin = x.clone().requires_grad_(True)
    out = omel.mel_spectrogram(xin, basis, n_fft, hop, win)
    (dx,) = torch.autograd.grad((out * g).sum(), xin)
    dref = mref.mel_gradient(x, g, window, basis, n_fft, hop)
    tol = 2 * n_fft * EPS32
    fwd, bwd = float((out.detach().double() - ref).abs().max()), rel_err(dx, dref)
    print(f"{case}: oracle (float32) vs helper (float64): log-mel {fwd:.2e}, gradient {bwd:.2e} (bound {tol:.2e}); "
          f"smallest mel energy {smallest / mref.CLIP:.1f} x clip")
    assert torch.isfinite(dref).all()
    assert fwd <= tol        # a relative error of the energy is an absolute one of its log
    assert bwd <= tol


def test_float64_helper_gives_zero_where_autograd_gives_nan():
    """400 random samples then 600 zeros: plain autograd through the oracle is NaN on every sample a silent frame
    touches; the helper is finite everywhere and exactly 0 on samples that only silent frames reach."""
    case = (256, 64, 256, 1000, 80, 16000)
    window, basis = _tables(case)
    x, g = mref.case_inputs(case, B=1)
    x[:, 400:] = 0
    xin = x.clone().requires_grad_(True)
    (dx,) = torch.autograd.grad((omel.mel_spectrogram(xin, basis, 256, 64, 256) * g).sum(), xin)
    assert torch.isnan(dx).any()
    dref = mref.mel_gradient(x, g, window, basis, 256, 64)
    assert torch.isfinite(dref).all()
    # frame f covers samples f 64 - 128 .. f 64 + 127: frame 8 (384 .. 639) is the last one that sees a non-zero sample
    assert float(dref[:, 640:].abs().max()) == 0 and float(dref[:, :400].abs().min()) > 0


def test_mel_operator_validates_its_arguments_and_refuses_cpu_tensors():
    from diffwave_sashimi_amd.mel import TacotronSTFT
    from diffwave_sashimi_amd.sampling import mel_operator
    kw = dict(filter_length=64, hop_length=16, win_length=64, n_mel_channels=20, sampling_rate=16000, mel_fmax=8000.0)
    st = TacotronSTFT(**kw)
    for A in (mel_operator(st), mel_operator(**kw)):
        assert callable(A) and A.stft.filter_length == 64 and A.stft.n_mel_channels == 20
    assert mel_operator(st).stft is st
    with pytest.raises(ValueError, match="not both"):
        mel_operator(st, hop_length=16)
    for bad in (3, dict(kw)):
        with pytest.raises(ValueError, match="TacotronSTFT"):
            mel_operator(bad)
    with pytest.raises(TypeError):
        mel_operator(bogus=1)
    A = mel_operator(st)
    for shape in ((2, 1, 100), (2, 100)):
        with pytest.raises(RuntimeError, match="GPU only|no CPU fallback"):
            A(torch.zeros(shape))
    with pytest.raises(ValueError, match="expected"):
        A(torch.zeros(2, 2, 100))
    with pytest.raises(ValueError, match="expected"):
        A(torch.zeros(100))
    x = torch.zeros(1, 100, requires_grad=True)
    with pytest.raises(RuntimeError, match="GPU only|no CPU fallback"):
        st.mel_spectrogram(x)


def test_generate_cli_checks_the_mel_guide_keys_before_any_gpu_work(tmp_path):
    from diffwave_sashimi_amd.generate import generate
    diff = dict(T=5, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="sc09", segment_length=640, sampling_rate=16000, data_path=str(tmp_path))
    call = lambda **kw: generate(0, diff, dict(WN), ds, ckpt_iter="init", n_samples=1, exp_root=str(tmp_path / "exp"), **kw)
    # with a recording
    with pytest.raises(ValueError, match="guide_scale"):
        call(guide_name="y", guide_op="mel")
    with pytest.raises(ValueError, match="guide_scale"):
        call(guide_name="y", guide_op="mel", guide_scale=0)
    with pytest.raises(ValueError, match="guide_clip belongs to generate.guide_op=declip"):
        call(guide_name="y", guide_op="mel", guide_scale=0.5, guide_clip=0.3)
    with pytest.raises(ValueError, match="guide_factor belongs to generate.guide_op=lowpass"):
        call(guide_name="y", guide_op="mel", guide_scale=0.5, guide_factor=2)
    with pytest.raises(ValueError, match="ddpm and ddim"):
        call(guide_name="y", guide_op="mel", guide_scale=0.5, sampler="dpmpp2m", steps=4)
    with pytest.raises(ValueError, match="editing"):
        call(guide_name="y", guide_op="mel", guide_scale=0.5, known_name="k", keep=[[0, 10]])
    with pytest.raises(ValueError, match="expected declip, lowpass or mel"):
        call(guide_name="y", guide_op="stft", guide_scale=0.5)
    # without one: only a mel-conditional run has a mel to be kept on
    with pytest.raises(ValueError, match=r"generate\.guide_op needs generate\.guide_name \(the degraded recording\)"):
        call(guide_op="mel", guide_scale=0.5)
    with pytest.raises(ValueError, match="guide_op=mel needs generate.guide_scale"):
        call(guide_op="mel", mel_name="m")
    with pytest.raises(ValueError, match="guide_clip"):
        call(guide_op="mel", mel_name="m", guide_scale=0.5, guide_clip=0.3)
    with pytest.raises(ValueError, match="guide_factor"):
        call(guide_op="mel", mel_name="m", guide_scale=0.5, guide_factor=2)
    with pytest.raises(ValueError, match="ddpm and ddim"):
        call(guide_op="mel", mel_name="m", guide_scale=0.5, sampler="aligned")
    with pytest.raises(ValueError, match="needs generate.guide_name"):        # the other operators still need a recording
        call(guide_op="declip", mel_name="m", guide_scale=0.5)
    # report_mel
    with pytest.raises(ValueError, match="report_mel needs a mel-conditional run"):
        call(report_mel=True)
    with pytest.raises(ValueError, match="report_mel"):
        call(report_mel="yes", mel_name="m")

"""GPU: `sampling.sampling_guided` on a SaShiMi model at run lengths other than its kernels' own -- every step a
`dws_model_forward_input` and a data-only `dws_model_backward_input` -- against the float64 loop through the CPU oracle
(tests/guided_reference.py) on the same weights, x_T and noise: <= REL_TOL = 1e-3 of max|x|.

The `SS` model of tests/test_guided_sampling_gpu.py (d32, L = 1024, pool [4, 4]) at 512 (truncated taps), 2048 (clamped
taps) and 1008 (stages 1008 / 252 / 63: the last on rocFFT); operators declip and lowpass, samplers DDIM (6 of 50 steps,
eta 0) and the 6-step DDPM schedule, scale 0.5; f32 everywhere, bf16x6 at 2048.  On the float64 reference the guidance
moves the result by 1.6e-2 .. 9.2e-2 over the twelve combinations (> 10 REL_TOL is asserted), and the same loop in fp32
lies <= 3.6e-5 from it.

`generate` end to end: a mel-conditional SaShiMi checkpoint with `dataset.segment_length = 1024` vocodes an utterance of
6 frames (1536 samples) under `generate.guide_op=mel` with `report_mel`.

Every run here raised NotImplementedError before `dws_model_forward_input` existed."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.conftest import REL_TOL, rel_err
from tests.guided_reference import oracle_net, reference_guided
from tests.test_guided_sampling_gpu import BETA6, SAMPLERS, SS_COND, _engine, _model, _schedule
from tests.test_mel_guided_gpu import _checkpoint

pytestmark = pytest.mark.gpu

LENGTHS = (512, 2048, 1008)
SAMPLER_KEYS = ("ddim_eta0", "ddpm6")
SCALE = 0.5
RUNS = ([(L, op, s, "f32") for L in LENGTHS for op in ("declip", "lowpass") for s in SAMPLER_KEYS]
        + [(2048, op, s, "bf16x6") for op in ("declip", "lowpass") for s in SAMPLER_KEYS])


def _problem(L, op_name, S=6):
    from diffwave_sashimi_amd.sampling import declip_operator, lowpass_operator
    cfg, B, Lcfg, wseed, sd = _model("sashimi")
    assert L != Lcfg == 1024
    g = torch.Generator().manual_seed(41)
    clean = torch.randn(B, 1, L, generator=g) * 0.3
    x_T = torch.randn(B, 1, L, generator=g)
    noise = torch.randn(S, B, 1, L, generator=g)
    op = declip_operator(0.2) if op_name == "declip" else lowpass_operator(2)
    return cfg, B, sd, op, op(clean), x_T, noise


def _reference(L, op_name, sampler_key):
    """Float64 guided run and the unguided one, once per (length, operator, sampler)."""
    def make():
        cfg, B, sd, op, y, x_T, noise = _problem(L, op_name)
        sampler, eta = SAMPLERS[sampler_key]
        dh, steps = _schedule(sampler)
        net64 = oracle_net(cfg, sd, torch.float64)
        run = lambda scale: reference_guided(net64, (B, 1, L), dh, y=y, operator=op, scale=scale, sampler=sampler,
                                             steps=steps, eta=eta, x_T=x_T, noise=noise)
        return run(SCALE), run(0.0)
    return cases.cached(("guided_any_length_reference", L, op_name, sampler_key), make)


@pytest.mark.parametrize("L,op_name,sampler_key,precision", RUNS)
def test_guided_run_at_another_length_matches_the_float64_oracle_loop(gpu, L, op_name, sampler_key, precision):
    from diffwave_sashimi_amd.sampling import sampling_guided
    cfg, B, sd, op, y, x_T, noise = _problem(L, op_name)
    sampler, eta = SAMPLERS[sampler_key]
    dh, steps = _schedule(sampler)
    ref, plain = _reference(L, op_name, sampler_key)
    net = _engine("sashimi", gpu, precision)
    got = sampling_guided(net, (B, 1, L), dh, measurement=y.to(gpu), operator=op, scale=SCALE, sampler=sampler, steps=steps,
                          eta=eta, x_T=x_T.to(gpu), noise=noise.to(gpu))
    assert got.device.type == "cuda" and got.shape == (B, 1, L) and torch.isfinite(got).all()
    err, moved = rel_err(got.cpu(), ref), rel_err(plain, ref)
    print(f"sashimi L={L} (kernels 1024) {op_name} {sampler_key} {precision}: engine vs float64 loop {err:.2e} "
          f"(guidance moves the result by {moved:.2e})")
    assert err <= REL_TOL
    assert moved > 10 * REL_TOL          # the bound tells a guided run from an unguided one
    assert all(p.grad is None for p in net.parameters())


def test_guided_run_in_train_mode_names_what_is_built(gpu):
    from diffwave_sashimi_amd.sampling import sampling_guided
    cfg, B, sd, op, y, x_T, noise = _problem(512, "declip")
    dh, steps = _schedule("ddim")
    net = _engine("sashimi", gpu).train()
    with pytest.raises(NotImplementedError, match="eval\\(\\) mode"):
        sampling_guided(net, (B, 1, 512), dh, measurement=y.to(gpu), operator=op, scale=SCALE, sampler="ddim", steps=steps,
                        x_T=x_T.to(gpu), noise=noise.to(gpu))


def test_generate_cli_holds_a_sashimi_vocoder_on_a_mel_of_another_length(tmp_path, gpu, capsys):
    """checkpoint (segment_length 1024) -> utterance of 6 frames -> generate.guide_op=mel + report_mel -> 1536-sample wavs."""
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import generate
    cfg = dict(SS_COND)
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=BETA6)
    data = tmp_path / "wavs"
    os.makedirs(data)
    wav = (np.random.default_rng(3).standard_normal(1500) * 0.3 * 32767).clip(-32767, 32767).astype(np.int16)
    wavfile.write(str(data / "LJ001-0001.wav"), 22050, wav)            # 1500 samples -> 6 frames -> L = 1536
    ds = dict(_name_="ljspeech", data_path=str(data), segment_length=1024, sampling_rate=22050, filter_length=1024,
              hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0)
    root = str(tmp_path / "exp")
    _checkpoint(root, cfg, diff, ds, 35)
    held, written = [], []
    a = generate(0, diff, dict(cfg), ds, ckpt_iter="max", n_samples=2, exp_root=root, seed=11, mel_name="LJ001-0001",
                 report_mel=True, mel_errors=held, written=written, guide_op="mel", guide_scale=0.5)
    text = capsys.readouterr().out
    assert a.shape == (2, 1, 1536) and torch.isfinite(a).all()
    assert "guided sampler ddpm (mel, scale 0.5): 6 network evaluations" in text
    assert len(held) == 1 and np.isfinite(held[0])
    assert f"batch 0 mel error: mean |log-mel(generated) - condition| = {held[0]:.4f}" in text
    assert len(written) == 2 and all(os.path.exists(f) for f in written)
    sr, w = wavfile.read(written[0])
    assert sr == 22050 and w.shape == (1536,)

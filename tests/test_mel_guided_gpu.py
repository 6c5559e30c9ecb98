"""GPU: `sampling.sampling_guided` with `sampling.mel_operator` (the engine's log-mel, adjoint
`dws_mel_spectrogram_backward`) against the float64 loop of tests/guided_reference.py with the float64 restatement of the
transform (tests/mel_reference.py) as its operator -- same weights, x_T and noise; and `generate.guide_op=mel` /
`generate.report_mel` end to end.

Models and problem construction are those of tests/test_guided_sampling_gpu.py (WaveNet 64 channels / 3 layers, B = 2,
L = 200; SaShiMi d32, L = 1024); the operator is n_fft 64, hop 16, 20 bands at 16 kHz, the measurement the mel of
randn 0.3.

Guidance scale 0.1 for both samplers.  Measured on the CPU with the reference alone (float64 oracle loop, and the same
loop run entirely in float32 -- network, operator and state):

    sampler            all-float32 loop vs float64 loop      guidance moves the result by
    DDIM 6/50, eta 1   2.0e-7 (WaveNet)  2.6e-5 (SaShiMi)    2.8e-2 (WaveNet)  7.0e-2 (SaShiMi)
    DDPM, 6 steps      4.9e-7 (WaveNet)  3.5e-7 (SaShiMi)    3.7e-2 (WaveNet)  5.4e-2 (SaShiMi)

so a float32 engine has room under REL_TOL = 1e-3 and the guided run is > 10 REL_TOL from the unguided one.  (On the
6-step DDPM schedule scale 0.2 moves the WaveNet result by 6.4e-1: the run leaves the regime where the comparison says
anything; 0.05 moves it by 1.8e-2, too close to 10 REL_TOL.)

CLI scale 0.5: on the CPU oracle of the conditional SaShiMi, three seeds, the mel error of the 6-step DDPM run falls
monotonically with the scale (1.80 -> 1.79 at 0.1 -> 1.74 at 0.5)."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import mel_reference as mref
from tests.conftest import REL_TOL, rel_err
from tests.guided_reference import oracle_net, reference_guided
from tests.test_guided_sampling_gpu import BETA6, SAMPLERS, SS_COND, WN, _engine, _model, _schedule

pytestmark = pytest.mark.gpu

STFT = dict(filter_length=64, hop_length=16, win_length=64, n_mel_channels=20, sampling_rate=16000, mel_fmin=0.0,
            mel_fmax=8000.0)
SCALE = 0.1


def _stft():
    from diffwave_sashimi_amd.mel import TacotronSTFT
    return cases.cached(("mel_guided_stft",), lambda: TacotronSTFT(**STFT))


def _problem(name, S=6):
    cfg, B, L, wseed, sd = _model(name)
    st = _stft()
    g = torch.Generator().manual_seed(41)
    clean = torch.randn(B, 1, L, generator=g) * 0.3
    x_T = torch.randn(B, 1, L, generator=g)
    noise = torch.randn(S, B, 1, L, generator=g)
    op64 = mref.reference_operator(st.window, st.mel_basis, 64, 16)
    return cfg, B, L, sd, op64, op64(clean.double()), x_T, noise


def _reference(name, sampler_key):
    def make():
        cfg, B, L, sd, op64, y, x_T, noise = _problem(name)
        sampler, eta = SAMPLERS[sampler_key]
        dh, steps = _schedule(sampler)
        net64 = oracle_net(cfg, sd, torch.float64)
        run = lambda scale: reference_guided(net64, (B, 1, L), dh, y=y, operator=op64, scale=scale, sampler=sampler,
                                             steps=steps, eta=eta, x_T=x_T, noise=noise)
        return run(SCALE), run(0.0)
    return cases.cached(("mel_guided_reference", name, sampler_key), make)


@pytest.mark.parametrize("precision", ["f32", "bf16x6"])
@pytest.mark.parametrize("sampler_key", ["ddim_eta1", "ddpm6"])
@pytest.mark.parametrize("name", ["wavenet", "sashimi"])
def test_engine_mel_guided_run_matches_the_float64_loop(gpu, name, sampler_key, precision):
    from diffwave_sashimi_amd.sampling import mel_operator, sampling_guided
    cfg, B, L, sd, op64, y, x_T, noise = _problem(name)
    sampler, eta = SAMPLERS[sampler_key]
    dh, steps = _schedule(sampler)
    ref, plain = _reference(name, sampler_key)
    net = _engine(name, gpu, precision)
    got = sampling_guided(net, (B, 1, L), dh, measurement=y.float().to(gpu), operator=mel_operator(_stft()), scale=SCALE,
                          sampler=sampler, steps=steps, eta=eta, x_T=x_T.to(gpu), noise=noise.to(gpu))
    assert got.device.type == "cuda" and got.shape == (B, 1, L) and torch.isfinite(got).all()
    err, moved = rel_err(got.cpu(), ref), rel_err(plain, ref)
    print(f"{name} mel {sampler_key} {precision}: engine vs float64 loop {err:.2e} (guidance moves the result by {moved:.2e})")
    assert err <= REL_TOL
    assert moved > 10 * REL_TOL
    assert all(p.grad is None for p in net.parameters())


def _checkpoint(root, cfg, diff, ds, wseed):
    from diffwave_sashimi_amd.generate import local_path_name
    run = local_path_name(None, cfg, diff, ds)
    os.makedirs(os.path.join(root, run, "checkpoint"))
    torch.save({"model_state_dict": cases.build_ours(cfg, wseed).state_dict()}, os.path.join(root, run, "checkpoint", "1000.pkl"))


def test_generate_cli_guides_towards_the_mel_of_a_wav(tmp_path, gpu, capsys):
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import generate
    cfg = dict(WN)
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=BETA6)
    data = tmp_path / "wavs"
    os.makedirs(data)
    wavfile.write(str(data / "target.wav"), 16000, np.random.default_rng(3).standard_normal(640).astype(np.float32) * 0.3)
    ds = dict(_name_="sc09", data_path=str(data), segment_length=640, sampling_rate=16000)      # no STFT keys: 1024 / 256
    root = str(tmp_path / "exp")
    _checkpoint(root, cfg, diff, ds, 5)
    written = []
    kw = dict(ckpt_iter="max", n_samples=2, exp_root=root, seed=11)
    a = generate(0, diff, dict(cfg), ds, written=written, guide_name="target", guide_op="mel", guide_scale=0.1, **kw)
    text = capsys.readouterr().out
    assert a.shape == (2, 1, 640) and torch.isfinite(a).all()
    assert "guided sampler ddpm (mel, scale 0.1): 6 network evaluations" in text and "mel error" not in text
    assert len(written) == 2 and all(os.path.exists(f) for f in written)
    sr, w = wavfile.read(written[0])
    assert sr == 16000 and np.array_equal(w, a[0, 0].cpu().numpy())
    assert torch.equal(a, generate(0, diff, dict(cfg), ds, guide_name="target", guide_op="mel", guide_scale=0.1, **kw))
    assert not torch.equal(a, generate(0, diff, dict(cfg), ds, **kw))
    capsys.readouterr()
    b = generate(0, diff, dict(cfg), ds, sampler="ddim", steps=4, eta=0.5, guide_name="target", guide_op="mel",
                 guide_scale=0.05, **kw)
    assert "guided sampler ddim (mel, scale 0.05): 4 network evaluations" in capsys.readouterr().out
    assert b.shape == (2, 1, 640) and torch.isfinite(b).all()


def test_generate_cli_keeps_a_vocoder_on_its_mel_and_reports_the_mel_error(tmp_path, gpu, capsys):
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import generate
    cfg = dict(SS_COND)
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=BETA6)
    data = tmp_path / "wavs"
    os.makedirs(data)
    wav = (np.random.default_rng(3).standard_normal(1000) * 0.3 * 32767).clip(-32767, 32767).astype(np.int16)
    wavfile.write(str(data / "LJ001-0001.wav"), 22050, wav)            # 1000 samples -> 4 frames -> L = 1024
    ds = dict(_name_="ljspeech", data_path=str(data), segment_length=1024, sampling_rate=22050, filter_length=1024,
              hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0)
    root = str(tmp_path / "exp")
    _checkpoint(root, cfg, diff, ds, 35)
    kw = dict(ckpt_iter="max", n_samples=2, exp_root=root, seed=11, mel_name="LJ001-0001")
    plain = generate(0, diff, dict(cfg), ds, **kw)
    assert "mel error" not in capsys.readouterr().out                   # without the key the output is today's
    free, held, written = [], [], []
    same = generate(0, diff, dict(cfg), ds, report_mel=True, mel_errors=free, **kw)
    text = capsys.readouterr().out
    assert torch.equal(same, plain) and len(free) == 1
    assert f"batch 0 mel error: mean |log-mel(generated) - condition| = {free[0]:.4f}" in text
    a = generate(0, diff, dict(cfg), ds, report_mel=True, mel_errors=held, written=written, guide_op="mel", guide_scale=0.5,
                 **kw)
    text = capsys.readouterr().out
    assert a.shape == (2, 1, 1024) and torch.isfinite(a).all() and not torch.equal(a, plain)
    assert "guided sampler ddpm (mel, scale 0.5): 6 network evaluations" in text
    assert f"batch 0 mel error: mean |log-mel(generated) - condition| = {held[0]:.4f}" in text
    assert len(written) == 2 and all(os.path.exists(f) for f in written)
    print(f"mel error of the identical run: {free[0]:.4f} unguided, {held[0]:.4f} guided")
    assert len(held) == 1 and held[0] < free[0]
    two = []
    generate(0, diff, dict(cfg), ds, report_mel=True, mel_errors=two, batch_size=1, **kw)
    assert len(two) == 2 and capsys.readouterr().out.count("mel error: mean") == 2

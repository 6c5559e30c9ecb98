"""GPU: the adaptive prior through ``generate`` and ``train`` (``+generate.prior=energy ...`` / ``+train.prior=energy ...``)."""
import os

import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu

E_MAX = 7.0


def test_generate_and_train_with_an_energy_prior(tmp_path, gpu, capsys):
    """wn_cond_c64: the smallest mel-conditional WaveNet the engine trains."""
    from scipy.io import wavfile
    from diffwave_sashimi_amd import sampling as smp
    from diffwave_sashimi_amd.generate import generate, local_path_name
    from diffwave_sashimi_amd.mel import prior_std_from_mel
    from diffwave_sashimi_amd.models import construct_model
    from diffwave_sashimi_amd.train import train
    cfg = dict(cases.WAVENET_COND_CASES["wn_cond_c64"][0])
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=None)
    data, mdir = tmp_path / "wavs", tmp_path / "mels"
    os.makedirs(data)
    os.makedirs(mdir)
    rng = np.random.default_rng(3)
    for stem, n in (("a", 1100), ("b", 900)):
        wavfile.write(str(data / f"{stem}.wav"), 22050, (rng.standard_normal(n) * 3000).astype(np.int16))
    mel = cases.mel_inputs(1, 2, 44)
    mel[0, :, 0] = float(np.log(1e-5))              # a silent first frame: sigma = std_min over its 256 samples
    torch.save(mel[0], str(mdir / "utt.wav.pt"))
    ds = dict(_name_="ljspeech", data_path=str(data), segment_length=768, sampling_rate=22050, filter_length=1024,
              hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0)
    root = str(tmp_path / "exp")

    # ---- generate from seeded random weights: the wav is the Python call with the same sigma
    gen = dict(ckpt_iter="init", n_samples=2, mel_name="utt", mel_path=str(mdir), sampler="ddim", steps=4, seed=5,
               clip_seeds=True, exp_root=root)
    torch.manual_seed(3)
    written = []
    audio = generate(0, diff, dict(cfg), ds, prior="energy", prior_energy_max=E_MAX, written=written, **gen)
    out = capsys.readouterr().out
    assert f"adaptive prior: energy_max={E_MAX:g} energy_min=0 std_min=0.1" in out
    torch.manual_seed(3)
    net = construct_model(dict(cfg)).cuda().eval()
    sg = prior_std_from_mel(mel.to(gpu), 256, 512, energy_max=E_MAX)
    assert float(sg[0, 0, 0]) == np.float32(0.1) and float(sg.max()) > 0.5
    dh = smp.calc_diffusion_hyperparams(50, 1e-4, 0.05)
    seeds = [smp.clip_seeds(5, k, 1)[0] for k in range(2)]
    want = smp.sampling_ddim(net, (2, 1, 512), dh, 4, eta=0.0, condition=mel.to(gpu), seed=seeds,
                             prior_std=sg.expand(2, 1, 512))
    assert torch.equal(audio, want) and torch.isfinite(audio).all()
    for k, f in enumerate(written):
        assert np.array_equal(wavfile.read(f)[1], want[k, 0].cpu().numpy())
    torch.manual_seed(3)
    plain = generate(0, diff, dict(cfg), ds, **gen)                     # no keys, no checkpoint entry: N(0, I)
    assert "adaptive prior" not in capsys.readouterr().out
    assert not torch.equal(plain, audio)
    assert float(audio[:, :, :256].abs().max()) < float(plain[:, :, :256].abs().max())      # the silent frame starts quieter

    # ---- a two-iteration training run writes the prior into its checkpoints; generate picks it up and prints it
    train(0, 1, diffusion_cfg=diff, model_cfg=dict(cfg), dataset_cfg=ds,
          generate_cfg={"n_samples": 1, "mel_name": "a", "sampler": "ddim", "steps": 4, "seed": 1},
          ckpt_iter=-1, n_iters=1, iters_per_ckpt=1, iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=2,
          exp_root=root, num_workers=0, prior="energy", prior_energy_max=E_MAX, prior_std_min=0.2)
    out = capsys.readouterr().out
    entry = {"kind": "energy", "energy_max": E_MAX, "energy_min": 0.0, "std_min": 0.2}
    ckpt = os.path.join(root, local_path_name(None, cfg, diff, ds), "checkpoint")
    for it in (0, 1):
        assert torch.load(os.path.join(ckpt, f"{it}.pkl"), map_location="cpu")["prior"] == entry
    line = f"adaptive prior (the checkpoint's prior entry): energy_max={E_MAX:g} energy_min=0 std_min=0.2"
    assert out.count(line) == 2                                         # the in-loop generation of both checkpoints
    again = dict(gen, ckpt_iter=1)
    a = generate(0, diff, dict(cfg), ds, **again)
    assert line in capsys.readouterr().out
    b = generate(0, diff, dict(cfg), ds, prior="energy", prior_energy_max=E_MAX, **again)       # the same, spelled out
    assert f"adaptive prior: energy_max={E_MAX:g} energy_min=0 std_min=0.2" in capsys.readouterr().out
    c = generate(0, diff, dict(cfg), ds, prior="none", **again)
    assert "adaptive prior" not in capsys.readouterr().out
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(a).all()
    with pytest.raises(ValueError, match="contradicts the checkpoint"):
        generate(0, diff, dict(cfg), ds, prior="energy", prior_energy_max=E_MAX + 1, **again)
    with pytest.raises(ValueError, match="contradicts the checkpoint"):
        generate(0, diff, dict(cfg), ds, prior="energy", prior_energy_max=E_MAX, prior_std_min=0.1, **again)

    # ---- checkpoint smoothing: the common prior of the averaged checkpoints is used; a mixed set is refused
    smooth = dict(gen, ckpt_iter=1, ckpt_smooth=-1)
    s = generate(0, diff, dict(cfg), ds, **smooth)
    assert line in capsys.readouterr().out and torch.isfinite(s).all()
    saved = torch.load(os.path.join(ckpt, "1.pkl"), map_location="cpu")
    del saved["prior"]
    torch.save(saved, os.path.join(ckpt, "2.pkl"))
    with pytest.raises(ValueError, match="different priors"):
        generate(0, diff, dict(cfg), ds, **dict(smooth, ckpt_iter=2))

    # ---- a resume must name the prior the checkpoint was trained with
    tr = dict(diffusion_cfg=diff, model_cfg=dict(cfg), dataset_cfg=ds, generate_cfg={}, ckpt_iter=1, n_iters=2,
              iters_per_ckpt=1, iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=2, exp_root=root, num_workers=0)
    with pytest.raises(ValueError, match="was trained with the prior"):
        train(0, 1, **tr)                                                               # no keys: would drop the prior
    with pytest.raises(ValueError, match="was trained with the prior"):
        train(0, 1, prior="energy", prior_energy_max=E_MAX, **tr)                       # std_min 0.1, trained with 0.2
    train(0, 1, prior="energy", prior_energy_max=E_MAX, prior_std_min=0.2, **tr)        # the same prior: resumes
    assert "Successfully loaded model at iteration 1" in capsys.readouterr().out
    assert torch.load(os.path.join(ckpt, "2.pkl"), map_location="cpu")["prior"] == entry

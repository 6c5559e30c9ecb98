"""GPU: the spectral prior through ``generate`` and ``train`` (``+generate.prior=spectral ...`` / ``+train.prior=spectral
...``)."""
import os

import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu

REF = 3.0


def test_generate_and_train_with_a_spectral_prior(tmp_path, gpu, capsys):
    """wn_cond_c64: the smallest mel-conditional WaveNet the engine trains; the dataset's STFT is 1024 / 256 / 1024, so a
    clip holds at least 513 samples: segments and the conditioning mel are three frames long."""
    from scipy.io import wavfile
    from diffwave_sashimi_amd import sampling as smp
    from diffwave_sashimi_amd.generate import generate, local_path_name
    from diffwave_sashimi_amd.mel import TacotronSTFT
    from diffwave_sashimi_amd.models import construct_model
    from diffwave_sashimi_amd.train import PriorMismatch, train
    cfg = dict(cases.WAVENET_COND_CASES["wn_cond_c64"][0])
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=None)
    data, mdir = tmp_path / "wavs", tmp_path / "mels"
    os.makedirs(data)
    os.makedirs(mdir)
    rng = np.random.default_rng(3)
    for stem, n in (("a", 1100), ("b", 900)):
        wavfile.write(str(data / f"{stem}.wav"), 22050, (rng.standard_normal(n) * 3000).astype(np.int16))
    mel = cases.mel_inputs(1, 3, 44)
    torch.save(mel[0], str(mdir / "utt.wav.pt"))
    ds = dict(_name_="ljspeech", data_path=str(data), segment_length=768, sampling_rate=22050, filter_length=1024,
              hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0)
    root = str(tmp_path / "exp")

    # ---- generate from seeded random weights: the wav is the Python call with the same filter
    gen = dict(ckpt_iter="init", n_samples=2, mel_name="utt", mel_path=str(mdir), sampler="ddim", steps=4, eta=0.5, seed=5,
               clip_seeds=True, exp_root=root)
    torch.manual_seed(3)
    written = []
    audio = generate(0, diff, dict(cfg), ds, prior="spectral", prior_ref=REF, prior_lifter=12, written=written, **gen)
    out = capsys.readouterr().out
    assert f"spectral prior: ref={REF:g} floor=0.01 lifter=12" in out
    torch.manual_seed(3)
    net = construct_model(dict(cfg)).cuda().eval()
    stft = TacotronSTFT(filter_length=1024, hop_length=256, win_length=1024, sampling_rate=22050, mel_fmin=0.0, mel_fmax=8000.0)
    F = stft.spectral_filter(mel.to(gpu), 768, ref=REF, lifter=12)
    dh = smp.calc_diffusion_hyperparams(50, 1e-4, 0.05)
    seeds = [smp.clip_seeds(5, k, 1)[0] for k in range(2)]
    want = smp.sampling_ddim(net, (2, 1, 768), dh, 4, eta=0.5, condition=mel.to(gpu), seed=seeds,
                             prior_filter=F.expand(2, -1, -1), prior_stft=stft)
    assert torch.equal(audio, want) and torch.isfinite(audio).all()
    for k, f in enumerate(written):
        assert np.array_equal(wavfile.read(f)[1], want[k, 0].cpu().numpy())
    torch.manual_seed(3)
    plain = generate(0, diff, dict(cfg), ds, **gen)                     # no keys, no checkpoint entry: N(0, I)
    assert "spectral prior" not in capsys.readouterr().out
    assert not torch.equal(plain, audio)
    for bad in (dict(known_name="a", keep=[[0, 100]]), dict(start_name="a", start_step=2),
                dict(guide_name="a", guide_op="declip", guide_scale=0.5)):
        with pytest.raises(ValueError, match="does not combine with the spectral prior"):
            generate(0, diff, dict(cfg), ds, prior="spectral", prior_ref=REF, **dict(gen, **bad))

    # ---- a two-iteration training run writes the prior into its checkpoints; generate picks it up and prints it
    train(0, 1, diffusion_cfg=diff, model_cfg=dict(cfg), dataset_cfg=ds,
          generate_cfg={"n_samples": 1, "mel_name": "a", "sampler": "ddim", "steps": 4, "seed": 1},
          ckpt_iter=-1, n_iters=1, iters_per_ckpt=1, iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=2,
          exp_root=root, num_workers=0, prior="spectral", prior_ref=REF, prior_floor=0.02)
    out = capsys.readouterr().out
    entry = {"kind": "spectral", "ref": REF, "floor": 0.02, "lifter": 24}
    ckpt = os.path.join(root, local_path_name(None, cfg, diff, ds), "checkpoint")
    for it in (0, 1):
        assert torch.load(os.path.join(ckpt, f"{it}.pkl"), map_location="cpu")["prior"] == entry
    line = f"spectral prior (the checkpoint's prior entry): ref={REF:g} floor=0.02 lifter=24"
    assert out.count(line) == 2                                         # the in-loop generation of both checkpoints
    again = dict(gen, ckpt_iter=1)
    a = generate(0, diff, dict(cfg), ds, **again)
    assert line in capsys.readouterr().out
    b = generate(0, diff, dict(cfg), ds, prior="spectral", prior_ref=REF, **again)              # the same, spelled out
    assert f"spectral prior: ref={REF:g} floor=0.02 lifter=24" in capsys.readouterr().out
    c = generate(0, diff, dict(cfg), ds, prior="none", **again)
    assert "spectral prior" not in capsys.readouterr().out
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(a).all() and torch.isfinite(c).all()
    with pytest.raises(ValueError, match="contradicts the checkpoint"):
        generate(0, diff, dict(cfg), ds, prior="spectral", prior_ref=REF + 1, **again)
    with pytest.raises(ValueError, match="contradicts the checkpoint"):
        generate(0, diff, dict(cfg), ds, prior="energy", prior_energy_max=7.0, **again)
    # a ragged batch of utterances: each with the filter of its own mel, its last frame repeated once
    torch.save(cases.mel_inputs(1, 4, 45)[0], str(mdir / "long.wav.pt"))
    ragged = {k: v for k, v in again.items() if k not in ("mel_name", "n_samples")}
    clips = generate(0, diff, dict(cfg), ds, mel_names=["long", "utt"], **ragged)
    assert line in capsys.readouterr().out
    assert [tuple(c.shape) for c in clips] == [(1, 1024), (1, 768)] and all(torch.isfinite(c).all() for c in clips)

    # ---- a resume must name the prior the checkpoint was trained with
    tr = dict(diffusion_cfg=diff, model_cfg=dict(cfg), dataset_cfg=ds, generate_cfg={}, ckpt_iter=1, n_iters=2,
              iters_per_ckpt=1, iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=2, exp_root=root, num_workers=0)
    with pytest.raises(PriorMismatch, match="was trained with the prior"):
        train(0, 1, **tr)                                                               # no keys: would drop the prior
    with pytest.raises(PriorMismatch, match="was trained with the prior"):
        train(0, 1, prior="spectral", prior_ref=REF, **tr)                              # floor 0.01, trained with 0.02
    with pytest.raises(PriorMismatch, match="was trained with the prior"):
        train(0, 1, prior="energy", prior_energy_max=7.0, **tr)                         # another kind
    train(0, 1, prior="spectral", prior_ref=REF, prior_floor=0.02, **tr)                # the same prior: resumes
    assert "Successfully loaded model at iteration 1" in capsys.readouterr().out
    assert torch.load(os.path.join(ckpt, "2.pkl"), map_location="cpu")["prior"] == entry

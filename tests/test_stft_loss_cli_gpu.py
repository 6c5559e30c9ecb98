"""GPU: the spectral training loss through ``train`` (``+train.stft_weight=0.1 ...``): two iterations on synthetic clips,
the log's ``train/stft_loss``, the checkpoint's ``stft_loss`` entry, a resume that prints it, and a run without the key."""
import json
import os

import pytest
import torch

from tests.test_generate_cli import _tree

pytestmark = pytest.mark.gpu


def test_train_with_and_without_the_spectral_term(tmp_path, gpu, capsys):
    from diffwave_sashimi_amd.generate import load_config, local_path_name
    from diffwave_sashimi_amd.train import distributed_train
    d = _tree(tmp_path / "configs")

    def train_main(overrides, exp_root):      # train.py's main() behind its device count: one rank on this GPU
        distributed_train(0, 1, "g", load_config(d, overrides), exp_root)
    model = ["model=wavenet", "model.res_channels=64", "model.skip_channels=64", "model.num_res_layers=4",
             "model.dilation_cycle=4", "+model.in_channels=1", "+model.out_channels=1",
             "+model.diffusion_step_embed_dim_in=128", "+model.diffusion_step_embed_dim_mid=512",
             "+model.diffusion_step_embed_dim_out=512", "dataset._name_=synthetic", "dataset.segment_length=1024",
             "+dataset.n_items=8", "diffusion.T=8", "generate.n_samples=0"]
    tr = ["+train.ckpt_iter=-1", "+train.n_iters=1", "+train.iters_per_ckpt=1", "+train.iters_per_logging=1",
          "+train.learning_rate=2e-3", "+train.batch_size_per_gpu=4", "+train.num_workers=0"]
    stft = ["+train.stft_weight=0.1", "+train.stft_max_step=6", "+train.stft_resolutions=[[256,64,128],[128,32,64]]"]
    cfg = load_config(d, model)
    run = local_path_name(None, cfg["model"], cfg["diffusion"], cfg["dataset"])
    entry = {"weight": 0.1, "max_step": 6, "resolutions": [[256, 64, 128], [128, 32, 64]]}

    exp = str(tmp_path / "exp_stft")
    torch.manual_seed(0)
    train_main(model + tr + stft, exp)                                  # iterations 0 and 1
    log = [json.loads(l) for l in open(os.path.join(exp, run, "train_log.jsonl"))]
    steps = [r for r in log if "train/loss" in r]
    assert len(steps) == 2
    for r in steps:
        assert r["train/stft_loss"] >= 0.0 and r["train/eps_loss"] > 0.0
        assert abs(r["train/loss"] - (r["train/eps_loss"] + 0.1 * r["train/stft_loss"])) <= 1e-5 * r["train/loss"]
    assert any(r["train/stft_loss"] > 0.0 for r in steps)
    for it in (0, 1):
        assert torch.load(os.path.join(exp, run, "checkpoint", f"{it}.pkl"), map_location="cpu")["stft_loss"] == entry
    capsys.readouterr()
    # a resume prints the entry; the keys are information, not a condition: this one drops the mask and trains on
    train_main(model + ["+train.ckpt_iter=max", "+train.n_iters=2"] + tr[2:] + stft[:1] + stft[2:], exp)
    out = capsys.readouterr().out
    assert "Successfully loaded model at iteration 1" in out
    assert f"checkpoint 1 was trained with stft_loss = {entry!r}" in out
    assert torch.load(os.path.join(exp, run, "checkpoint", "2.pkl"), map_location="cpu")["stft_loss"] == \
        dict(entry, max_step=None)

    # without the key: neither the log entries nor the checkpoint entry, and a resume prints nothing about it
    plain = str(tmp_path / "exp_plain")
    torch.manual_seed(0)
    train_main(model + tr, plain)
    log = [json.loads(l) for l in open(os.path.join(plain, run, "train_log.jsonl"))]
    assert sum("train/loss" in r for r in log) == 2
    assert not any("train/stft_loss" in r or "train/eps_loss" in r for r in log)
    assert "stft_loss" not in torch.load(os.path.join(plain, run, "checkpoint", "1.pkl"), map_location="cpu")
    train_main(model + ["+train.ckpt_iter=max", "+train.n_iters=2"] + tr[2:], plain)
    out = capsys.readouterr().out
    assert "Successfully loaded model at iteration 1" in out and "stft_loss" not in out

    # a bad value stops the run before a model is built
    with pytest.raises(ValueError, match="stft_weight"):
        train_main(model + tr + ["+train.stft_weight=-1"], str(tmp_path / "exp_bad"))
    assert "parameters:" not in capsys.readouterr().out

"""GPU: the class-conditional path through the two drivers -- two training iterations on labelled synthetic clips, the
checkpoint's table, then guided generation of chosen classes from that checkpoint."""
import os

import pytest
import torch

from tests.test_generate_cli import _tree

pytestmark = pytest.mark.gpu


def test_train_then_generate_chosen_classes(tmp_path, gpu):
    from diffwave_sashimi_amd.generate import generate, load_config, local_path_name
    from diffwave_sashimi_amd.train import train
    d = _tree(tmp_path / "configs")
    cfg = load_config(d, ["model=wavenet", "model.res_channels=64", "model.skip_channels=64", "model.num_res_layers=4",
                          "model.dilation_cycle=4", "model.in_channels=1", "model.out_channels=1",
                          "model.diffusion_step_embed_dim_in=128", "model.diffusion_step_embed_dim_mid=512",
                          "model.diffusion_step_embed_dim_out=512", "model.n_classes=3",
                          "dataset._name_=synthetic", "dataset.segment_length=1024", "dataset.n_items=8",
                          "diffusion.T=8"])
    exp = str(tmp_path / "exp")
    diffusion = {k: v for k, v in cfg["diffusion"].items() if k != "beta"}
    torch.manual_seed(0)
    train(0, 1, diffusion_cfg=diffusion, model_cfg=cfg["model"], dataset_cfg=cfg["dataset"],
          generate_cfg={"n_samples": 3, "batch_size": 3}, ckpt_iter=-1, n_iters=1, iters_per_ckpt=1, iters_per_logging=1,
          learning_rate=2e-3, batch_size_per_gpu=4, exp_root=exp, num_workers=0)
    run = local_path_name(None, cfg["model"], cfg["diffusion"], cfg["dataset"])
    assert "_cls3" in run
    saved = torch.load(os.path.join(exp, run, "checkpoint", "1.pkl"), map_location="cpu")["model_state_dict"]
    key = "residual_layer.label_embedding.weight"
    assert tuple(saved[key].shape) == (4, 512)
    first = torch.load(os.path.join(exp, run, "checkpoint", "0.pkl"), map_location="cpu")["model_state_dict"]
    assert not torch.equal(saved[key], first[key])                 # the table is trained
    # the in-loop generation cycled the classes
    wavs = sorted(os.listdir(os.path.join(exp, run, "waveforms", "1")))
    assert wavs == ["0k_0_c0.wav", "0k_1_c1.wav", "0k_2_c2.wav"]
    out = generate(0, diffusion, cfg["model"], cfg["dataset"], ckpt_iter=1, n_samples=2, exp_root=exp, seed=3,
                   label=[0, 2], cfg_scale=1.0)
    assert out.shape == (2, 1, 1024) and bool(torch.isfinite(out).all())
    wavs = sorted(os.listdir(os.path.join(exp, run, "waveforms", "1")))
    assert "0k_0_c0.wav" in wavs and "0k_1_c2.wav" in wavs
    plain = generate(0, diffusion, cfg["model"], cfg["dataset"], ckpt_iter=1, n_samples=2, exp_root=exp, seed=3, label=[0, 2])
    assert not torch.equal(plain, out)

"""GPU: multi-band runs through ``train`` and ``generate`` (``+model.subbands=4``): two training iterations on tiny seeded
wavs, the checkpoint's ``pqmf`` entry, generation from it (with and without the key), ragged batches, the refusals, and
a full-band checkpoint that runs as before."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.conftest import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

K = 4


def test_train_and_generate_on_subbands(tmp_path, gpu, capsys):
    """wn_cond_c64 (the smallest mel-conditional WaveNet the engine trains) with ``mel_upsample = [8, 8]``: 64 sub-band
    positions per mel frame, hop 256 with K = 4."""
    from scipy.io import wavfile
    from diffwave_sashimi_amd import sampling as smp
    from diffwave_sashimi_amd.generate import generate, local_path_name
    from diffwave_sashimi_amd.models import construct_model
    from diffwave_sashimi_amd.pqmf import PQMF
    from diffwave_sashimi_amd.train import train
    base = {k: v for k, v in cases.WAVENET_COND_CASES["wn_cond_c64"][0].items() if k not in ("in_channels", "out_channels")}
    plain_cfg = dict(base, mel_upsample=[8, 8])                # no key: what generate sees when it follows the checkpoint
    cfg = dict(plain_cfg, subbands=K)
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=None)
    data, mdir = tmp_path / "wavs", tmp_path / "mels"
    os.makedirs(data)
    os.makedirs(mdir)
    rng = np.random.default_rng(3)
    wavs = {"a": 1100, "b": 900}                               # n // 256 + 1 = 5 and 4 mel frames
    for stem, n in wavs.items():
        wavfile.write(str(data / f"{stem}.wav"), 22050, (rng.standard_normal(n) * 3000).astype(np.int16))
    mel = cases.mel_inputs(1, 3, 44)
    torch.save(mel[0], str(mdir / "utt.wav.pt"))
    ds = dict(_name_="ljspeech", data_path=str(data), segment_length=768, sampling_rate=22050, filter_length=1024,
              hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0)
    root = str(tmp_path / "exp")
    entry = PQMF(K).options()
    line = "subbands=4 taps=62 cutoff=0.142 beta=9"

    # ---- two training iterations write the entry; the in-loop generate runs on the sub-bands
    torch.manual_seed(0)
    train(0, 1, diffusion_cfg=diff, model_cfg=dict(cfg), dataset_cfg=ds,
          generate_cfg={"n_samples": 1, "mel_name": "a", "sampler": "ddim", "steps": 4, "seed": 1},
          ckpt_iter=-1, n_iters=1, iters_per_ckpt=1, iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=2,
          exp_root=root, num_workers=0)
    out = capsys.readouterr().out
    assert out.count("multi-band run: " + line) == 3            # the training run and the in-loop generation of both checkpoints
    ckpt = os.path.join(root, local_path_name(None, cfg, diff, ds), "checkpoint")
    for it in (0, 1):
        saved = torch.load(os.path.join(ckpt, f"{it}.pkl"), map_location="cpu")
        assert saved["pqmf"] == entry
        assert saved["model_state_dict"]["init_conv.0.conv.weight_v"].shape[1] == K

    # ---- generate from it: the wavs are P.synthesis(sampler(...)) of the Python call with the same seeds
    gen = dict(ckpt_iter=1, n_samples=2, mel_name="utt", mel_path=str(mdir), sampler="ddim", steps=4, seed=5,
               clip_seeds=True, exp_root=root)
    written = []
    audio = generate(0, diff, dict(cfg), ds, written=written, **gen)
    assert "multi-band run: " + line in capsys.readouterr().out
    net = construct_model(dict(cfg)).cuda().eval()
    net.load_state_dict(torch.load(os.path.join(ckpt, "1.pkl"), map_location="cpu")["model_state_dict"])
    assert net.in_channels == net.out_channels == K
    dh = smp.calc_diffusion_hyperparams(50, 1e-4, 0.05)
    seeds = [smp.clip_seeds(5, k, 1)[0] for k in range(2)]
    bands = smp.sampling_ddim(net, (2, K, 768 // K), dh, 4, eta=0.0, condition=mel.to(gpu), seed=seeds)
    want = PQMF(K).synthesis(bands)
    assert audio.shape == (2, 1, 3 * 256) and torch.equal(audio, want) and torch.isfinite(audio).all()
    assert float(audio.abs().max()) > 0
    for k, f in enumerate(written):
        got = wavfile.read(f)[1]
        assert got.shape == (3 * 256,) and np.array_equal(got, want[k, 0].cpu().numpy())
    # without the key the entry is used (and printed as the checkpoint's); keys that contradict it are refused
    follow = generate(0, diff, dict(plain_cfg), ds, **gen)
    assert "multi-band run (the checkpoint's pqmf entry): " + line in capsys.readouterr().out
    assert torch.equal(follow, audio)
    with pytest.raises(ValueError, match="contradicts the checkpoint"):
        generate(0, diff, dict(cfg, pqmf_taps=30), ds, **gen)
    with pytest.raises(ValueError, match="known_name does not combine with model.subbands"):
        generate(0, diff, dict(cfg), ds, known_name="a", keep=[[0, 100]], **gen)
    with pytest.raises(ValueError, match="known_name does not combine with model.subbands"):
        generate(0, diff, dict(plain_cfg), ds, known_name="a", keep=[[0, 100]], **gen)      # (K from the checkpoint)

    # ---- ragged batches: two utterances of two lengths in one batch, each wav at its own length and as it is alone
    rag = dict(ckpt_iter=1, sampler="ddim", steps=4, seed=5, clip_seeds=True, exp_root=root)
    written = []
    clips = generate(0, diff, dict(cfg), ds, mel_names=list(wavs), written=written, **rag)
    out = capsys.readouterr().out
    assert "L_max = 1280, lengths = [1280, 1024]" in out
    assert [tuple(c.shape) for c in clips] == [(1, 1280), (1, 1024)]
    for c, f in zip(clips, written):
        got = wavfile.read(f)[1]
        assert np.array_equal(got, c[0].cpu().numpy()) and np.isfinite(got).all() and np.abs(got).max() > 0
    alone = generate(0, diff, dict(cfg), ds, mel_names=list(wavs), batch_size=1, **rag)
    assert [tuple(c.shape) for c in alone] == [(1, 1280), (1, 1024)]
    # The longest utterance runs at its own length in both plans: the same audio up to the arithmetic of the kernel path.
    # The shorter one is another draw: a per-clip seed numbers the noise of a [C, L_max] state by c L_max + position, which
    # is the position alone only for one channel -- a valid sample of its own length, not the same.
    e = rel_err(clips[0], alone[0])
    print(f"the longest utterance: one batch vs alone: {e:.3e}")
    assert e < REL_TOL
    assert torch.isfinite(alone[1]).all() and float(alone[1].abs().max()) > 0

    # ---- a resume must name the bank the checkpoint was trained with
    tr = dict(diffusion_cfg=diff, dataset_cfg=ds, generate_cfg={}, ckpt_iter=1, n_iters=2, iters_per_ckpt=1,
              iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=2, exp_root=root, num_workers=0)
    with pytest.raises(ValueError, match="was trained with the filter bank"):
        train(0, 1, model_cfg=dict(cfg, pqmf_taps=30), **tr)
    train(0, 1, model_cfg=dict(cfg), **tr)
    assert "Successfully loaded model at iteration 1" in capsys.readouterr().out
    assert torch.load(os.path.join(ckpt, "2.pkl"), map_location="cpu")["pqmf"] == entry


def test_a_full_band_checkpoint_runs_as_before(tmp_path, gpu, capsys):
    """No ``pqmf`` entry and no ``model.subbands``: the wav is the plain sampler's output, bit for bit, and the same
    bytes on a second run; ``model.subbands`` on such a checkpoint is refused."""
    from scipy.io import wavfile
    from diffwave_sashimi_amd import sampling as smp
    from diffwave_sashimi_amd.generate import generate, local_path_name
    cfg, _, _, _, wseed, _, _ = cases.WAVENET_COND_CASES["wn_cond_c64"]
    diff = dict(T=4, beta_0=1e-4, beta_T=0.05, beta=None)
    mdir = tmp_path / "mels"
    os.makedirs(mdir)
    mel = cases.mel_inputs(1, 2, 41)
    torch.save(mel[0], str(mdir / "utt.wav.pt"))
    ds = dict(_name_="ljspeech", data_path=str(tmp_path), segment_length=768, sampling_rate=22050, filter_length=1024,
              hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0)
    root = str(tmp_path / "exp")
    run = local_path_name(None, cfg, diff, ds)
    os.makedirs(os.path.join(root, run, "checkpoint"))
    net = cases.build_ours(cfg, wseed)
    torch.save({"model_state_dict": net.state_dict()}, os.path.join(root, run, "checkpoint", "7.pkl"))
    gen = dict(ckpt_iter=7, n_samples=2, mel_name="utt", mel_path=str(mdir), seed=5, clip_seeds=True, exp_root=root)
    first, second = [], []
    a = generate(0, diff, dict(cfg), ds, written=first, **gen)
    b = generate(0, diff, dict(cfg), ds, written=second, **gen)
    assert "multi-band" not in capsys.readouterr().out
    dh = smp.calc_diffusion_hyperparams(**diff, fast=True)
    seeds = [smp.clip_seeds(5, k, 1)[0] for k in range(2)]
    want = smp.sampling(net.to(gpu), (2, 1, 512), dh, condition=mel.to(gpu), seed=seeds)
    assert torch.equal(a, want) and torch.equal(a, b)
    for k, (f, g) in enumerate(zip(first, second)):
        assert open(f, "rb").read() == open(g, "rb").read()
        assert np.array_equal(wavfile.read(f)[1], want[k, 0].cpu().numpy())
    with pytest.raises(ValueError, match="holds no pqmf entry"):
        generate(0, diff, {k: v for k, v in dict(cfg, subbands=K, mel_upsample=[8, 8]).items()
                           if k not in ("in_channels", "out_channels")}, ds, **gen)

"""GPU: ``generate.mel_names`` -- a list of utterances of different lengths vocoded in ragged batches."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.conftest import REL_TOL, rel_err

pytestmark = pytest.mark.gpu


def test_generate_vocodes_a_list_of_utterances(tmp_path, gpu, capsys):
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import generate, local_path_name
    cfg, _, _, _, wseed, _, _ = cases.WAVENET_COND_CASES["wn_cond_c64"]
    diff = dict(T=4, beta_0=1e-4, beta_T=0.05, beta=None)
    data = tmp_path / "wavs"
    os.makedirs(data)
    # utterances of 1, 3 and 2 mel frames.  The mel front-end's reflect padding needs more than filter_length / 2 = 512
    # samples (3 frames), so the short ones come as pre-generated spectrograms (generate.mel_path, `<stem>.wav.pt`); the
    # route from wavs is run below on longer ones.
    frames = {"short": 1, "long": 3, "mid": 2}
    mdir = tmp_path / "mels"
    os.makedirs(mdir)
    for i, (stem, f) in enumerate(frames.items()):
        torch.save(cases.mel_inputs(1, f, 40 + i)[0], str(mdir / f"{stem}.wav.pt"))
    ds = dict(_name_="ljspeech", data_path=str(data), segment_length=768, sampling_rate=22050, filter_length=1024,
              hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0)
    root = str(tmp_path / "exp")
    run = local_path_name(None, cfg, diff, ds)
    os.makedirs(os.path.join(root, run, "checkpoint"))
    torch.save({"model_state_dict": cases.build_ours(cfg, wseed).state_dict()}, os.path.join(root, run, "checkpoint", "7.pkl"))
    names = list(frames)

    def vocode(batch_size):
        written = []
        clips = generate(0, diff, dict(cfg), ds, ckpt_iter=7, mel_names=names, mel_path=str(mdir), batch_size=batch_size,
                         exp_root=root, seed=5, clip_seeds=True, written=written)
        files = {os.path.basename(f): wavfile.read(f)[1].copy() for f in written}
        return clips, files

    clips3, files3 = vocode(3)
    out = capsys.readouterr().out
    assert "L_max = 768" in out and "lengths = [768, 512, 256]" in out and "padded share = 0.333" in out
    assert sorted(files3) == sorted(f"0k_{s}.wav" for s in names)
    for k, stem in enumerate(names):
        assert clips3[k].shape == (1, frames[stem] * 256)
        assert files3[f"0k_{stem}.wav"].shape == (frames[stem] * 256,) and files3[f"0k_{stem}.wav"].dtype == np.float32
        assert np.array_equal(files3[f"0k_{stem}.wav"], clips3[k][0].cpu().numpy())
        assert np.isfinite(files3[f"0k_{stem}.wav"]).all() and np.abs(files3[f"0k_{stem}.wav"]).max() > 0
    # the same plan again: the same files, bit for bit
    _, again = vocode(3)
    for f in files3:
        assert np.array_equal(files3[f], again[f]), f
    # one utterance per batch, each at its own length: the same audio up to the arithmetic of the kernel path (the padded
    # length of a batch selects kernels and edge indicators: not bit for bit)
    _, files1 = vocode(1)
    for f in files3:
        e = rel_err(files3[f], files1[f])
        print(f"{f}: batch_size 3 vs 1: {e:.3e}")
        assert e < REL_TOL, (f, e)
    # the route from wavs (the HIP mel front-end): 600, 1100 and 800 samples -> n // 256 + 1 = 3, 5 and 4 frames, two batches
    rng = np.random.default_rng(3)
    wavs = {"w600": 600, "w1100": 1100, "w800": 800}
    for stem, n in wavs.items():
        wavfile.write(str(data / f"{stem}.wav"), 22050, (rng.standard_normal(n) * 3000).astype(np.int16))
    written = []
    clips = generate(0, diff, dict(cfg), ds, ckpt_iter=7, mel_names=list(wavs), batch_size=2, exp_root=root, seed=5,
                     clip_seeds=True, written=written)
    assert [tuple(c.shape) for c in clips] == [(1, (n // 256 + 1) * 256) for n in wavs.values()]
    assert [os.path.basename(f) for f in written] == ["0k_w600.wav", "0k_w1100.wav", "0k_w800.wav"]
    assert all(torch.isfinite(c).all() for c in clips)
    # argument checks
    with pytest.raises(ValueError, match="exclude"):
        generate(0, diff, dict(cfg), ds, ckpt_iter=7, mel_names=names, mel_name="long", exp_root=root)
    with pytest.raises(ValueError, match="seed"):
        generate(0, diff, dict(cfg), ds, ckpt_iter=7, mel_names=names, clip_seeds=True, exp_root=root)

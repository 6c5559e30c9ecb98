"""GPU: ``generate.mel_names`` with ``model=sashimi`` -- a list of utterances of different lengths vocoded in ragged batches."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.conftest import REL_TOL, rel_err

pytestmark = pytest.mark.gpu


def test_generate_vocodes_a_list_of_utterances_with_sashimi(tmp_path, gpu, capsys):
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import generate, local_path_name
    cfg, _, _, wseed, _, _ = cases.SASHIMI_COND_CASES["ss_cond_d32"]
    diff = dict(T=4, beta_0=1e-4, beta_T=0.05, beta=None)
    data = tmp_path / "wavs"
    os.makedirs(data)
    # utterances of 1, 3 and 2 mel frames as pre-generated spectrograms (generate.mel_path, `<stem>.wav.pt`); hop 256 is a
    # multiple of the pooling factors' product 16, so every length frames x hop divides through the stages
    frames = {"short": 1, "long": 3, "mid": 2}
    mdir = tmp_path / "mels"
    os.makedirs(mdir)
    for i, (stem, f) in enumerate(frames.items()):
        torch.save(cases.mel_inputs(1, f, 40 + i)[0], str(mdir / f"{stem}.wav.pt"))
    ds = dict(_name_="ljspeech", data_path=str(data), segment_length=1024, sampling_rate=22050, filter_length=1024,
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
    # one utterance per batch, each at its own length: the same audio up to the arithmetic of the kernel path (the run length
    # selects the FFT plan: not bit for bit)
    _, files1 = vocode(1)
    for f in files3:
        e = rel_err(files3[f], files1[f])
        print(f"{f}: batch_size 3 vs 1: {e:.3e}")
        assert e < REL_TOL, (f, e)
    # a hop that does not divide through the pooling stages is refused before a model is built
    with pytest.raises(ValueError, match="multiple of 16"):
        generate(0, diff, dict(cfg), dict(ds, hop_length=200), ckpt_iter=7, mel_names=names, mel_path=str(mdir), exp_root=root)

"""GPU: the objective metrics through the command-line tools -- ``python -m diffwave_sashimi_amd.evaluate`` on wav
directories, ``+generate.report_metrics=true`` and the ``val/*`` keys of a training run's log."""
import json
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import spectral_reference as ref

pytestmark = pytest.mark.gpu


def test_evaluate_directories_against_float64(tmp_path, gpu, capsys):
    """Three pairs of different lengths in two batches, one generated file with the ``0k_`` prefix, the generated wavs
    float32 and up to a hop longer than their int16 recordings."""
    from scipy.io import wavfile
    from diffwave_sashimi_amd import evaluate
    g, r = tmp_path / "gen", tmp_path / "ref"
    os.makedirs(g)
    os.makedirs(r)
    want = {}
    for stem, gname, n_ref, n_gen in (("LJ001-0001", "0k_LJ001-0001", 4000, 4096), ("b", "b", 2500, 2500),
                                      ("c", "c", 1300, 1536)):
        x, y = ref.signal_pair("noise", n_gen)
        y16 = (y[:n_ref] * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
        wavfile.write(str(g / f"{gname}.wav"), 22050, x.numpy())
        wavfile.write(str(r / f"{stem}.wav"), 22050, y16.numpy())
        want[gname + ".wav"] = ref.metrics(x[:n_ref], y16.float() / 32768.0)
    out = tmp_path / "m.json"
    rows = evaluate.main(["--generated", str(g), "--reference", str(r), "--batch-size", "2", "--json", str(out)])
    printed = capsys.readouterr().out
    rec = json.load(open(out))
    assert [f["generated"] for f in rec["files"]] == sorted(want) and len(rows) == 3
    assert [f["samples"] for f in rec["files"]] == [4000, 2500, 1300]
    for f in rec["files"]:
        for key, v in want[f["generated"]].items():
            assert ref.close(f[key], v, key), (f["generated"], key, f[key], v)
    for key in ref.HEADLINE:
        assert abs(rec["summary"][key]["mean"] - np.mean([w[key] for w in want.values()])) < 1e-4
        assert rec["summary"][key]["n"] == 3 and key in printed
    assert "unpaired" not in printed


def test_generate_and_train_report_metrics(tmp_path, gpu, capsys):
    """wn_cond_c64 from seeded weights, ddim over 4 of T = 50 steps, wavs of about 1100 samples."""
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import generate, local_path_name
    from diffwave_sashimi_amd.metrics import METRICS, spectral_metrics
    from diffwave_sashimi_amd.train import train
    cfg = dict(cases.WAVENET_COND_CASES["wn_cond_c64"][0])
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=None)
    data = tmp_path / "wavs"
    os.makedirs(data)
    rng = np.random.default_rng(3)
    src = {}
    for stem, n in (("a", 1100), ("b", 1300)):
        src[stem] = (rng.standard_normal(n) * 3000).astype(np.int16)
        wavfile.write(str(data / f"{stem}.wav"), 22050, src[stem])
    ds = dict(_name_="ljspeech", data_path=str(data), segment_length=768, sampling_rate=22050, filter_length=1024,
              hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0)
    root = str(tmp_path / "exp")
    gen = dict(ckpt_iter="init", n_samples=2, mel_name="a", sampler="ddim", steps=4, seed=5, exp_root=root)

    rows = []
    torch.manual_seed(3)
    audio = generate(0, diff, dict(cfg), ds, report_metrics=True, metric_rows=rows, **gen)
    out = capsys.readouterr().out
    assert out.count("batch 0 metrics: mr_stft = ") == 1 and "mcd = " in out
    assert tuple(audio.shape) == (2, 1, 1280) and len(rows) == 2
    y = torch.from_numpy(src["a"].astype(np.float32) / 32768.0).to(gpu)[None].expand(2, -1)
    want = spectral_metrics(audio[:, :, :1100], y)
    for b, row in enumerate(rows):
        assert row["name"] == "a" and row["clip"] == b
        for key, v in want.items():
            assert row[key] == float(v[b]), (b, key)
        assert all(np.isfinite(row[k]) and row[k] > 0 for k in METRICS)
    torch.manual_seed(3)
    plain = generate(0, diff, dict(cfg), ds, **gen)
    assert torch.equal(plain, audio)                                        # the key changes no sample
    assert "metrics:" not in capsys.readouterr().out                        # and without it nothing is printed

    # ---- ragged runs: every utterance against its own source
    rows = []
    torch.manual_seed(3)
    clips = generate(0, diff, dict(cfg), ds, report_metrics=True, metric_rows=rows,
                     **dict(gen, mel_name=None, mel_names=["a", "b"], n_samples=1))
    assert capsys.readouterr().out.count("batch 0 metrics: ") == 1
    assert [row["name"] for row in rows] == ["b", "a"]                      # longest first, as the batch ran
    for row in rows:
        n = src[row["name"]].shape[0]
        k = ["a", "b"].index(row["name"])
        yk = torch.from_numpy(src[row["name"]].astype(np.float32) / 32768.0).to(gpu)[None]
        alone = spectral_metrics(clips[k][:, :n], yk)
        for key, v in alone.items():
            assert row[key] == float(v[0]), (row["name"], key)               # a clip's numbers do not depend on its batch

    # ---- a two-iteration training run logs the means at the iterations it generates
    train(0, 1, diffusion_cfg=diff, model_cfg=dict(cfg), dataset_cfg=ds,
          generate_cfg={"n_samples": 1, "mel_name": "a", "sampler": "ddim", "steps": 4, "seed": 1, "report_metrics": True},
          ckpt_iter=-1, n_iters=1, iters_per_ckpt=1, iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=2,
          exp_root=root, num_workers=0)
    log = os.path.join(root, local_path_name(None, cfg, diff, ds), "train_log.jsonl")
    records = [json.loads(line) for line in open(log)]
    val = [rec for rec in records if "val/mr_stft" in rec]
    assert [rec["step"] for rec in val] == [0, 1]
    for rec in val:
        assert sorted(k for k in rec if k.startswith("val/")) == ["val/ls_mae", "val/lsd", "val/mcd", "val/mr_stft"]
        assert all(np.isfinite(rec["val/" + k]) and rec["val/" + k] > 0 for k in METRICS)
    assert sum("val/audio" in rec for rec in records) == 2

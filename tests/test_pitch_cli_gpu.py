"""GPU: the pitch metrics through the command-line tools -- ``evaluate --pitch``, ``+generate.report_pitch=true`` and the
``val/*`` keys of a training run's log.  Models run from seeded random weights: their output is noise, so the F0 keys
may legitimately be absent or NaN there; only the keys that are always finite are asserted on them."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import pitch_reference as ref

pytestmark = pytest.mark.gpu

ALWAYS = ("vuv_error", "periodicity_rmse")


def test_evaluate_pitch_rows_are_pitch_metrics_of_the_files(tmp_path, gpu, capsys):
    """Two pairs with voiced frames and one pair of noise (no frame voiced in both: its F0 numbers are NaN and it is
    left out of their means)."""
    from scipy.io import wavfile
    from diffwave_sashimi_amd import evaluate
    from diffwave_sashimi_amd.metrics import METRICS, PITCH_METRICS, pitch_metrics
    g, r = tmp_path / "gen", tmp_path / "ref"
    os.makedirs(g)
    os.makedirs(r)
    x, y, _ = ref.signal_pair("A")
    rng = np.random.default_rng(7)
    noise = (0.1 * rng.standard_normal(3000)).astype(np.float32)
    clips = {"0k_a": (x[:6000], y[:6000], "a"), "b": (x[9000:14000], y[9000:14000], "b"),
             "c": (noise, noise[::-1].copy(), "c")}
    want = {}
    for gname, (xc, yc, stem) in clips.items():
        wavfile.write(str(g / f"{gname}.wav"), 22050, xc)
        wavfile.write(str(r / f"{stem}.wav"), 22050, yc)
        m = pitch_metrics(torch.from_numpy(xc).to(gpu)[None], torch.from_numpy(yc).to(gpu)[None], win=512, fmin=60.0)
        want[gname + ".wav"] = {k: float(m[k][0]) for k in PITCH_METRICS}
    out = tmp_path / "m.json"
    base = ["--generated", str(g), "--reference", str(r), "--batch-size", "2"]
    rows = evaluate.main(base + ["--json", str(out), "--pitch", "--pitch-win", "512", "--pitch-fmin", "60"])
    printed = capsys.readouterr().out
    assert "NaN" not in open(out).read()                                    # strict JSON: an undefined value is null
    rec = json.load(open(out))
    assert rec["pitch"] == dict(sampling_rate=22050, hop=256, win=512, fmin=60.0, fmax=550.0, threshold=0.15)
    assert [f["generated"] for f in rec["files"]] == sorted(want) and len(rows) == 3
    for f in rec["files"]:
        for k, v in want[f["generated"]].items():
            assert f[k] == v or (math.isnan(v) and f[k] is None), (f["generated"], k, f[k], v)
    assert math.isnan(rows[2]["f0_rmse"])                                   # the returned rows keep the NaN
    assert math.isnan(want["c.wav"]["f0_rmse"]) and not math.isnan(want["b.wav"]["f0_rmse"])
    for k in PITCH_METRICS:
        finite = [w[k] for w in want.values() if math.isfinite(w[k])]
        assert rec["summary"][k]["n"] == len(finite)
        assert abs(rec["summary"][k]["mean"] - np.mean(finite)) < 1e-12
    assert rec["summary"]["f0_rmse"]["n"] == 2 and rec["summary"]["vuv_error"]["n"] == 3
    lines = [line.split()[0] for line in printed.splitlines()[1:]]
    assert lines[-6:] == list(PITCH_METRICS) and lines.index("mcd") < lines.index("f0_rmse")

    # ---- without --pitch: the table and the JSON keys of before
    plain_json = tmp_path / "plain.json"
    evaluate.main(base + ["--json", str(plain_json)])
    plain = capsys.readouterr().out
    assert plain.splitlines() == printed.splitlines()[:-6]
    assert not any(k in plain for k in PITCH_METRICS)
    prec = json.load(open(plain_json))
    assert sorted(prec) == ["files", "stft", "summary", "unpaired_generated", "unpaired_reference"]
    assert not set(PITCH_METRICS) & set(prec["summary"]) and not set(PITCH_METRICS) & set(prec["files"][0])
    assert all(k in prec["summary"] for k in METRICS)
    assert {k: v for k, v in rec["summary"].items() if k not in PITCH_METRICS} == prec["summary"]


def test_generate_and_train_report_pitch(tmp_path, gpu, capsys):
    """wn_cond_c64 from seeded weights, ddim over 4 of T = 50 steps, source wavs that hold a tone."""
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import generate, local_path_name
    from diffwave_sashimi_amd.metrics import METRICS, PITCH_METRICS, pitch_metrics
    from diffwave_sashimi_amd.train import train
    cfg = dict(cases.WAVENET_COND_CASES["wn_cond_c64"][0])
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=None)
    data = tmp_path / "wavs"
    os.makedirs(data)
    rng = np.random.default_rng(3)
    src = {}
    for stem, n in (("a", 1100), ("b", 1300)):
        v = ref.tone(n, 140.0, 22050, rng)[0] * 32768.0 + rng.standard_normal(n) * 30.0
        src[stem] = v.astype(np.int16)
        wavfile.write(str(data / f"{stem}.wav"), 22050, src[stem])
    ds = dict(_name_="ljspeech", data_path=str(data), segment_length=768, sampling_rate=22050, filter_length=1024,
              hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0)
    root = str(tmp_path / "exp")
    gen = dict(ckpt_iter="init", n_samples=2, mel_name="a", sampler="ddim", steps=4, seed=5, exp_root=root)

    rows = []
    torch.manual_seed(3)
    audio = generate(0, diff, dict(cfg), ds, report_pitch=True, metric_rows=rows, **gen)
    out = capsys.readouterr().out
    assert out.count("batch 0 pitch: f0_rmse = ") == 1 and " Hz  f0_cents = " in out and "periodicity_rmse = " in out
    assert "batch 0 metrics:" not in out
    assert len(rows) == 2
    y = torch.from_numpy(src["a"].astype(np.float32) / 32768.0).to(gpu)[None].expand(2, -1)
    want = pitch_metrics(audio[:, :, :1100], y)
    assert int(want["frames"][0]) == 5
    for b, row in enumerate(rows):
        assert row["name"] == "a" and row["clip"] == b and sorted(row) == sorted(PITCH_METRICS + ("name", "clip"))
        for k in PITCH_METRICS:
            v = float(want[k][b])
            assert row[k] == v or (math.isnan(v) and math.isnan(row[k])), (b, k)
        assert all(np.isfinite(row[k]) for k in ALWAYS)
    torch.manual_seed(3)
    plain = generate(0, diff, dict(cfg), ds, **gen)
    assert torch.equal(plain, audio)                                        # the key changes no sample
    assert "pitch:" not in capsys.readouterr().out                          # and without it nothing is printed

    # ---- a source too short for the tracker is refused before anything is sampled (700 < 734 samples)
    wavfile.write(str(data / "s.wav"), 22050, src["a"][:700])
    for short in (dict(mel_name="s"), dict(mel_name=None, mel_names=["a", "s"], n_samples=1)):
        with pytest.raises(ValueError, match=r"generate.report_pitch \(s.wav\): clip 0 has 700 samples"):
            generate(0, diff, dict(cfg), ds, report_pitch=True, **dict(gen, **short))
        assert "batch 0" not in capsys.readouterr().out

    # ---- with report_metrics: one dict per clip holds both families; ragged: every utterance against its own source
    rows = []
    torch.manual_seed(3)
    generate(0, diff, dict(cfg), ds, report_metrics=True, report_pitch=True, metric_rows=rows,
             **dict(gen, mel_name=None, mel_names=["a", "b"], n_samples=1))
    out = capsys.readouterr().out
    assert out.count("batch 0 metrics: ") == 1 and out.count("batch 0 pitch: ") == 1
    assert out.index("batch 0 metrics: ") < out.index("batch 0 pitch: ")
    assert [row["name"] for row in rows] == ["b", "a"]
    for row in rows:
        assert all(k in row for k in METRICS + PITCH_METRICS)
        assert all(np.isfinite(row[k]) for k in METRICS + ALWAYS)

    # ---- a two-iteration training run logs the keys that are defined
    train(0, 1, diffusion_cfg=diff, model_cfg=dict(cfg), dataset_cfg=ds,
          generate_cfg={"n_samples": 1, "mel_name": "a", "sampler": "ddim", "steps": 4, "seed": 1, "report_pitch": True},
          ckpt_iter=-1, n_iters=1, iters_per_ckpt=1, iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=2,
          exp_root=root, num_workers=0)
    log = os.path.join(root, local_path_name(None, cfg, diff, ds), "train_log.jsonl")
    records = [json.loads(line) for line in open(log)]
    val = [rec for rec in records if "val/vuv_error" in rec]
    assert [rec["step"] for rec in val] == [0, 1]
    for rec in val:
        keys = {k[4:] for k in rec if k.startswith("val/")}
        assert set(ALWAYS) <= keys <= set(PITCH_METRICS) and "mr_stft" not in keys
        assert all(np.isfinite(rec["val/" + k]) for k in keys)
    assert sum("val/audio" in rec for rec in records) == 2

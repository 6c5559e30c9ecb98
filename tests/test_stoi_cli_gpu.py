"""GPU: the intelligibility metrics through the command-line tools -- ``evaluate --stoi`` and ``--resample``,
``+generate.report_stoi=true`` and the ``val/stoi`` / ``val/estoi`` keys of a training run's log.  Models run from seeded
random weights: their output is noise, so only that the numbers are those of ``metrics.stoi`` is asserted on them."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import stoi_reference as ref

pytestmark = pytest.mark.gpu


def _int16(v):
    return np.round(np.asarray(v, dtype=np.float64) * 32767.0).astype(np.int16)


def test_evaluate_stoi_rows_and_resample(tmp_path, gpu, capsys):
    """A float32 generated set against an int16 reference set: two pairs with segments and one too short to have any
    (its values are NaN, ``null`` in the JSON, and it is left out of the means)."""
    from scipy.io import wavfile
    from diffwave_sashimi_amd import audio, evaluate
    from diffwave_sashimi_amd.metrics import METRICS, PITCH_METRICS, STOI_DEFAULTS, STOI_METRICS, stoi
    g, r = tmp_path / "gen", tmp_path / "ref"
    os.makedirs(g)
    os.makedirs(r)
    sr, y, xs = ref.signal_set("A")
    clips = {"0k_a": (xs[1], _int16(y), "a"), "b": (xs[2][:20000], _int16(y[:20100]), "b"),
             "c": (xs[0][:3000], _int16(y[:3000]), "c")}
    want = {}
    for gname, (xc, yc, stem) in clips.items():
        wavfile.write(str(g / f"{gname}.wav"), sr, xc)
        wavfile.write(str(r / f"{stem}.wav"), sr, yc)
        n = min(len(xc), len(yc))
        m = stoi(torch.from_numpy(xc[:n]).to(gpu)[None], torch.from_numpy(yc[:n].astype(np.float32) / 32768.0).to(gpu)[None],
                 sampling_rate=sr)
        want[gname + ".wav"] = {k: float(m[k][0]) for k in STOI_METRICS}
    assert math.isnan(want["c.wav"]["stoi"]) and 0.5 < want["b.wav"]["stoi"] < want["0k_a.wav"]["stoi"] < 1.0
    out = tmp_path / "m.json"
    base = ["--generated", str(g), "--reference", str(r), "--batch-size", "2"]
    rows = evaluate.main(base + ["--json", str(out), "--stoi", "--pitch"])
    printed = capsys.readouterr().out
    assert "NaN" not in open(out).read()                                    # strict JSON: an undefined value is null
    rec = json.load(open(out))
    assert rec["stoi"] == dict(STOI_DEFAULTS, sampling_rate=sr) and "converted" not in rec
    assert [f["generated"] for f in rec["files"]] == sorted(want) and len(rows) == 3
    for f in rec["files"]:
        for k, v in want[f["generated"]].items():
            assert f[k] == v or (math.isnan(v) and f[k] is None), (f["generated"], k, f[k], v)
    assert math.isnan(rows[2]["stoi"]) and math.isnan(rows[2]["estoi"])      # the returned rows keep the NaN
    for k in STOI_METRICS:
        finite = [w[k] for w in want.values() if math.isfinite(w[k])]
        assert rec["summary"][k]["n"] == len(finite) == 2
        assert abs(rec["summary"][k]["mean"] - np.mean(finite)) < 1e-12
    lines = [line.split()[0] for line in printed.splitlines()[1:]]
    assert lines[-2:] == list(STOI_METRICS) and lines[-8:-2] == list(PITCH_METRICS)      # after the pitch rows
    assert lines.index("mcd") < lines.index("f0_rmse") < lines.index("stoi")
    assert "converted to" not in printed

    # ---- --stoi alone: after the spectral rows; without it: the table and the JSON keys of before
    evaluate.main(base + ["--stoi"])
    alone = capsys.readouterr().out
    lines = [line.split()[0] for line in alone.splitlines()[1:]]
    assert lines[-2:] == list(STOI_METRICS) and lines[-3] == "mcd"
    plain_json = tmp_path / "plain.json"
    evaluate.main(base + ["--json", str(plain_json)])
    plain = capsys.readouterr().out
    assert plain.splitlines() == alone.splitlines()[:-2]
    prec = json.load(open(plain_json))
    assert sorted(prec) == ["files", "stft", "summary", "unpaired_generated", "unpaired_reference"]
    assert not set(STOI_METRICS) & set(prec["summary"]) and not set(STOI_METRICS) & set(prec["files"][0])
    assert {k: v for k, v in rec["summary"].items() if k in METRICS} == {k: prec["summary"][k] for k in METRICS}

    # ---- a reference directory at 16000 Hz: refused with the old message, converted with --resample
    sr16, y16, _ = ref.signal_set("B")
    g2, r2 = tmp_path / "gen2", tmp_path / "ref16"
    os.makedirs(g2)
    os.makedirs(r2)
    x22 = xs[1][:22050 + 100]                                # within one hop of the converted reference's 22050 samples
    wavfile.write(str(g2 / "u.wav"), sr, x22)
    wavfile.write(str(r2 / "u.wav"), sr16, _int16(y16))
    base2 = ["--generated", str(g2), "--reference", str(r2)]
    with pytest.raises(ValueError, match=r"u\.wav has sampling rate 16000, expected 22050"):
        evaluate.main(base2 + ["--stoi"])
    capsys.readouterr()
    out2 = tmp_path / "m2.json"
    rows = evaluate.main(base2 + ["--stoi", "--resample", "--json", str(out2)])
    printed = capsys.readouterr().out
    assert "converted to 22050 Hz: 1 files" in printed
    y_conv, lens = audio.resample(torch.from_numpy(_int16(y16).astype(np.float32) / 32768.0).to(gpu)[None], sr16, sr)
    assert lens == [22050]
    m = stoi(torch.from_numpy(x22[:22050]).to(gpu)[None], y_conv, sampling_rate=sr)
    assert rows[0]["stoi"] == float(m["stoi"][0]) and rows[0]["estoi"] == float(m["estoi"][0])
    rec2 = json.load(open(out2))
    assert rec2["converted"] == ["u.wav"] and rec2["files"][0]["samples"] == 22050
    # a pair more than one hop apart AFTER the conversion is still refused
    wavfile.write(str(g2 / "u.wav"), sr, xs[1][:22050 + 300])
    with pytest.raises(ValueError, match="more than one hop"):
        evaluate.main(base2 + ["--resample"])


def test_generate_and_train_report_stoi(tmp_path, gpu, capsys):
    """wn_cond_c64 from seeded weights, ddim over 4 of T = 50 steps; the source wavs hold a tone in noise, long enough for
    a segment (9300 samples at 22050 Hz are 4218 at 10 kHz: 31 frames, all kept)."""
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import generate, local_path_name
    from diffwave_sashimi_amd.metrics import METRICS, STOI_METRICS, stoi
    from diffwave_sashimi_amd.train import train
    cfg = dict(cases.WAVENET_COND_CASES["wn_cond_c64"][0])
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=None)
    data = tmp_path / "wavs"
    os.makedirs(data)
    rng = np.random.default_rng(3)
    src = {}
    for stem, n in (("a", 9300), ("b", 9900)):
        v = 0.3 * np.sin(2 * np.pi * 140.0 * np.arange(n) / 22050) * 32768.0 + rng.standard_normal(n) * 300.0
        src[stem] = v.astype(np.int16)
        wavfile.write(str(data / f"{stem}.wav"), 22050, src[stem])
    ds = dict(_name_="ljspeech", data_path=str(data), segment_length=768, sampling_rate=22050, filter_length=1024,
              hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0)
    root = str(tmp_path / "exp")
    gen = dict(ckpt_iter="init", n_samples=2, mel_name="a", sampler="ddim", steps=4, seed=5, exp_root=root)

    rows = []
    torch.manual_seed(3)
    audio = generate(0, diff, dict(cfg), ds, report_stoi=True, metric_rows=rows, **gen)
    out = capsys.readouterr().out
    assert out.count("batch 0 intelligibility: stoi = ") == 1 and "  estoi = " in out
    assert "batch 0 metrics:" not in out and "pitch:" not in out
    assert len(rows) == 2
    y = torch.from_numpy(src["a"].astype(np.float32) / 32768.0).to(gpu)[None].expand(2, -1)
    want = stoi(audio[:, :, :9300], y)
    assert want["frames_kept"].tolist() == [31.0, 31.0] and want["segments"].tolist() == [2.0, 2.0]
    for b, row in enumerate(rows):
        assert row["name"] == "a" and row["clip"] == b and sorted(row) == sorted(STOI_METRICS + ("name", "clip"))
        for k in STOI_METRICS:
            assert row[k] == float(want[k][b]) and np.isfinite(row[k]), (b, k)
    torch.manual_seed(3)
    plain = generate(0, diff, dict(cfg), ds, **gen)
    assert torch.equal(plain, audio)                                        # the key changes no sample
    assert "intelligibility" not in capsys.readouterr().out                 # and without it nothing is printed

    # ---- a source shorter than one frame at 10 kHz is refused before anything is sampled (562 samples are 255)
    wavfile.write(str(data / "s.wav"), 22050, src["a"][:562])
    with pytest.raises(ValueError, match=r"generate.report_stoi \(s.wav\): clip 0 has 562 samples"):
        generate(0, diff, dict(cfg), ds, report_stoi=True, **dict(gen, mel_name="s"))
    assert "batch 0" not in capsys.readouterr().out

    # ---- with the other two reports: one dict per clip holds all three families; ragged batches
    rows = []
    torch.manual_seed(3)
    generate(0, diff, dict(cfg), ds, report_metrics=True, report_pitch=True, report_stoi=True, metric_rows=rows,
             **dict(gen, mel_name=None, mel_names=["a", "b"], n_samples=1))
    out = capsys.readouterr().out
    assert out.index("batch 0 metrics: ") < out.index("batch 0 pitch: ") < out.index("batch 0 intelligibility: ")
    assert [row["name"] for row in rows] == ["b", "a"]
    for row in rows:
        assert all(k in row and np.isfinite(row[k]) for k in METRICS + STOI_METRICS) and "vuv_error" in row

    # ---- a two-iteration training run logs the two keys
    train(0, 1, diffusion_cfg=diff, model_cfg=dict(cfg), dataset_cfg=ds,
          generate_cfg={"n_samples": 1, "mel_name": "a", "sampler": "ddim", "steps": 4, "seed": 1, "report_stoi": True},
          ckpt_iter=-1, n_iters=1, iters_per_ckpt=1, iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=2,
          exp_root=root, num_workers=0)
    log = os.path.join(root, local_path_name(None, cfg, diff, ds), "train_log.jsonl")
    records = [json.loads(line) for line in open(log)]
    val = [rec for rec in records if "val/stoi" in rec]
    assert [rec["step"] for rec in val] == [0, 1]
    for rec in val:
        keys = {k[4:] for k in rec if k.startswith("val/")}
        assert keys == set(STOI_METRICS) and all(np.isfinite(rec["val/" + k]) for k in keys)

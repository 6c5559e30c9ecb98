"""GPU: mel inversion through the command-line tools -- ``+generate.start_griffinlim=N`` (the warm start from the
conditioning mel) and ``evaluate --griffin-lim N`` (the baseline rows).  The model runs from seeded random weights: its
output is noise, so only that the samples are those of the Python calls is asserted on them."""
import json
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import stoi_reference as ref

pytestmark = pytest.mark.gpu

DIFF = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=None)


def _dataset(tmp_path):
    from scipy.io import wavfile
    data = tmp_path / "wavs"
    os.makedirs(data)
    rng = np.random.default_rng(3)
    for stem, n in (("a", 1100), ("b", 900)):
        wavfile.write(str(data / f"{stem}.wav"), 22050, (rng.standard_normal(n) * 3000).astype(np.int16))
    return dict(_name_="ljspeech", data_path=str(data), segment_length=768, sampling_rate=22050, filter_length=1024,
                hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0)


def _mel_of(ds, stem):
    from diffwave_sashimi_amd.mel import Mel2Samp, load_wav_to_torch
    keys = ("filter_length", "hop_length", "win_length", "sampling_rate", "mel_fmin", "mel_fmax")
    m2s = Mel2Samp(**{k: ds[k] for k in keys})
    audio, _ = load_wav_to_torch(os.path.join(ds["data_path"], f"{stem}.wav"))
    return m2s.stft, m2s.get_mel(audio).unsqueeze(0)


def _with_last_frame_repeated(mel):
    return torch.cat([mel, mel[..., -1:]], dim=-1)


def test_generate_warm_start_from_the_conditioning_mel(tmp_path, gpu, capsys):
    from scipy.io import wavfile
    from diffwave_sashimi_amd import sampling as smp
    from diffwave_sashimi_amd.generate import generate
    from diffwave_sashimi_amd.models import construct_model
    cfg = dict(cases.WAVENET_COND_CASES["wn_cond_c64"][0])
    ds = _dataset(tmp_path)
    root = str(tmp_path / "exp")
    gen = dict(ckpt_iter="init", n_samples=2, mel_name="a", seed=5, exp_root=root)
    dh = smp.calc_diffusion_hyperparams(50, 1e-4, 0.05)

    # ---- one utterance, two clips: the wavs are the Python call with mel_to_audio as x_start
    torch.manual_seed(3)
    written = []
    audio = generate(0, DIFF, dict(cfg), ds, start_griffinlim=8, start_step=20, written=written, **gen)
    assert "start: Griffin-Lim estimate of the conditioning mel (8 iterations, momentum 0)" in capsys.readouterr().out
    torch.manual_seed(3)
    net = construct_model(dict(cfg)).cuda().eval()
    stft, mel = _mel_of(ds, "a")
    L = int(mel.shape[-1]) * 256
    x0 = stft.mel_to_audio(_with_last_frame_repeated(mel), n_iters=8)
    assert tuple(x0.shape) == (1, L)
    want = smp.sampling(net, (2, 1, L), dh, mel, x_start=x0[:, None, :], start_step=20, seed=5)
    assert torch.equal(audio, want) and bool(torch.isfinite(audio).all())
    for k, f in enumerate(written):
        assert np.array_equal(wavfile.read(f)[1], want[k, 0].cpu().numpy())
    torch.manual_seed(3)
    fast = generate(0, DIFF, dict(cfg), ds, start_griffinlim=8, griffinlim_momentum=0.99, start_step=20, start_noise=False,
                    **gen)
    x1 = stft.mel_to_audio(_with_last_frame_repeated(mel), n_iters=8, momentum=0.99)
    want = smp.sampling(net, (2, 1, L), dh, mel, x_start=x1[:, None, :], start_step=20, start_noise=False, seed=5)
    assert torch.equal(fast, want) and not torch.equal(fast, audio)

    # ---- two utterances of different length: every clip inverted at its own length
    torch.manual_seed(3)
    clips = generate(0, DIFF, dict(cfg), ds, start_griffinlim=8, start_step=20,
                     **dict(gen, mel_name=None, mel_names=["a", "b"], n_samples=1))
    _, mel_b = _mel_of(ds, "b")
    fa, fb = int(mel.shape[-1]), int(mel_b.shape[-1])
    assert fa > fb
    cond = torch.zeros(2, mel.shape[1], fa, device=gpu)
    cond[0], cond[1, :, :fb] = mel[0], mel_b[0]
    ext = torch.zeros(2, mel.shape[1], fa + 1, device=gpu)
    ext[0], ext[1, :, :fb + 1] = _with_last_frame_repeated(mel)[0], _with_last_frame_repeated(mel_b)[0]
    lens = [fa * 256, fb * 256]
    xs = stft.mel_to_audio(ext, n_iters=8, lengths=lens)
    assert torch.equal(xs[1, :lens[1]], stft.mel_to_audio(_with_last_frame_repeated(mel_b), n_iters=8)[0])   # as alone
    want = smp.sampling(net, (2, 1, lens[0]), dh, cond, x_start=xs[:, None, :], start_step=20, seed=5, lengths=lens)
    assert torch.equal(clips[0], want[0, :, :lens[0]]) and torch.equal(clips[1], want[1, :, :lens[1]])

    # ---- without the key nothing changes: the call of before, and the keyword left at its default
    capsys.readouterr()
    torch.manual_seed(3)
    plain = generate(0, DIFF, dict(cfg), ds, **gen)
    torch.manual_seed(3)
    same = generate(0, DIFF, dict(cfg), ds, start_griffinlim=None, griffinlim_momentum=None, **gen)
    assert torch.equal(plain, same) and not torch.equal(plain, audio)
    assert "Griffin-Lim" not in capsys.readouterr().out


def test_generate_refusals_come_before_a_model_is_built(tmp_path, gpu, monkeypatch):
    from diffwave_sashimi_amd import generate as gen_mod
    from diffwave_sashimi_amd import models
    cfg = dict(cases.WAVENET_COND_CASES["wn_cond_c64"][0])
    ds = _dataset(tmp_path)

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(models, "construct_model", no_model)        # generate imports it from there when it runs
    base = dict(ckpt_iter="init", n_samples=1, mel_name="a", seed=5, exp_root=str(tmp_path / "exp"), start_step=20)
    cases_ = [
        (dict(model=dict(cfg, unconditional=True), mel_name=None), "needs a mel-conditional run"),
        (dict(mel_name=None), "needs a mel-conditional run"),
        (dict(start_name="a"), "exclude each other"),
        (dict(start_step=None), "needs generate.start_step"),
        (dict(mel_path=str(tmp_path)), "does not combine with generate.mel_path"),
        (dict(model=dict({k: v for k, v in cfg.items() if k not in ("in_channels", "out_channels")}, mel_upsample=[8, 8],
                         subbands=4)), "start_griffinlim does not combine with model.subbands"),
        (dict(start_griffinlim=4097), "n_iters = 4097"),
        (dict(start_griffinlim=-1), "n_iters = -1"),
        (dict(start_griffinlim=2.5), "n_iters = 2.5"),
        (dict(griffinlim_momentum=1.0), "momentum = 1.0"),
    ]
    for change, match in cases_:
        kw = dict(base, start_griffinlim=8)
        kw.update({k: v for k, v in change.items() if k != "model"})
        with pytest.raises(ValueError, match=match):
            gen_mod.generate(0, DIFF, dict(change.get("model", cfg)), ds, **kw)
    with pytest.raises(ValueError, match="griffinlim_momentum belongs to generate.start_griffinlim"):
        gen_mod.generate(0, DIFF, dict(cfg), ds, griffinlim_momentum=0.5, **dict(base, start_step=None))


def test_evaluate_baseline_rows(tmp_path, gpu, capsys):
    from scipy.io import wavfile
    from diffwave_sashimi_amd import evaluate
    from diffwave_sashimi_amd.mel import TacotronSTFT
    from diffwave_sashimi_amd.metrics import METRICS, spectral_metrics
    g, r = tmp_path / "gen", tmp_path / "ref"
    os.makedirs(g)
    os.makedirs(r)
    sr, y, xs = ref.signal_set("A")
    pairs = {"0k_a": (xs[1], y, "a"), "b": (xs[2][:20000], y[:20100], "b")}
    stft = TacotronSTFT()
    want = {}
    for gname, (xc, yc, stem) in pairs.items():
        wavfile.write(str(g / f"{gname}.wav"), sr, xc)
        wavfile.write(str(r / f"{stem}.wav"), sr, yc)
        n = min(len(xc), len(yc)) // 256 * 256
        yd = torch.from_numpy(yc[:n]).to(gpu)[None]
        m = spectral_metrics(stft.mel_to_audio(stft.mel_spectrogram(yd), n_iters=4), yd, stft=stft)
        want[gname + ".wav"] = {k: float(v[0]) for k, v in m.items()}
    base = ["--generated", str(g), "--reference", str(r), "--batch-size", "2"]
    out = tmp_path / "m.json"
    evaluate.main(base + ["--griffin-lim", "4", "--json", str(out)])
    printed = capsys.readouterr().out.splitlines()
    rec = json.load(open(out))
    assert rec["griffin_lim"]["n_iters"] == 4 and rec["griffin_lim"]["momentum"] == 0.0
    for f in rec["files"]:
        for k, v in want[f["generated"]].items():
            assert f["baseline_" + k] == v, (f["generated"], k)
        assert f["baseline_mr_stft"] != f["mr_stft"]
    for k in METRICS:
        assert abs(rec["griffin_lim"]["summary"][k]["mean"] - np.mean([w[k] for w in want.values()])) < 1e-12
    head = printed.index("griffin-lim baseline (4 iterations)")
    assert printed[head + 1] == printed[0] and len(printed) == 2 * head + 1        # the same table once more
    assert [line.split()[0] for line in printed[head + 2:]] == [line.split()[0] for line in printed[1:head]]

    # ---- without the flag: the output and the JSON of before
    plain_json = tmp_path / "plain.json"
    evaluate.main(base + ["--json", str(plain_json)])
    assert capsys.readouterr().out.splitlines() == printed[:head]
    prec = json.load(open(plain_json))
    assert sorted(prec) == ["files", "stft", "summary", "unpaired_generated", "unpaired_reference"]
    assert not any("baseline" in k for f in prec["files"] for k in f)
    assert prec["files"] == [{k: v for k, v in f.items() if not k.startswith("baseline_")} for f in rec["files"]]
    assert prec["summary"] == rec["summary"]
    with pytest.raises(ValueError, match="--griffin-lim-momentum needs --griffin-lim"):
        evaluate.main(base + ["--griffin-lim-momentum", "0.5"])
    with pytest.raises(ValueError, match="n_iters = 5000"):
        evaluate.main(base + ["--griffin-lim", "5000"])
    evaluate.main(base + ["--griffin-lim", "2", "--griffin-lim-momentum", "0.99", "--stoi"])
    both = capsys.readouterr().out.splitlines()
    head = both.index("griffin-lim baseline (2 iterations)")
    assert both[head - 1].split()[0] == "estoi" == both[-1].split()[0]

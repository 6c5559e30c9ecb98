"""CPU: the float64 reference of the objective metrics obeys its identities, ``metrics`` checks its arguments before any
library call, and ``evaluate`` pairs, loads and trims wav files (the metric call stubbed: it needs a GPU)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import spectral_reference as ref


# ---- identities of the reference (1e-3: the floors 1e-7 and 1e-5 are the only departure; not a bound on the kernel)
def test_reference_half_gain_identities():
    x, y = ref.signal_pair("gain", 4000)
    m = ref.metrics(x, y)
    for r in ref.RESOLUTIONS:
        assert abs(m["sc_{}_{}_{}".format(*r)] - 0.5) < 1e-3
        assert abs(m["mag_{}_{}_{}".format(*r)] - math.log(2.0)) < 1e-3
    assert abs(m["mr_stft"] - (0.5 + math.log(2.0))) < 1e-3
    assert abs(m["ls_mae"] - math.log(2.0)) < 1e-3
    assert abs(m["lsd"] - 20.0 * math.log10(2.0) / 10.0) < 1e-3
    assert abs(m["mcd"]) < 1e-3


def test_reference_identical_signals_give_zero():
    _, y = ref.signal_pair("noise", 2500)
    assert all(v == 0.0 for v in ref.metrics(y, y).values())
    z = torch.zeros(1300)
    assert all(v == 0.0 for v in ref.metrics(z, z).values())


def test_cepstral_table_is_the_dct_rows_of_the_reference():
    from diffwave_sashimi_amd.metrics import cepstral_table
    D = cepstral_table(13, 80)
    assert D.dtype == torch.float64 and tuple(D.shape) == (13, 80)
    assert torch.allclose(D, ref.cepstral_table(13, 80), rtol=0, atol=1e-15)
    assert torch.allclose(D @ D.T, torch.eye(13, dtype=torch.float64), atol=1e-13)      # orthonormal rows
    assert float((D @ torch.ones(80, dtype=torch.float64)).abs().max()) < 1e-13         # blind to a level change


# ---- argument errors: all before a library call (the tensors are CPU tensors: a call that got that far would raise
# RuntimeError instead)
def test_argument_errors_come_before_any_library_call():
    from diffwave_sashimi_amd.metrics import spectral_metrics, spectral_sums
    x = torch.zeros(2, 4000)
    with pytest.raises(ValueError, match=r"n_fft=2048.*clip 0 has 1024 samples"):
        spectral_metrics(x[:, :1024], x[:, :1024])                     # one sample too short for n_fft = 2048
    with pytest.raises(ValueError, match=r"n_fft=512.*clip 1 has 256 samples"):
        spectral_metrics(x, x, [4000, 256], resolutions=((512, 50, 240),))
    with pytest.raises(ValueError, match="power of two"):
        spectral_metrics(x, x, resolutions=((1000, 120, 600),))
    with pytest.raises(ValueError, match="power of two"):
        spectral_metrics(x, x, resolutions=((4096, 120, 600),))
    with pytest.raises(ValueError, match="win must be"):
        spectral_metrics(x, x, resolutions=((512, 50, 600),))
    with pytest.raises(ValueError, match="hop must be"):
        spectral_sums(x, x, n_fft=512, hop=0, win=512)
    with pytest.raises(ValueError, match="lengths has 3 entries for a batch of 2"):
        spectral_metrics(x, x, [4000, 4000, 4000])
    with pytest.raises(ValueError, match="lengths"):
        spectral_metrics(x, x, [4000, 4001])
    with pytest.raises(ValueError, match="equal non-empty"):
        spectral_metrics(x, x[:, :3000])
    with pytest.raises(ValueError, match="n_cep"):
        spectral_metrics(x, x, n_cep=80)


def test_cpu_tensors_are_refused():
    from diffwave_sashimi_amd.metrics import spectral_metrics, spectral_sums
    x = torch.zeros(1, 1, 4000)
    with pytest.raises(RuntimeError, match="GPU only|no CPU fallback"):
        spectral_metrics(x, x)
    with pytest.raises(RuntimeError, match="GPU only|no CPU fallback"):
        spectral_sums(x, x, n_fft=512, hop=50, win=240)


def test_generate_refuses_report_metrics_without_a_source_wav(tmp_path):
    from diffwave_sashimi_amd.generate import generate
    from tests import cases
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="ljspeech", data_path=str(tmp_path), segment_length=768, sampling_rate=22050, hop_length=256)
    cond = dict(cases.WAVENET_COND_CASES["wn_cond_tiny"][0])
    with pytest.raises(ValueError, match="does not combine with generate.mel_path"):
        generate(0, diff, cond, ds, ckpt_iter="init", mel_name="a", mel_path=str(tmp_path), report_metrics=True,
                 exp_root=str(tmp_path))
    with pytest.raises(ValueError, match="needs a mel-conditional run"):
        generate(0, diff, dict(cases.WAVENET_CASES["wn_tiny"][0]), ds, ckpt_iter="init", report_metrics=True,
                 exp_root=str(tmp_path))
    with pytest.raises(ValueError, match="expected true or false"):
        generate(0, diff, cond, ds, ckpt_iter="init", mel_name="a", report_metrics="yes", exp_root=str(tmp_path))


# ---- evaluate: pairing, loading, trimming (metric call stubbed)
def _write(path, n, rate=22050, dtype=np.int16, seed=0):
    from scipy.io import wavfile
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) * 0.1
    wavfile.write(str(path), rate, (v * 32768).astype(np.int16) if dtype == np.int16 else v.astype(np.float32))
    return v


@pytest.fixture
def stubbed(monkeypatch):
    """``spectral_metrics`` replaced by a recorder that returns each clip's length as its only metric."""
    from diffwave_sashimi_amd import evaluate
    calls = []

    def fake(x, y, lengths, **kw):
        calls.append((x.clone(), y.clone(), list(lengths), kw))
        return {"mr_stft": torch.tensor([float(n) for n in lengths], dtype=torch.float64)}
    monkeypatch.setattr(evaluate._metrics, "spectral_metrics", fake)
    return calls


def test_evaluate_pairs_by_stem_and_prefix_and_trims(tmp_path, stubbed, capsys):
    from diffwave_sashimi_amd import evaluate
    g, r = tmp_path / "gen", tmp_path / "ref"
    os.makedirs(g)
    os.makedirs(r)
    _write(g / "0k_LJ001-0001.wav", 1280, dtype=np.float32, seed=1)      # prefixed, float, one hop-multiple long
    ya = _write(r / "LJ001-0001.wav", 1100, seed=2)
    _write(g / "b.wav", 2000, seed=3)
    _write(r / "b.wav", 2100, seed=4)
    _write(g / "3k_lonely.wav", 1500, seed=6)
    _write(r / "unused.wav", 1500, seed=7)
    out = tmp_path / "m.json"
    rows = evaluate.main(["--generated", str(g), "--reference", str(r), "--batch-size", "1", "--json", str(out)])
    printed = capsys.readouterr().out
    assert "unpaired generated files (1): 3k_lonely.wav" in printed
    assert "unpaired reference files (1): unused.wav" in printed
    assert [c[2] for c in stubbed] == [[2000], [1100]]                   # longest first, each trimmed to the shorter
    assert [row["mr_stft"] for row in rows] == [1100.0, 2000.0]          # reported in the order of the pairs
    x, y, _, kw = stubbed[1]
    assert tuple(x.shape) == (1, 1100) and x.dtype == torch.float32
    want = ((ya * 32768).astype(np.int16).astype(np.float32) / 32768.0)
    assert np.array_equal(y[0].numpy(), want)                            # int16 / 32768
    assert float(x.abs().max()) < 1.0 and float(x.abs().max()) > 0.01    # the float wav as it is
    assert kw["stft"].hop_length == 256
    rec = json.load(open(out))
    assert [(f["generated"], f["reference"], f["samples"]) for f in rec["files"]] == \
        [("0k_LJ001-0001.wav", "LJ001-0001.wav", 1100), ("b.wav", "b.wav", 2000)]
    assert rec["summary"]["mr_stft"]["n"] == 2 and rec["summary"]["mr_stft"]["mean"] == 1550.0
    assert rec["unpaired_generated"] == ["3k_lonely"] and rec["unpaired_reference"] == ["unused"]
    assert "mr_stft" in printed and "1550.000000" in printed
    with pytest.raises(ValueError, match="--strict"):
        evaluate.main(["--generated", str(g), "--reference", str(r), "--strict"])


def test_evaluate_prefers_the_plain_stem_and_refuses_a_double_claim(tmp_path):
    from diffwave_sashimi_amd.evaluate import pair_files
    g, r = tmp_path / "gen", tmp_path / "ref"
    os.makedirs(g)
    os.makedirs(r)
    for p in (g / "0k_a.wav", r / "0k_a.wav", r / "a.wav"):
        _write(p, 1100)
    assert pair_files(str(g), str(r)) == ([("0k_a", "0k_a")], [], ["a"])
    _write(g / "a.wav", 1100)
    _write(g / "1k_a.wav", 1100)
    with pytest.raises(ValueError, match="both pair with the reference a.wav"):
        pair_files(str(g), str(r))


def test_evaluate_refuses_rate_mismatch_and_distant_lengths(tmp_path, stubbed):
    from diffwave_sashimi_amd import evaluate
    g, r = tmp_path / "gen", tmp_path / "ref"
    os.makedirs(g)
    os.makedirs(r)
    _write(g / "a.wav", 1400)
    _write(r / "a.wav", 1400, rate=16000)
    with pytest.raises(ValueError, match="sampling rate 16000, expected 22050"):
        evaluate.main(["--generated", str(g), "--reference", str(r)])
    _write(r / "a.wav", 1400 + 257)
    with pytest.raises(ValueError, match="more than one hop"):
        evaluate.main(["--generated", str(g), "--reference", str(r)])
    _write(r / "a.wav", 1400 + 256)              # exactly one hop apart: trimmed
    evaluate.main(["--generated", str(g), "--reference", str(r)])
    assert stubbed[-1][2] == [1400]
    _write(r / "a.wav", 1400 + 300)
    evaluate.main(["--generated", str(g), "--reference", str(r), "--hop-length", "300"])
    assert stubbed[-1][2] == [1400] and stubbed[-1][3]["stft"].hop_length == 300


def test_evaluate_summary_statistics():
    from diffwave_sashimi_amd.evaluate import summarise
    s = summarise([{"m": 1.0}, {"m": 2.0}, {"m": 3.0}, {"m": 6.0}])["m"]
    assert s[0] == 3.0 and s[3] == 4
    assert abs(s[1] - math.sqrt(14.0 / 3.0)) < 1e-12 and abs(s[2] - 1.96 * s[1] / 2.0) < 1e-12
    assert summarise([{"m": 5.0}])["m"] == (5.0, 0.0, 0.0, 1)

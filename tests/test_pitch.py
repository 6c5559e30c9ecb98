"""CPU: the float64 reference of the pitch tracker finds what was put into its test signals, ``metrics`` checks the pitch
arguments before any library call, ``generate`` refuses ``report_pitch`` where it refuses ``report_metrics``, and
``evaluate`` parses the ``--pitch`` flags and summarises NaN-aware."""
import math

import numpy as np
import pytest
import torch

from tests import pitch_reference as ref


# ---- the reference on its own signals
@pytest.mark.parametrize("name", sorted(ref.PARAMS))
def test_reference_recovers_the_tones_and_leaves_noise_and_silence_unvoiced(name):
    _, _, segments, _, (f0, per, voiced, _) = ref.reference_tracks(name)
    p = ref.PARAMS[name]
    S = ref.frame_size(**p)
    assert len(f0) == ref.SAMPLES[name] // p["hop"] + 1
    seen = set()
    for seg in segments:
        inside = ref.frames_inside(seg, p["hop"], S, len(f0))
        assert inside, seg
        kind, want = seg[2], seg[3]
        seen.add(kind)
        if kind == "tone":
            assert voiced[inside].all()
            assert np.abs(f0[inside] - want).max() < 0.5, (name, want, f0[inside])
            assert per[inside].min() > 0.99
        elif kind == "vibrato":                           # 5 Hz, +-3 %
            assert voiced[inside].all() and np.abs(f0[inside] / want - 1.0).max() < 0.035
        else:
            assert not voiced[inside].any() and (f0[inside] == 0).all()
            if kind == "silence":
                assert (per[inside] == 0).all()           # "1 where the sum is 0"
            else:
                assert per[inside].max() < 0.5
    assert seen == {"tone", "noise", "silence", "vibrato"}


@pytest.mark.parametrize("name", sorted(ref.PARAMS))
def test_reference_margins_leave_out_at_most_five_percent(name):
    """The seeds of the GPU comparison: the reference alone decides how many frames sit on a decision boundary."""
    _, _, _, tx, ty = ref.reference_tracks(name)
    for t in (tx, ty):
        assert (t[3] < ref.MARGIN).mean() <= ref.LEFT_OUT_CAP


def test_reference_detuned_partner_and_sums():
    x, y, segments, tx, ty = ref.reference_tracks("A")
    p = ref.PARAMS["A"]
    inside = ref.frames_inside(segments[0], p["hop"], ref.frame_size(**p), len(tx[0]))
    assert np.abs(tx[0][inside] / ty[0][inside] - 1.025).max() < 2e-3          # the first segment is 2.5 % sharp
    s = ref.sums(tx[0], tx[1], ty[0], ty[1])
    m = ref.metrics_from_sums(s, len(tx[0]))
    assert s[0] <= min(s[3], s[4]) and s[5] == s[3] + s[4] - 2 * s[0] and s[7] == 0
    assert 0.3 < m["f0_rmse"] < 3.0 and 0.9 < m["vuv_f1"] <= 1.0
    same = ref.sums(ty[0], ty[1], ty[0], ty[1])
    assert same[1] == same[2] == same[5] == same[6] == same[7] == 0 and same[0] == same[3] == same[4]
    silent = ref.metrics_from_sums(ref.sums(np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4)), 4)
    assert all(math.isnan(silent[k]) for k in ("f0_rmse", "f0_cents", "gpe", "vuv_f1"))
    assert silent["vuv_error"] == 0 and silent["periodicity_rmse"] == 0


def test_lags_of_the_three_parameter_sets():
    from diffwave_sashimi_amd.metrics import check_pitch, pitch_lags
    assert pitch_lags(22050, 50.0, 550.0) == (40, 441) == ref.lags(22050, 50.0, 550.0)
    assert pitch_lags(8000, 80.0, 800.0) == (10, 100)
    assert pitch_lags(22050, 40.0, 550.0) == (40, 552)
    assert check_pitch([734]) == (40, 441) and ref.min_samples() == 734          # S = 1024 + 442


# ---- argument errors: all before a library call (CPU tensors: a call that got that far would raise RuntimeError)
def test_argument_errors_come_before_any_library_call():
    from diffwave_sashimi_amd.metrics import pitch_metrics, pitch_sums, pitch_track
    x = torch.zeros(2, 4000)
    for bad in (63, 2049, 1024.0):
        with pytest.raises(ValueError, match="win = "):
            pitch_track(x, win=bad)
    with pytest.raises(ValueError, match=r"fmin = 10.*M = 2206"):
        pitch_metrics(x, x, fmin=10.0)                                     # M > 2048
    with pytest.raises(ValueError, match=r"fmax = 12000.*tau_lo = 1"):
        pitch_metrics(x, x, fmax=12000.0)                                  # tau_lo < 2
    with pytest.raises(ValueError, match="tau_lo must lie below tau_hi"):
        pitch_track(x, fmin=500.0, fmax=400.0)
    with pytest.raises(ValueError, match="hop = 0"):
        pitch_sums(x, x, hop=0)
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="threshold = "):
            pitch_metrics(x, x, threshold=bad)
    need = ref.min_samples()
    with pytest.raises(ValueError, match=rf"clip 1 has {need - 1} samples.*at least.*{need}"):
        pitch_metrics(x, x, [4000, need - 1])                              # one sample too short: refused, not clamped
    with pytest.raises(ValueError, match=rf"clip 0 has {need - 1} samples"):
        pitch_track(x[:, :need - 1])
    with pytest.raises(ValueError, match="lengths has 3 entries for a batch of 2"):
        pitch_metrics(x, x, [4000, 4000, 4000])
    with pytest.raises(ValueError, match="lengths has 1 entries for a batch of 2"):
        pitch_track(x, [4000])
    with pytest.raises(ValueError, match="equal non-empty"):
        pitch_sums(x, x[:, :3000])


def test_cpu_tensors_are_refused():
    from diffwave_sashimi_amd.metrics import pitch_metrics, pitch_sums, pitch_track
    x = torch.zeros(1, 1, 4000)
    for call in (lambda: pitch_track(x), lambda: pitch_sums(x, x), lambda: pitch_metrics(x, x, [ref.min_samples()])):
        with pytest.raises(RuntimeError, match="GPU only|no CPU fallback"):
            call()


def test_generate_refuses_report_pitch_where_it_refuses_report_metrics(tmp_path):
    from diffwave_sashimi_amd.generate import generate
    from tests import cases
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="ljspeech", data_path=str(tmp_path), segment_length=768, sampling_rate=22050, hop_length=256)
    cond = dict(cases.WAVENET_COND_CASES["wn_cond_tiny"][0])
    with pytest.raises(ValueError, match="report_pitch does not combine with generate.mel_path"):
        generate(0, diff, cond, ds, ckpt_iter="init", mel_name="a", mel_path=str(tmp_path), report_pitch=True,
                 exp_root=str(tmp_path))
    with pytest.raises(ValueError, match="report_pitch needs a mel-conditional run"):
        generate(0, diff, dict(cases.WAVENET_CASES["wn_tiny"][0]), ds, ckpt_iter="init", report_pitch=True,
                 exp_root=str(tmp_path))
    with pytest.raises(ValueError, match="report_pitch needs a mel-conditional run"):
        generate(0, diff, cond, ds, ckpt_iter="init", report_pitch=True, exp_root=str(tmp_path))
    with pytest.raises(ValueError, match="report_pitch='yes': expected true or false"):
        generate(0, diff, cond, ds, ckpt_iter="init", mel_name="a", report_pitch="yes", exp_root=str(tmp_path))


# ---- evaluate: the flags and the NaN-aware summary
def test_evaluate_parses_the_pitch_flags():
    from diffwave_sashimi_amd import evaluate
    from diffwave_sashimi_amd.metrics import PITCH_DEFAULTS
    keys = dict(evaluate.STFT_DEFAULTS, sampling_rate=16000, hop_length=200)
    base = ["--generated", "g", "--reference", "r"]
    args = evaluate.build_parser().parse_args(base)
    assert args.pitch is False and evaluate.pitch_arguments(args, keys) is None
    args = evaluate.build_parser().parse_args(base + ["--pitch"])
    assert evaluate.pitch_arguments(args, keys) == dict(PITCH_DEFAULTS, sampling_rate=16000, hop=200)
    args = evaluate.build_parser().parse_args(base + ["--pitch", "--pitch-win", "512", "--pitch-fmin", "60", "--pitch-fmax",
                                                      "400.5", "--pitch-threshold", "0.1"])
    assert evaluate.pitch_arguments(args, keys) == dict(sampling_rate=16000, hop=200, win=512, fmin=60.0, fmax=400.5,
                                                        threshold=0.1)
    args = evaluate.build_parser().parse_args(base + ["--pitch-fmin", "60"])
    with pytest.raises(ValueError, match="--pitch-fmin needs --pitch"):
        evaluate.pitch_arguments(args, keys)


def test_evaluate_refuses_bad_pitch_parameters_before_reading_files(tmp_path):
    from diffwave_sashimi_amd import evaluate
    with pytest.raises(ValueError, match="evaluate --pitch: win = 32"):
        evaluate.main(["--generated", str(tmp_path / "none"), "--reference", str(tmp_path / "none"), "--pitch",
                       "--pitch-win", "32"])


def test_evaluate_summary_leaves_nan_clips_out():
    from diffwave_sashimi_amd.evaluate import summarise, summarise_finite
    from diffwave_sashimi_amd.metrics import nanmean
    nan = float("nan")
    rows = [{"f0_rmse": 1.0, "vuv_error": 0.1}, {"f0_rmse": nan, "vuv_error": 0.2}, {"f0_rmse": 3.0, "vuv_error": 0.3},
            {"f0_rmse": 8.0, "vuv_error": 0.6}]
    s = summarise_finite(rows, ("f0_rmse", "vuv_error"))
    assert s["f0_rmse"][0] == 4.0 and s["f0_rmse"][3] == 3
    assert abs(s["f0_rmse"][1] - math.sqrt(13.0)) < 1e-12 and abs(s["f0_rmse"][2] - 1.96 * math.sqrt(13.0 / 3.0)) < 1e-12
    assert s["vuv_error"] == summarise([{"vuv_error": r["vuv_error"]} for r in rows])["vuv_error"]
    none = summarise_finite([{"gpe": nan}, {"gpe": nan}], ("gpe",))["gpe"]
    assert math.isnan(none[0]) and none[1:] == (0.0, 0.0, 0)
    assert summarise_finite([{"gpe": nan}, {"gpe": 0.5}], ("gpe",))["gpe"] == (0.5, 0.0, 0.0, 1)
    assert nanmean([1.0, nan, 3.0]) == 2.0 and math.isnan(nanmean([nan]))


def test_evaluate_pairs_adds_the_pitch_keys(monkeypatch):
    """Both metric calls stubbed (they need a GPU): the pitch keys come after the others, NaN as it is."""
    from diffwave_sashimi_amd import evaluate
    from diffwave_sashimi_amd.metrics import PITCH_METRICS
    seen = []

    def spectral(x, y, lengths, **kw):
        return {"mr_stft": torch.tensor([float(n) for n in lengths], dtype=torch.float64)}

    def pitch(x, y, lengths, **kw):
        seen.append((list(lengths), kw))
        out = {k: torch.tensor([float(n) for n in lengths], dtype=torch.float64) for k in PITCH_METRICS}
        out["f0_rmse"] = torch.full((len(lengths),), float("nan"), dtype=torch.float64)
        return dict(out, frames=torch.ones(len(lengths)), voiced_both=torch.zeros(len(lengths)))
    monkeypatch.setattr(evaluate._metrics, "spectral_metrics", spectral)
    monkeypatch.setattr(evaluate._metrics, "pitch_metrics", pitch)
    clips = [(torch.zeros(900), torch.zeros(900)), (torch.zeros(1200), torch.zeros(1200))]
    rows = evaluate.evaluate_pairs(clips, None, batch_size=1, device="cpu", pitch=dict(win=512))
    assert [c[0] for c in seen] == [[1200], [900]] and seen[0][1] == dict(win=512)
    assert list(rows[0]) == ["mr_stft"] + list(PITCH_METRICS)
    assert rows[0]["gpe"] == 900.0 and rows[1]["vuv_f1"] == 1200.0 and math.isnan(rows[0]["f0_rmse"])
    assert list(evaluate.evaluate_pairs(clips, None, batch_size=2, device="cpu")[0]) == ["mr_stft"]


def test_the_library_exports_the_pitch_entry_points():
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd import metrics
    for name in ("dws_pitch_track", "dws_pitch_distance", "dws_pitch_distance_workspace"):
        assert name in _lib.EXPORTS
    assert metrics.PITCH_METRICS == ("f0_rmse", "f0_cents", "gpe", "vuv_error", "vuv_f1", "periodicity_rmse")
    assert metrics.METRICS == ("mr_stft", "ls_mae", "lsd", "mcd")

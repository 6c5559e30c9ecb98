"""CPU: the filter design and the band matrix against independent formulae, the float64 restatement of STOI / ESTOI on
signals with known answers, ``audio.resample`` / ``metrics.stoi`` check their arguments before any library call, and
``evaluate`` parses ``--stoi`` and ``--resample``."""
import math

import numpy as np
import pytest
import torch

from tests import stoi_reference as ref


@pytest.mark.parametrize("sr_in,sr_out,U,D", [(22050, 10000, 200, 441), (16000, 10000, 5, 8), (10000, 16000, 8, 5),
                                              (16000, 22050, 441, 320), (2, 1, 1, 2), (1, 1, 1, 1)])
def test_resample_filter_against_the_formula(sr_in, sr_out, U, D):
    from diffwave_sashimi_amd.audio import resample_filter
    u, d, h = resample_filter(sr_in, sr_out)
    assert (u, d) == (U, D) and h.dtype == np.float64
    assert len(h) == 2 * 10 * max(U, D) + 1
    assert abs(h.sum() - U) < 1e-12 * U
    assert np.array_equal(h, h[::-1])
    want = ref.kaiser_sinc(U, D)
    assert np.abs(h - want).max() < 1e-13 * np.abs(want).max()
    _, _, h6 = resample_filter(sr_in, sr_out, zeros=6, beta=8.0)
    assert len(h6) == 2 * 6 * max(U, D) + 1
    assert np.abs(h6 - ref.kaiser_sinc(U, D, 6, 8.0)).max() < 1e-13 * np.abs(h6).max()


def test_third_octave_bands_are_taals():
    from diffwave_sashimi_amd.metrics import STOI_DEFAULTS, STOI_METRICS, third_octave_bands
    assert STOI_METRICS == ("stoi", "estoi")
    assert STOI_DEFAULTS == dict(fs=10000, frame=256, hop=128, n_fft=512, n_bands=15, f_min=150.0, segment=30, beta=-15.0,
                                 dyn_range=40.0)
    obm, centres = third_octave_bands()
    assert obm.shape == (15, 257) and obm.dtype == np.float64 and set(np.unique(obm)) == {0.0, 1.0}
    assert np.allclose(centres, 150.0 * 2.0 ** (np.arange(15) / 3.0), rtol=1e-15)
    edges = [(int(np.flatnonzero(row)[0]), int(np.flatnonzero(row)[-1]) + 1) for row in obm]
    # the edges 150 2^((2k -+ 1) / 6) Hz in bins of 10000 / 512 Hz are 6.84, 8.62, 10.86, 13.68, 17.24, 21.72, 27.37,
    # 34.48, 43.45, 54.74, 68.96, 86.89, 109.47, 137.93, 173.78, 218.95: each to the nearest bin
    assert edges == [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69),
                     (69, 87), (87, 109), (109, 138), (138, 174), (174, 219)]
    for row, (lo, hi) in zip(obm, edges):                   # contiguous, non-empty, inside bins 7 .. 219
        assert hi > lo and row[lo:hi].all() and row.sum() == hi - lo
    assert np.array_equal(obm, ref.bands())


def test_restatement_known_answers():
    sr, y, xs = ref.signal_set("C")
    vals = ref.reference_values("C")
    s, e, K, M, margins = vals[-1]                          # y against itself
    assert abs(s - 1.0) < 1e-12 and abs(e - 1.0) < 1e-12
    assert K < len(margins) and M == K - 29                 # frames really are removed
    snr = [v[0] for v in vals[:4]]
    assert all(a > b for a, b in zip(snr, snr[1:])) and snr[0] > 0.95 and snr[-1] < 0.6
    esnr = [v[1] for v in vals[:4]]
    assert all(a > b for a, b in zip(esnr, esnr[1:]))
    zero = ref.stoi(np.zeros_like(y), y)
    assert zero[0] == 0.0 and zero[1] == 0.0 and zero[2] == K
    x, yn = ref.stationary_noise(3968)
    assert ref.stoi(x, yn)[2:4] == (30, 1)
    x, yn = ref.stationary_noise(3967)
    short = ref.stoi(x, yn)
    assert math.isnan(short[0]) and math.isnan(short[1]) and short[2:4] == (29, 0)


def test_silent_frames_go_at_both_ends_and_inside():
    for name in ref.SETS:
        sr, y, _ = ref.signal_set(name)
        from diffwave_sashimi_amd.audio import resample_filter
        y10 = y if sr == ref.FS else ref.resample(y, *resample_filter(sr, ref.FS))
        w = np.hanning(ref.FRAME + 2)[1:-1]
        e = np.array([20 * np.log10(np.linalg.norm(w * y10[i:i + ref.FRAME]) + ref.EPS)
                      for i in range(0, len(y10) - ref.FRAME + 1, ref.HOP)])
        keep = e > e.max() - ref.DYN_RANGE
        inner = np.flatnonzero(keep)
        assert not keep[0] and not keep[-1] and not keep[inner[0]:inner[-1] + 1].all(), name


def test_resample_checks_arguments_before_the_device():
    from diffwave_sashimi_amd.audio import resample
    x = torch.zeros(2, 100)
    for args, match in (((x, 22050.5, 10000), "positive integers"), ((x, 0, 10000), "positive integers"),
                        ((x, True, 10000), "positive integers"), ((x, 22050, -1), "positive integers"),
                        ((x, 22050, 22051), r"22050 -> 22051 is the ratio 22051 / 22050, whose filter has 441021 taps"),
                        ((x, 48000, 1000), r"48000 -> 1000 is the ratio 1 / 48: a tile of 1024 outputs reads 50066 input"),
                        ((torch.zeros(100), 2, 1), "expected a non-empty float tensor"),
                        ((torch.zeros(2, 2, 100), 2, 1), "expected a non-empty float tensor"),
                        ((torch.zeros(2, 100, dtype=torch.int32), 2, 1), "expected a non-empty float tensor"),
                        ((x, 2, 1, [100]), "lengths"), ((x, 2, 1, [100, 101]), "lengths"), ((x, 2, 1, [0, 5]), "lengths")):
        with pytest.raises(ValueError, match=match):
            resample(*args)
    with pytest.raises(ValueError, match="zeros"):
        resample(x, 2, 1, zeros=0)
    with pytest.raises(ValueError, match="requires grad"):
        resample(torch.zeros(2, 100, requires_grad=True), 2, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resample(x, 2, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resample(x[:, None], 16000, 10000, [100, 7])


def test_stoi_checks_arguments_before_the_device():
    from diffwave_sashimi_amd.metrics import stoi, stoi_sums
    x = torch.zeros(2, 4000)
    with pytest.raises(ValueError, match="two equal non-empty batches"):
        stoi(x, torch.zeros(2, 3999))
    with pytest.raises(ValueError, match="positive integers"):
        stoi(x, x, sampling_rate=22050.0)
    with pytest.raises(ValueError, match="ratio 10000 / 10001"):
        stoi(x, x, sampling_rate=10001)
    # 563 samples at 22050 Hz are ceil(563 * 200 / 441) = 256 at 10 kHz, 562 are 255
    with pytest.raises(ValueError, match=r"stoi: clip 1 has 562 samples at 22050 Hz, 255 at 10000 Hz: one frame is 256"):
        stoi(x, x, [4000, 562])
    with pytest.raises(ValueError, match="clip 0 has 255 samples"):
        stoi_sums(x[:, :255], x[:, :255])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stoi(x, x, [4000, 563])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stoi_sums(x, x)


def test_generate_refuses_report_stoi_where_it_refuses_report_metrics(tmp_path):
    from diffwave_sashimi_amd.generate import generate
    from tests import cases
    diff = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="ljspeech", data_path=str(tmp_path), segment_length=768, sampling_rate=22050, hop_length=256)
    cond = dict(cases.WAVENET_COND_CASES["wn_cond_tiny"][0])
    with pytest.raises(ValueError, match="report_stoi does not combine with generate.mel_path"):
        generate(0, diff, cond, ds, ckpt_iter="init", mel_name="a", mel_path=str(tmp_path), report_stoi=True,
                 exp_root=str(tmp_path))
    with pytest.raises(ValueError, match="report_stoi needs a mel-conditional run"):
        generate(0, diff, dict(cases.WAVENET_CASES["wn_tiny"][0]), ds, ckpt_iter="init", report_stoi=True,
                 exp_root=str(tmp_path))
    with pytest.raises(ValueError, match="report_stoi='yes': expected true or false"):
        generate(0, diff, cond, ds, ckpt_iter="init", mel_name="a", report_stoi="yes", exp_root=str(tmp_path))


def test_evaluate_parses_the_flags():
    from diffwave_sashimi_amd.evaluate import build_parser
    base = ["--generated", "g", "--reference", "r"]
    args = build_parser().parse_args(base)
    assert args.stoi is False and args.resample is False
    args = build_parser().parse_args(base + ["--stoi", "--resample", "--pitch"])
    assert args.stoi is True and args.resample is True and args.pitch is True

"""GPU: ``metrics.stoi`` (``dws_resample`` + ``dws_stoi``) against the float64 restatement (tests/stoi_reference.py) on
speech-like signals at 22050 Hz (A, 1.2 s), 16000 Hz (B, 1.0 s) and 10000 Hz (C, 0.9 s, no conversion), each with noise at
30 / 10 / 0 / -10 dB SNR and a hard-clipped copy, and on stationary noise at 10 kHz (D) of 3968 samples (30 frames, one
segment) and 3967 (29 frames: NaN).

A condition on the inputs, not a tolerance: no frame of any reference lies within 0.01 dB of the silence threshold (the
restatement's margins; the smallest here is 2.08 dB), so ``frames_kept`` and ``segments`` must equal the restatement's.

Tolerance of ``stoi`` / ``estoi``.  Measured on an MI355X on exactly these inputs, the largest absolute difference from
float64 per set (stoi, estoi): A 1.69e-7, 1.24e-7; B 4.7e-8, 6.1e-8; C 1.4e-8, 1.30e-7; D 5e-10, 8e-9 (y against itself: 0
and 1.1e-16).  The largest, 1.69e-7, times 8 and rounded up to one digit: 2e-6.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import stoi_reference as ref

pytestmark = pytest.mark.gpu

TOL = 2e-6
NAMES = sorted(ref.SETS)


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _stoi(x, y, gpu, sr, lengths=None):
    from diffwave_sashimi_amd.metrics import stoi
    return stoi(_dev(x, gpu), _dev(y, gpu), lengths, sampling_rate=sr)


@pytest.mark.parametrize("name", NAMES)
def test_against_float64(name, gpu):
    sr, y, xs = ref.signal_set(name)
    want = ref.reference_values(name)
    for v in want:
        assert v[4].min() > ref.MARGIN_DB, (name, v[4].min())        # the share of frames near the threshold is zero
    got = _stoi(np.stack(xs + [y]), np.stack([y] * (len(xs) + 1)), gpu, sr)
    assert all(got[k].dtype == torch.float64 and got[k].device.type == "cpu" and tuple(got[k].shape) == (6,) for k in got)
    assert sorted(got) == ["estoi", "frames_kept", "segments", "stoi"]
    worst = [0.0, 0.0]
    for b, (s, e, K, M, _) in enumerate(want):
        assert int(got["frames_kept"][b]) == K and int(got["segments"][b]) == M and M > 0, (name, b)
        ds, de = abs(float(got["stoi"][b]) - s), abs(float(got["estoi"][b]) - e)
        print(f"stoi set {name} case {b}: kept {K} frames, {M} segments, stoi {s:.6f} (diff {ds:.3e}), estoi {e:.6f} "
              f"(diff {de:.3e})")
        worst = [max(worst[0], ds), max(worst[1], de)]
    print(f"stoi set {name}: largest differences {worst[0]:.3e} (stoi) {worst[1]:.3e} (estoi)")
    assert worst[0] <= TOL and worst[1] <= TOL, (name, worst)
    s = got["stoi"][:4].tolist()
    assert all(a > b for a, b in zip(s, s[1:])), s                   # strictly decreasing over the SNRs
    e = got["estoi"][:4].tolist()
    assert all(a > b for a, b in zip(e, e[1:])), e
    assert abs(float(got["stoi"][5]) - 1.0) <= TOL and abs(float(got["estoi"][5]) - 1.0) <= TOL      # y against itself


def test_one_segment_and_none(gpu):
    """Set D: 3968 samples are 30 frames, all kept, exactly one segment; 3967 are 29 and the metric is undefined."""
    x, y = ref.stationary_noise(3968)
    s, e, K, M, margins = ref.stoi(x, y)
    assert (K, M) == (30, 1) and margins.min() > ref.MARGIN_DB
    got = _stoi(x[None], y[None], gpu, 10000)
    assert (int(got["frames_kept"][0]), int(got["segments"][0])) == (30, 1)
    ds, de = abs(float(got["stoi"][0]) - s), abs(float(got["estoi"][0]) - e)
    print(f"stoi set D: stoi {s:.6f} (diff {ds:.3e}), estoi {e:.6f} (diff {de:.3e})")
    assert ds <= TOL and de <= TOL
    x, y = ref.stationary_noise(3967)
    got = _stoi(x[None], y[None], gpu, 10000)
    assert (int(got["frames_kept"][0]), int(got["segments"][0])) == (29, 0)
    assert math.isnan(float(got["stoi"][0])) and math.isnan(float(got["estoi"][0]))
    # in a batch with a clip that has segments, and as sums: zero, not garbage
    from diffwave_sashimi_amd.metrics import stoi_sums
    x2, y2 = ref.stationary_noise(3968)
    sums = stoi_sums(_dev(np.stack([x2, x2]), gpu), _dev(np.stack([y2, y2]), gpu), [3968, 3967])
    assert sums[1].tolist() == [0.0, 0.0, 0.0, 29.0] and sums[0, 2:].tolist() == [1.0, 30.0]


def test_a_silent_generated_signal_scores_exactly_zero(gpu):
    for name in ("A", "C"):
        sr, y, _ = ref.signal_set(name)
        got = _stoi(np.zeros_like(y)[None], y[None], gpu, sr)
        assert float(got["stoi"][0]) == 0.0 and float(got["estoi"][0]) == 0.0 and int(got["segments"][0]) > 0


def test_ragged_batch_rows_are_the_clips_alone(gpu):
    sr, y, xs = ref.signal_set("A")
    n = len(y)
    lengths = [n, n - 3001, n - 7000]
    x = _dev(np.stack([xs[1], xs[2], xs[4]]), gpu)
    yy = _dev(np.stack([y, y, y]), gpu)
    for b, m in enumerate(lengths):
        x[b, m:] = float("nan")                             # nothing behind len_b is read
        yy[b, m:] = float("nan")
    from diffwave_sashimi_amd.metrics import stoi
    got = stoi(x, yy, lengths, sampling_rate=sr)
    again = stoi(x, yy, lengths, sampling_rate=sr)
    for k in got:
        assert torch.equal(got[k].view(torch.int64), again[k].view(torch.int64)), k       # two calls, the same bits
    assert got["segments"].min() > 0 and len(set(got["frames_kept"].tolist())) == 3
    for b, m in enumerate(lengths):
        alone = stoi(x[b:b + 1, :m].contiguous(), yy[b:b + 1, :m].contiguous(), sampling_rate=sr)
        for k in got:
            assert got[k][b].view(torch.int64) == alone[k][0].view(torch.int64), (b, k, float(got[k][b]), float(alone[k][0]))


def test_invalid_arguments_through_the_c_entry(gpu):
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.metrics import _stoi_constants
    lib = _lib.load()
    B, T = 2, 4000
    x = torch.zeros(B, T, device=gpu)
    window, obm = _stoi_constants(gpu)
    ws = torch.zeros(lib.dws_stoi_workspace(B, T, 256, 128, 15) // 8, dtype=torch.float64, device=gpu)
    assert ws.numel() > 0 and lib.dws_stoi_workspace(0, T, 256, 128, 15) == 0 and lib.dws_stoi_workspace(B, 255, 256, 128, 15) == 0
    out = torch.zeros(B, 4, dtype=torch.float64, device=gpu)
    dev_len = torch.tensor([4000, 256], dtype=torch.int32, device=gpu)
    host_len = (ctypes.c_int32 * 2)(4000, 256)

    def call(xp=None, yp=None, B=B, T=T, dl=None, hl=None, wp=None, frame=256, hop=128, n_fft=512, op=None, n_bands=15,
             segment=30, wsp=None, outp=None):
        return lib.dws_stoi(x.data_ptr() if xp is None else xp, x.data_ptr() if yp is None else yp, B, T, dl, hl,
                            window.data_ptr() if wp is None else wp, frame, hop, n_fft, obm.data_ptr() if op is None else op,
                            n_bands, segment, -15.0, 40.0, ws.data_ptr() if wsp is None else wsp,
                            out.data_ptr() if outp is None else outp, 0)

    assert call() == _lib.DWS_OK and call(dl=dev_len.data_ptr(), hl=host_len) == _lib.DWS_OK
    torch.cuda.synchronize()
    for kw, text in ((dict(xp=0), "null"), (dict(yp=0), "null"), (dict(wp=0), "null"), (dict(op=0), "null"),
                     (dict(wsp=0), "null workspace"), (dict(outp=0), "null"), (dict(n_fft=500), "n_fft = 500"),
                     (dict(n_fft=32), "n_fft = 32"), (dict(n_fft=4096), "n_fft = 4096"),
                     (dict(frame=513), "frame = 513"), (dict(hop=0), "hop = 0"), (dict(segment=1), "segment = 1"),
                     (dict(n_bands=0), "n_bands = 0"), (dict(n_bands=65), "n_bands = 65"), (dict(B=0), "B = 0"),
                     (dict(B=65536), "B = 65536"), (dict(T=255), "T = 255"), (dict(dl=dev_len.data_ptr()), "come together"),
                     (dict(dl=dev_len.data_ptr(), hl=(ctypes.c_int32 * 2)(4000, 255)), "clip 1 has 255 samples"),
                     (dict(dl=dev_len.data_ptr(), hl=(ctypes.c_int32 * 2)(4001, 256)), "clip 0 has 4001 samples")):
        assert call(**kw) == _lib.DWS_ERR_INVALID, kw
        assert text in lib.dws_last_error().decode(), (kw, lib.dws_last_error().decode())

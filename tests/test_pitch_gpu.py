"""GPU: ``dws_pitch_track`` / ``dws_pitch_distance`` against the float64 restatement (tests/pitch_reference.py) at three
parameter sets chosen for where the kernel can go wrong -- (A) the defaults: 111 lag groups, the window in two parts;
(B) W = 200 and M = 101: nine parts of 50 blocks, the last ones empty, M + 1 no multiple of 4; (C) W = 2048, M = 553:
more lag groups than half a workgroup, one part, three lags per thread in the prefix sum.

Bounds of the frame-wise comparison.  Measured on an MI355X on exactly these inputs (frames whose decision margin is
below 1e-5 left out; none is, with these seeds): f0 within 2.07e-7 relative (largest per set A / B / C: 8.9e-8, 5.7e-8,
2.07e-7 -- the rounding of the output to float32, 2^-24 = 6.0e-8, is part of it), periodicity within 1.27e-6 absolute
(4.5e-7, 1.2e-7, 1.27e-6).  Times 8, rounded up to one digit: 2e-6 and 2e-5.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import pitch_reference as ref

pytestmark = pytest.mark.gpu

F0_RTOL = 2e-6
P_ATOL = 2e-5
SETS = sorted(ref.PARAMS)


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _track(s, gpu, lengths=None, **p):
    from diffwave_sashimi_amd.metrics import pitch_track
    s = _dev(s, gpu) if isinstance(s, np.ndarray) else s
    f0, per = pitch_track(s[None] if s.dim() == 1 else s, lengths, **p)
    return f0.cpu().numpy(), per.cpu().numpy()


@pytest.mark.parametrize("name", SETS)
def test_tracks_against_float64(name, gpu):
    x, y, _, tx, ty = ref.reference_tracks(name)
    worst = [0.0, 0.0]
    for which, s, (f0, per, voiced, margin) in (("x", x, tx), ("y", y, ty)):
        got_f0, got_per = (v[0] for v in _track(s, gpu, **ref.PARAMS[name]))
        assert got_f0.dtype == np.float32 and got_f0.shape == f0.shape == got_per.shape
        keep = margin >= ref.MARGIN
        assert (~keep).mean() <= ref.LEFT_OUT_CAP, (name, which, int((~keep).sum()), len(keep))
        assert np.array_equal(got_f0[keep] > 0, voiced[keep]), (name, which)
        v = keep & voiced
        err_f0 = float(np.abs(got_f0[v].astype(np.float64) / f0[v] - 1.0).max())
        err_p = float(np.abs(got_per[keep].astype(np.float64) - per[keep]).max())
        print(f"pitch set {name} {which}: frames {len(keep)}, left out {int((~keep).sum())}, voiced {int(v.sum())}, "
              f"max rel f0 error {err_f0:.3e}, max abs periodicity error {err_p:.3e}")
        assert (got_f0[keep & ~voiced] == 0).all()
        worst = [max(worst[0], err_f0), max(worst[1], err_p)]
    assert worst[0] <= F0_RTOL and worst[1] <= P_ATOL, (name, worst)


@pytest.mark.parametrize("name", SETS)
def test_sums_restated_from_the_kernels_own_tracks(name, gpu):
    """The rolled pair sets tones against noise, silence and other tones: gross errors and voicing errors both occur."""
    from diffwave_sashimi_amd.metrics import pitch_metrics, pitch_sums
    p = ref.PARAMS[name]
    x, y, _ = ref.signal_pair(name)
    n = len(y)
    rolled = np.roll(y, n // 3)
    xs, ys = _dev(np.stack([x, rolled]), gpu), _dev(np.stack([y, y]), gpu)
    short = n - n // 5 - 7
    for lengths in (None, [n, short]):
        f0x, px = _track(xs, gpu, lengths, **p)
        f0y, py = _track(ys, gpu, lengths, **p)
        got = pitch_sums(xs, ys, lengths, **p)
        assert got.dtype == torch.float64 and tuple(got.shape) == (2, 8) and got.device.type == "cpu"
        m = pitch_metrics(xs, ys, lengths, **p)
        for b in range(2):
            frames = (n if lengths is None else lengths[b]) // p["hop"] + 1
            want = ref.sums(f0x[b], px[b], f0y[b], py[b], frames)
            g = got[b].numpy()
            for q in (0, 3, 4, 5, 7):
                assert g[q] == want[q], (name, lengths, b, q, g, want)
            for q in (1, 2, 6):
                assert abs(g[q] - want[q]) <= 1e-12 * abs(want[q]), (name, lengths, b, q, g[q], want[q])
            wm = ref.metrics_from_sums(g, frames)
            for k, v in wm.items():
                assert float(m[k][b]) == v or (np.isnan(v) and np.isnan(float(m[k][b]))), (k, b)
            assert float(m["frames"][b]) == frames and float(m["voiced_both"][b]) == g[0]
        assert got[1, 7] > 0 and got[1, 5] > 0 and got[0, 1] > 0      # the cases do what they were built for


@pytest.mark.parametrize("name", SETS)
def test_known_answers(name, gpu):
    from diffwave_sashimi_amd.metrics import PITCH_METRICS, pitch_metrics
    p = ref.PARAMS[name]
    _, y, _ = ref.signal_pair(name)
    yd = _dev(y, gpu)[None]
    m = pitch_metrics(yd, yd, **p)
    for k in PITCH_METRICS:
        assert float(m[k][0]) == (1.0 if k == "vuv_f1" else 0.0), k
    full, half = _track(yd, gpu, **p), _track(0.5 * yd, gpu, **p)
    assert np.array_equal(full[0], half[0]) and np.array_equal(full[1], half[1])      # a power of two passes exactly
    assert (full[0] > 0).any() and (full[0] == 0).any()
    again = _track(yd, gpu, **p)
    assert np.array_equal(full[0], again[0]) and np.array_equal(full[1], again[1])    # two calls, the same bits
    silent = _track(torch.zeros(1, len(y), device=gpu), gpu, **p)
    assert (silent[0] == 0).all() and (silent[1] == 0).all()
    m = pitch_metrics(torch.zeros(1, len(y), device=gpu), yd, **p)
    assert all(np.isnan(float(m[k][0])) for k in ("f0_rmse", "f0_cents", "gpe")) and float(m["vuv_f1"][0]) == 0.0


@pytest.mark.parametrize("name", SETS)
def test_ragged_batch_rows_are_the_clips_alone(name, gpu):
    """Full length (a multiple of hop: the last frame starts at len_b), a length that is no multiple of hop, and the
    shortest admitted; NaN behind every length."""
    from diffwave_sashimi_amd.metrics import pitch_sums
    p = ref.PARAMS[name]
    x, y, _ = ref.signal_pair(name)
    n, hop = len(y), p["hop"]
    lens = [n, (3 * n) // 5 + 13, ref.min_samples(**p)]
    assert n % hop == 0 and lens[1] % hop != 0
    xs = torch.full((3, n), float("nan"))
    ys = torch.full((3, n), float("nan"))
    for b, ln in enumerate(lens):
        xs[b, :ln], ys[b, :ln] = torch.from_numpy(x[:ln]), torch.from_numpy(y[:ln])
    xs, ys = xs.to(gpu), ys.to(gpu)
    f0, per = _track(ys, gpu, lens, **p)
    sums = pitch_sums(xs, ys, lens, **p)
    assert f0.shape == (3, n // hop + 1)
    for b, ln in enumerate(lens):
        frames = ln // hop + 1
        a_f0, a_per = _track(ys[b, :ln].clone(), gpu, **p)
        assert a_f0.shape == (1, frames)
        assert np.array_equal(f0[b, :frames], a_f0[0]) and np.array_equal(per[b, :frames], a_per[0]), (name, b)
        assert (f0[b, frames:] == 0).all() and (per[b, frames:] == 0).all()
        assert not np.isnan(f0[b]).any() and not np.isnan(per[b]).any()
        alone = pitch_sums(xs[b:b + 1, :ln].clone(), ys[b:b + 1, :ln].clone(), **p)
        assert torch.equal(sums[b], alone[0]), (name, b, sums[b], alone[0])
    assert (f0[0] > 0).any()


def test_a_clip_one_sample_too_short_is_refused(gpu):
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.metrics import pitch_metrics, pitch_track
    need = ref.min_samples()
    y = torch.zeros(2, 4000, device=gpu)
    with pytest.raises(ValueError, match=rf"clip 1 has {need - 1} samples"):
        pitch_metrics(y, y, [4000, need - 1])
    with pytest.raises(ValueError, match=rf"clip 0 has {need - 1} samples"):
        pitch_track(y[:, :need - 1])
    lib = _lib.load()
    track = torch.full((2, 4000 // 256 + 1, 2), 7.0, device=gpu)
    args = (256, 1024, 40, 441, 0.15, 22050.0, track.data_ptr(), _lib.current_stream())
    host = (ctypes.c_int32 * 2)(4000, need - 1)
    dev = torch.tensor([4000, need - 1], dtype=torch.int32, device=gpu)
    assert lib.dws_pitch_track(y.data_ptr(), 2, 4000, dev.data_ptr(), host, *args) == _lib.DWS_ERR_INVALID
    assert b"clip 1" in lib.dws_last_error()
    assert lib.dws_pitch_track(y.data_ptr(), 2, need - 1, None, None, *args) == _lib.DWS_ERR_INVALID
    for bad in ((256, 2049, 40, 441, 0.15), (256, 1024, 1, 441, 0.15), (256, 1024, 40, 2048, 0.15), (0, 1024, 40, 441, 0.15),
                (256, 1024, 40, 441, 1.0), (256, 1024, 441, 441, 0.15)):
        assert lib.dws_pitch_track(y.data_ptr(), 2, 4000, None, None, *bad, *args[5:]) == _lib.DWS_ERR_INVALID, bad
    torch.cuda.synchronize()
    assert bool((track == 7.0).all())                                          # nothing ran
    assert lib.dws_pitch_distance_workspace(2, 4000, 256) == 2 * 2 * 16 * 2 * 4
    assert lib.dws_pitch_distance_workspace(2, 4000, 0) == 0


def test_a_device_length_the_host_did_not_admit_makes_an_empty_clip(gpu):
    """The host copy is what is checked; whatever the device copy holds, no index leaves the row."""
    from diffwave_sashimi_amd import _lib
    _, y, _ = ref.signal_pair("B")
    p = ref.PARAMS["B"]
    n = len(y)
    ys = _dev(np.stack([y, y, y]), gpu)
    lib = _lib.load()
    frames = n // p["hop"] + 1
    track = torch.full((3, frames, 2), 7.0, device=gpu)
    host = (ctypes.c_int32 * 3)(n, n, n)
    dev = torch.tensor([n + 1000, 5, n], dtype=torch.int32, device=gpu)
    _lib.check(lib.dws_pitch_track(ys.data_ptr(), 3, n, dev.data_ptr(), host, p["hop"], p["win"], 10, 100, p["threshold"],
                                   float(p["sampling_rate"]), track.data_ptr(), _lib.current_stream()))
    want = _track(y, gpu, **p)
    assert bool((track[:2] == 0).all())
    assert np.array_equal(track[2, :, 0].cpu().numpy(), want[0][0])

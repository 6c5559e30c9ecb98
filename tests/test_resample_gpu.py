"""GPU: ``dws_resample`` against ``scipy.signal.resample_poly`` in float64 (tests/stoi_reference.py) at the ratios and
lengths at which the kernel can go wrong: the 441-based ratios (8821 taps, down and up), 5/8 and 8/5, a single phase
(2 -> 1), the copy; one and seven samples (every output sees the table cut at both edges) and output lengths on both
sides of the tile.

The bound is derived, not measured, per output sample: ``|y - y_ref| <= (n + 2) 2^-24 sum_i |x_i| |h_k|`` with ``n`` the
products of that sample -- gamma_n of the fp32 fmaf chain plus the rounding of the taps to float32 (the oracle runs on the
float64 table).  The test prints the largest ratio of error to bound.

Output lengths: a clip of ``n`` samples gives ``ceil(n U / D)``, so when upsampling not every length exists; a wanted
length that does not is replaced by the next one above it that does (8/5: 1025 -> 1026)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import stoi_reference as ref

pytestmark = pytest.mark.gpu

RATIOS = [(22050, 10000), (16000, 10000), (10000, 16000), (16000, 22050), (2, 1)]


def _tile():
    from diffwave_sashimi_amd import _lib
    return _lib.load().dws_resample_tile()


def _input_length(out_len, U, D):
    """The shortest clip with at least ``out_len`` output samples."""
    n = max(1, (out_len * D) // U - 2)
    while -((-n * U) // D) < out_len:
        n += 1
    return n


def _lengths(U, D):
    tile = _tile()
    return [1, 7] + [_input_length(m, U, D) for m in (tile - 1, tile, tile + 1, 2 * tile + 3)]


def _signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (0.4 * rng.standard_normal(n) + 0.5 * np.sin(0.05 * t + seed)).astype(np.float32)


def test_tile_is_what_python_assumes():
    from diffwave_sashimi_amd import audio
    assert _tile() == audio.TILE == 1024


@pytest.mark.parametrize("sr_in,sr_out", RATIOS)
def test_against_float64(sr_in, sr_out, gpu):
    from diffwave_sashimi_amd.audio import resample, resample_filter
    U, D, h = resample_filter(sr_in, sr_out)
    h32 = h.astype(np.float32)
    tile = _tile()
    outs, worst = [], 0.0
    for n in _lengths(U, D):
        x = _signal(n, n)
        y, lens = resample(torch.from_numpy(x).to(gpu)[None], sr_in, sr_out)
        want = ref.resample(x, U, D, h)
        assert y.dtype == torch.float32 and tuple(y.shape) == (1, len(want)) and lens == [len(want)] == [-((-n * U) // D)]
        outs.append(len(want))
        err = np.abs(y[0].cpu().numpy().astype(np.float64) - want)
        bound = ref.resample_bound(x, U, D, h32)
        assert (bound > 0).all()
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print(f"resample {sr_in} -> {sr_out} ({U}/{D}), {n} -> {len(want)} samples: max |err| {err.max():.3e}, "
              f"max err / bound {ratio:.3f}")
        assert ratio <= 1.0, (sr_in, sr_out, n, ratio)
    assert outs[0] == -((-U) // D) and outs[2:4] == [tile - 1, tile]           # shapes on both sides of the tile
    assert outs[4] in (tile + 1, tile + 2) and outs[5] in (2 * tile + 3, 2 * tile + 4)
    print(f"resample {sr_in} -> {sr_out}: largest err / bound {worst:.3f}")


def test_equal_rates_copy_bit_for_bit(gpu):
    from diffwave_sashimi_amd.audio import resample
    tile = _tile()
    for n in (1, 7, tile - 1, tile, tile + 1, 2 * tile + 3):
        x = torch.from_numpy(_signal(n, 3)).to(gpu)[None]
        x[0, n // 2] = float("inf")                         # a copy carries every bit pattern
        y, lens = resample(x, 16000, 16000)
        assert lens == [n] and torch.equal(y.view(torch.int32), x.view(torch.int32))
    x = torch.from_numpy(_signal(300, 4)).to(gpu)[None].repeat(2, 1)
    x[1, 100:] = float("nan")
    y, lens = resample(x[:, None], 5, 5, [300, 100])
    assert lens == [300, 100] and tuple(y.shape) == (2, 1, 300)
    assert torch.equal(y[0, 0], x[0]) and torch.equal(y[1, 0, :100], x[1, :100]) and (y[1, 0, 100:] == 0).all()


@pytest.mark.parametrize("sr_in,sr_out", RATIOS)
def test_ragged_batch_rows_are_the_clips_alone(sr_in, sr_out, gpu):
    from diffwave_sashimi_amd.audio import output_length, resample, resample_filter
    U, D, _ = resample_filter(sr_in, sr_out)
    T = _input_length(2 * _tile() + 3, U, D)
    lengths = [T, T - 37, 1]
    x = torch.from_numpy(np.stack([_signal(T, s) for s in (1, 2, 3)])).to(gpu)
    for b, n in enumerate(lengths):
        x[b, n:] = float("nan")                             # nothing behind len_b is read
    y, lens = resample(x, sr_in, sr_out, lengths)
    assert lens == [output_length(n, U, D) for n in lengths] and tuple(y.shape) == (3, lens[0])
    again, _ = resample(x, sr_in, sr_out, lengths)
    assert torch.equal(y.view(torch.int32), again.view(torch.int32))
    assert not torch.isnan(y).any()
    for b, n in enumerate(lengths):
        alone, one = resample(x[b:b + 1, :n].contiguous(), sr_in, sr_out)
        assert one == [lens[b]]
        assert torch.equal(y[b, :lens[b]].view(torch.int32), alone[0].view(torch.int32)), (b, n)
        assert (y[b, lens[b]:].view(torch.int32) == 0).all()       # the padding is exactly +0


def test_refusals(gpu):
    from diffwave_sashimi_amd import _lib
    lib = _lib.load()
    x = torch.zeros(2, 64, device=gpu)
    h = torch.zeros(161, device=gpu)
    y = torch.zeros(2, 64, device=gpu)
    dev_len = torch.tensor([64, 10], dtype=torch.int32, device=gpu)
    host_len = (ctypes.c_int32 * 2)(64, 10)

    def call(xp=None, B=2, T=64, dl=None, hl=None, hp=None, taps=161, U=5, D=8, yp=None, T_out=40):
        return lib.dws_resample(x.data_ptr() if xp is None else xp, B, T, dl, hl, h.data_ptr() if hp is None else hp, taps, U,
                                D, y.data_ptr() if yp is None else yp, T_out, 0)

    def message():
        return lib.dws_last_error().decode()

    assert call() == _lib.DWS_OK and call(dl=dev_len.data_ptr(), hl=host_len) == _lib.DWS_OK
    torch.cuda.synchronize()
    for kw, text in ((dict(xp=0), "null"), (dict(hp=0), "null"), (dict(yp=0), "null"),
                     (dict(taps=160), "160 taps at ratio 5 / 8"), (dict(U=0), "ratio U / D = 0 / 8"),
                     (dict(D=0), "ratio U / D = 5 / 0"), (dict(B=0), "B = 0"), (dict(B=65536), "B = 65536"),
                     (dict(T_out=39), "T_out = 39 at ratio 5 / 8"), (dict(dl=dev_len.data_ptr()), "come together"),
                     (dict(hl=host_len), "come together"),
                     (dict(dl=dev_len.data_ptr(), hl=(ctypes.c_int32 * 2)(64, 0)), "clip 1 has 0 samples"),
                     (dict(dl=dev_len.data_ptr(), hl=(ctypes.c_int32 * 2)(65, 10)), "clip 0 has 65 samples")):
        assert call(**kw) == _lib.DWS_ERR_INVALID, kw
        assert text in message(), (kw, message())
    # 22050 -> 22051: 2 * 10 * 22051 + 1 taps; 48000 -> 1000 with its 961 taps: a tile reads 50066 samples
    assert call(taps=441021, U=22051, D=22050, T_out=80) == _lib.DWS_ERR_UNSUPPORTED
    assert "ratio 22051 / 22050 comes with 441021 taps" in message()
    assert call(taps=961, U=1, D=48, T_out=2) == _lib.DWS_ERR_UNSUPPORTED
    assert "ratio 1 / 48" in message() and "50066 input samples" in message()
    with pytest.raises(ValueError, match="22050 -> 22051 is the ratio 22051 / 22050"):
        from diffwave_sashimi_amd.audio import resample
        resample(x, 22050, 22051)

"""Sample-rate conversion on the HIP engine (not in the reference, which leaned on torchaudio / librosa for it).

``resample(x, sr_in, sr_out)`` converts a batch of waveforms by the rational factor ``U / D = sr_out / sr_in`` with a
Kaiser-windowed sinc filter, the filter family of ``scipy.signal.resample_poly``: the polyphase sum runs in
``dws_resample`` (``csrc/resample_kernels.hip``; DESIGN.md section 4, "Intelligibility metrics"), this module designs the
table, checks the arguments and caches the table per device.  There is no CPU path and no adjoint.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

MAX_TAPS = 16384        # dws_resample's table in LDS
MAX_SPAN = 16384        # ... and the input samples of one tile of TILE outputs
TILE = 1024             # dws_resample_tile()

_tables = {}            # (device, U, D, zeros, beta) -> h float32 [2 half + 1] on the device


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_real(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(float(v))


def check_ratio(sr_in, sr_out, zeros=10, what="resample"):
    """``(U, D)`` of a conversion the kernel runs, or ValueError naming the ratio: both rates positive integers, at most
    16384 taps (``2 zeros max(U, D) + 1``) and a tile's input span within the kernel's LDS."""
    if not (_is_int(sr_in) and _is_int(sr_out)) or sr_in < 1 or sr_out < 1:
        raise ValueError(f"{what}: {sr_in!r} -> {sr_out!r}: the sampling rates must be positive integers")
    if not _is_int(zeros) or zeros < 1:
        raise ValueError(f"{what}: zeros = {zeros!r}: expected an integer >= 1")
    g = math.gcd(int(sr_in), int(sr_out))
    U, D = int(sr_out) // g, int(sr_in) // g
    if (U, D) == (1, 1):
        return U, D
    taps = 2 * zeros * max(U, D) + 1
    if taps > MAX_TAPS:
        raise ValueError(f"{what}: {sr_in} -> {sr_out} is the ratio {U} / {D}, whose filter has {taps} taps: the kernel "
                         f"holds at most {MAX_TAPS}")
    span = ((TILE - 1) * D + taps - 1) // U + 2
    if span > MAX_SPAN:
        raise ValueError(f"{what}: {sr_in} -> {sr_out} is the ratio {U} / {D}: a tile of {TILE} outputs reads {span} input "
                         f"samples, the kernel holds at most {MAX_SPAN}")
    return U, D


def resample_filter(sr_in, sr_out, zeros=10, beta=5.0):
    """``(U, D, h)``: the reduced ratio and the float64 table ``h[0 .. 2 half]``, ``half = zeros max(U, D)``:
    ``h[n + half] = sinc(n / M) kaiser(2 half + 1, beta)[n + half]`` with ``M = max(U, D)`` (the cutoff at the lower of the
    two Nyquist frequencies), normalised to ``sum h = U``."""
    if not (_is_int(sr_in) and _is_int(sr_out)) or sr_in < 1 or sr_out < 1:
        raise ValueError(f"resample_filter: {sr_in!r} -> {sr_out!r}: the sampling rates must be positive integers")
    if not _is_int(zeros) or zeros < 1 or not _is_real(beta) or beta < 0:
        raise ValueError(f"resample_filter: zeros = {zeros!r}, beta = {beta!r}: expected an integer >= 1 and a number >= 0")
    g = math.gcd(int(sr_in), int(sr_out))
    U, D = int(sr_out) // g, int(sr_in) // g
    M = max(U, D)
    half = zeros * M
    n = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(n / M) * np.kaiser(2 * half + 1, float(beta))
    return U, D, h * (U / h.sum())


def output_length(n, U, D):
    """``ceil(n U / D)``: the samples a clip of ``n`` becomes."""
    return -((-int(n) * U) // D)


def _table(device, sr_in, sr_out, zeros, beta):
    U, D, h = resample_filter(sr_in, sr_out, zeros, beta)
    key = (device, U, D, zeros, float(beta))
    if key not in _tables:
        _tables[key] = torch.from_numpy(h.astype(np.float32)).to(device)
    return U, D, _tables[key]


def resample(x, sr_in, sr_out, lengths=None, *, zeros=10, beta=5.0):
    """``x`` ([B, T] or [B, 1, T], cuda) converted from ``sr_in`` to ``sr_out``: ``(y, out_lengths)`` with ``y`` float32
    of the same rank, ``[B, ceil(T U / D)]``, and ``out_lengths`` the list ``ceil(len_b U / D)``.  ``lengths`` (B
    integers) marks a ragged batch: clip b is its first ``lengths[b]`` samples, nothing behind them is read, and ``y``
    is exactly 0 behind ``out_lengths[b]``.  The definition is ``dws_resample``'s (include/dws.h) with the table of
    ``resample_filter``: ``scipy.signal.resample_poly(x, U, D, window=h / U)``.  A clip's row depends on its own samples
    alone, bit for bit; equal rates copy.

    ValueError before anything runs: rates that are not positive integers or a ratio the kernel refuses (named in the
    message), a bad shape or ``lengths``, ``x.requires_grad`` (no adjoint is built).  Then the device: RuntimeError for a
    CPU tensor."""
    U, D = check_ratio(sr_in, sr_out, zeros)
    if not _is_real(beta) or beta < 0:
        raise ValueError(f"resample: beta = {beta!r}: expected a number >= 0")
    if not isinstance(x, torch.Tensor) or not x.dtype.is_floating_point or x.dim() not in (2, 3) or \
            (x.dim() == 3 and x.shape[1] != 1) or x.shape[0] < 1 or x.shape[-1] < 1:
        raise ValueError(f"resample: x has shape {tuple(getattr(x, 'shape', ()))!r}, expected a non-empty float tensor "
                         "[B, T] or [B, 1, T]")
    B, T = int(x.shape[0]), int(x.shape[-1])
    host = None
    if lengths is not None:
        host = lengths.detach().cpu().tolist() if isinstance(lengths, torch.Tensor) else list(lengths)
        if len(host) != B or any(not _is_int(n) or not 1 <= n <= T for n in host):
            raise ValueError(f"resample: lengths = {host!r}: expected {B} integers in 1 .. T = {T}")
        host = [int(n) for n in host]
    if x.requires_grad:
        raise ValueError("resample: x requires grad, and the adjoint of the resampler is not built (pass x.detach())")
    if x.device.type != "cuda":
        raise RuntimeError("libdws runs on the GPU only: move the waveform to a cuda device (there is no CPU fallback)")
    lib = _lib.load()
    squeeze = x.dim() == 3
    x2 = (x[:, 0] if squeeze else x).detach().to(torch.float32).contiguous()
    dev = x2.device
    _, _, h = _table(dev, sr_in, sr_out, zeros, beta)
    T_out = output_length(T, U, D)
    y = torch.empty(B, T_out, device=dev, dtype=torch.float32)
    dev_len = host_len = None
    if host is not None:
        dev_len = torch.tensor(host, dtype=torch.int32).to(dev)
        host_len = (ctypes.c_int32 * B)(*host)
    with torch.cuda.device(dev):
        _lib.check(lib.dws_resample(x2.data_ptr(), B, T, _lib.ptr(dev_len), host_len, h.data_ptr(), int(h.shape[0]), U, D,
                                    y.data_ptr(), T_out, _lib.current_stream()))
    out_lengths = [output_length(n, U, D) for n in (host if host is not None else [T] * B)]
    return (y[:, None] if squeeze else y), out_lengths

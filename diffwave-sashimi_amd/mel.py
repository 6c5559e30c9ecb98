"""Mel-spectrogram front-end of the vocoding path on the HIP engine.

Mirrors ``dataloaders/stft.py:196-244`` (``TacotronSTFT``) and ``dataloaders/mel2samp.py:45-82``
(``load_wav_to_torch``, ``Mel2Samp.get_mel``): reflect padding by ``filter_length/2``, Hann-windowed DFT
magnitudes at hop ``hop_length``, Slaney-normalised mel filterbank, ``log(clamp(., 1e-5))``.  The transform
runs in ``dws_mel_spectrogram`` (``csrc/mel_kernels.hip``); this module builds the two constant tables on
the host (window, filterbank) and keeps the reference's call surface.

The filterbank restates the published algorithm of ``librosa.filters.mel`` (``htk=False``,
``norm='slaney'``) -- librosa itself is not a dependency here; its numbers are pinned against an independent
implementation through ``tests/golden/mel.npz`` (``tests/test_mel.py``).
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_WAV_VALUE = 32768.0     # `dataloaders/mel2samp.py:43`


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mels = f / f_sp
    min_log_hz, min_log_mel, logstep = 1000.0, 1000.0 / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, mels)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz, min_log_mel, logstep = 1000.0, 1000.0 / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr, n_fft, n_mels=80, fmin=0.0, fmax=None):
    """Slaney-style triangular mel filterbank, area-normalised: float32 ``[n_mels, n_fft//2 + 1]``."""
    fmax = sr / 2.0 if fmax is None else fmax
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return weights.astype(np.float32)


def padded_hann(win_length, filter_length):
    """``scipy.signal.get_window('hann', win_length, fftbins=True)`` centre-padded to ``filter_length``
    (`stft.py:122-126`)."""
    n = np.arange(win_length, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)
    lpad = (filter_length - win_length) // 2
    return np.pad(w, (lpad, filter_length - win_length - lpad)).astype(np.float32)


MEL_CLIP = 1e-5             # `stft.py:222-224`: log(clamp(., 1e-5))


def _mel_forward(y, win, basis, n_fft, hop, n_mels):
    B, T = y.shape
    out = torch.empty(B, n_mels, T // hop + 1, device=y.device, dtype=torch.float32)
    with torch.cuda.device(y.device):
        _lib.check(_lib.load().dws_mel_spectrogram(y.data_ptr(), B, T, win.data_ptr(), basis.data_ptr(), n_fft, hop, n_mels,
                                                   MEL_CLIP, out.data_ptr(), _lib.current_stream()))
    return out


def mel_energy(mel):
    """Frame energy of a log-mel [B, bands, frames] (natural log, ``TacotronSTFT.mel_spectrogram``):
    ``sqrt(sum_k exp(mel[b, k, f]))`` -> [B, frames], in the mel's dtype on its device.  The largest value over a
    dataset is the ``energy_max`` of ``prior_std_from_mel``."""
    if not isinstance(mel, torch.Tensor) or mel.dim() != 3:
        raise ValueError(f"mel_energy: the mel has shape {tuple(getattr(mel, 'shape', ()))!r}, expected [B, bands, frames]")
    return torch.sqrt(torch.exp(mel).sum(dim=1))


def _check_prior_range(energy_max, energy_min, std_min):
    """(e_min, e_max, std_min) as floats, or ValueError."""
    try:
        e_max, e_min, s_min = float(energy_max), float(energy_min), float(std_min)
    except (TypeError, ValueError):
        raise ValueError(f"prior: energy_max = {energy_max!r}, energy_min = {energy_min!r}, std_min = {std_min!r} "
                         "(need numbers)")
    if not (np.isfinite(e_max) and np.isfinite(e_min) and e_max > e_min):
        raise ValueError(f"prior: energy range {e_min!r} .. {e_max!r} (needs finite values, energy_max > energy_min)")
    if not 0.0 < s_min <= 1.0:
        raise ValueError(f"prior: std_min = {std_min!r} (needs 0 < std_min <= 1)")
    return e_min, e_max, s_min


def prior_std_from_mel(mel, hop, L=None, *, energy_max, energy_min=0.0, std_min=0.1):
    """Standard deviation of the adaptive prior (PriorGrad: Lee et al., ICLR 2022) from a clip's own conditioning mel::

        energy[b, f]   = sqrt(sum_k exp(mel[b, k, f]))
        sigma_f[b, f]  = clamp((energy[b, f] - energy_min) / (energy_max - energy_min), std_min, 1)
        sigma[b, 0, l] = sigma_f[b, l // hop]          l = 0 .. L-1   (default L = frames * hop)

    ``mel`` [B, bands, frames] is the engine's log-mel, ``hop`` the samples per frame (``prod(mel_upsample)``).  Each
    frame stands on its own: a clip's sigma does not depend on the batch around it.  Returns float32 [B, 1, L] on the
    mel's device: a cuda mel runs ``dws_prior_std_from_mel``, a CPU mel a plain torch evaluation.  ``energy_max`` is
    required: it is a property of the dataset (the largest ``mel_energy`` over it), and none is at hand to take a default
    from; ``std_min = 0.1`` is the paper's.  Bad arguments raise ValueError before anything runs."""
    if not isinstance(mel, torch.Tensor) or mel.dim() != 3 or not mel.dtype.is_floating_point:
        raise ValueError(f"prior_std_from_mel: the mel has shape {tuple(getattr(mel, 'shape', ()))!r}, expected a float "
                         "tensor [B, bands, frames]")
    e_min, e_max, s_min = _check_prior_range(energy_max, energy_min, std_min)
    B, bands, frames = (int(v) for v in mel.shape)
    if isinstance(hop, bool) or int(hop) != hop or int(hop) < 1:
        raise ValueError(f"prior_std_from_mel: hop = {hop!r} (needs an integer >= 1)")
    hop = int(hop)
    if B < 1 or bands < 1 or frames < 1:
        raise ValueError(f"prior_std_from_mel: empty mel {tuple(mel.shape)}")
    L = frames * hop if L is None else L
    if isinstance(L, bool) or int(L) != L or not 1 <= int(L) <= frames * hop:
        raise ValueError(f"prior_std_from_mel: L = {L!r} (needs 1 .. frames * hop = {frames * hop})")
    L = int(L)
    mel = mel.detach().to(torch.float32)
    if mel.device.type != "cuda":
        sf = ((mel_energy(mel) - e_min) / (e_max - e_min)).clamp(s_min, 1.0)
        return sf.repeat_interleave(hop, dim=1)[:, None, :L].contiguous()
    mel = mel.contiguous()
    out = torch.empty(B, 1, L, device=mel.device, dtype=torch.float32)
    with torch.cuda.device(mel.device):
        _lib.check(_lib.load().dws_prior_std_from_mel(mel.data_ptr(), B, bands, frames, hop, L, e_min, e_max, s_min,
                                                      out.data_ptr(), _lib.current_stream()))
    return out


# ---- inversion: dws_istft / dws_griffin_lim (csrc/griffinlim_kernels.hip; DESIGN.md section 4, "Mel inversion")
GL_MAX_ITERS = 4096


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_griffin_lim(n_iters, momentum, what="griffin_lim"):
    """``(n_iters, momentum)`` as an int in 0 .. 4096 and a float in [0, 1), or ValueError."""
    if not _is_int(n_iters) or not 0 <= n_iters <= GL_MAX_ITERS:
        raise ValueError(f"{what}: n_iters = {n_iters!r} (needs an integer in 0 .. {GL_MAX_ITERS})")
    if isinstance(momentum, bool) or not isinstance(momentum, (int, float, np.integer, np.floating)) or \
            not 0.0 <= float(momentum) < 1.0:
        raise ValueError(f"{what}: momentum = {momentum!r} (needs a number in [0, 1))")
    return int(n_iters), float(momentum)


def _check_spectrum(what, name, t, shape=None):
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} has shape {tuple(getattr(t, 'shape', ()))!r} and dtype "
                         f"{getattr(t, 'dtype', type(t).__name__)}, expected a float32 tensor [B, K, F]")
    if t.device.type != "cuda":
        raise ValueError(f"{what}: {name} is on {t.device}: libdws runs on the GPU only (there is no CPU path)")
    if t.requires_grad:
        raise ValueError(f"{what}: {name} requires grad: no adjoint of the inversion is built (detach it)")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected magnitude's {tuple(shape)}")


def _check_inversion(what, magnitude, phase, window, hop_length, lengths, name="magnitude"):
    """Argument checks of ``istft`` / ``griffin_lim`` / ``tv_filter`` (ValueError before anything runs); ``name`` is what
    the messages call the [B, K, F] array.  Returns ``(n_fft, hop, host)``: ``host`` the lengths as a list of ints, or
    None."""
    _check_spectrum(what, name, magnitude)
    B, K, F = (int(v) for v in magnitude.shape)
    if isinstance(phase, torch.Tensor):
        _check_spectrum(what, "phase", phase, magnitude.shape)
        if phase.device != magnitude.device:
            raise ValueError(f"{what}: phase is on {phase.device}, magnitude on {magnitude.device}")
    if not isinstance(window, torch.Tensor) or window.dim() != 1 or window.dtype != torch.float32 or \
            window.device != magnitude.device or window.requires_grad:
        raise ValueError(f"{what}: window must be a float32 tensor [n_fft] on {name}'s device that does not require grad "
                         f"(got shape {tuple(getattr(window, 'shape', ()))!r})")
    n_fft = int(window.shape[0])
    if n_fft < 64 or n_fft > 4096 or n_fft & (n_fft - 1):
        raise ValueError(f"{what}: window has {n_fft} points: n_fft must be a power of two in 64 .. 4096")
    if B < 1 or K != n_fft // 2 + 1:
        raise ValueError(f"{what}: {name} has shape {(B, K, F)}, expected K = n_fft/2 + 1 = {n_fft // 2 + 1} bins "
                         "and at least one clip")
    if not _is_int(hop_length) or hop_length < 1:
        raise ValueError(f"{what}: hop_length = {hop_length!r} (needs an integer >= 1)")
    hop = int(hop_length)
    T = (F - 1) * hop
    if T < n_fft // 2 + 1:
        raise ValueError(f"{what}: F = {F} frames at hop_length {hop} make {T} samples, reflect padding needs at least "
                         f"n_fft/2 + 1 = {n_fft // 2 + 1}")
    if lengths is None:
        return n_fft, hop, None
    host = lengths.detach().cpu().tolist() if isinstance(lengths, torch.Tensor) else list(lengths)
    if len(host) != B or (isinstance(lengths, torch.Tensor) and lengths.dim() != 1):
        raise ValueError(f"{what}: lengths has {len(host)} entries for a batch of {B} clips")
    for b, n in enumerate(host):
        if not _is_int(n) or not n_fft // 2 + 1 <= n <= T:
            raise ValueError(f"{what}: lengths: clip {b} has {n!r} samples (needs an integer in n_fft/2 + 1 = "
                             f"{n_fft // 2 + 1} .. (F - 1) hop = {T})")
        if n % hop:
            raise ValueError(f"{what}: lengths: clip {b} has {n} samples, not a multiple of hop_length = {hop}")
    return n_fft, hop, [int(n) for n in host]


def _invert(magnitude, phase, window, n_fft, hop, host, n_iters, momentum):
    lib = _lib.load()
    dev = magnitude.device
    B, _, F = (int(v) for v in magnitude.shape)
    magnitude = magnitude.contiguous()
    phase = None if phase is None else phase.contiguous()
    window = window.contiguous()
    out = torch.empty(B, (F - 1) * hop, device=dev, dtype=torch.float32)
    ws = torch.empty(lib.dws_griffin_lim_workspace(B, F, n_fft, hop, int(momentum != 0.0)) // 4, device=dev,
                     dtype=torch.float32)
    dev_len = None if host is None else torch.tensor(host, dtype=torch.int32).to(dev)
    host_len = None if host is None else (ctypes.c_int32 * B)(*host)
    with torch.cuda.device(dev):
        if n_iters is None:
            _lib.check(lib.dws_istft(magnitude.data_ptr(), _lib.ptr(phase), B, F, _lib.ptr(dev_len), host_len,
                                     window.data_ptr(), n_fft, hop, out.data_ptr(), ws.data_ptr(), _lib.current_stream()))
        else:
            _lib.check(lib.dws_griffin_lim(magnitude.data_ptr(), _lib.ptr(phase), B, F, _lib.ptr(dev_len), host_len,
                                           window.data_ptr(), n_fft, hop, n_iters, momentum, out.data_ptr(), ws.data_ptr(),
                                           _lib.current_stream()))
    return out


def istft(magnitude, phase, *, window, hop_length, lengths=None):
    """``STFT.inverse(magnitude, phase)`` of `dataloaders/stft.py:165-194` (= ``torch.istft(center=True)`` of
    ``magnitude * exp(1j * phase)``) in ``dws_istft``: magnitude and phase [B, K, F] (cuda, float32, ``K = n_fft/2 + 1``),
    ``window`` [n_fft] on the same device -> [B, (F - 1) * hop_length].  ``lengths`` (B integers, multiples of the hop)
    marks a ragged batch: clip b has ``lengths[b] // hop + 1`` frames, nothing behind them is read, and its row is exactly
    0 from ``lengths[b]`` on.  Bad arguments raise ValueError before anything runs; there is no CPU path and no adjoint."""
    if not isinstance(phase, torch.Tensor):
        raise ValueError(f"istft: phase is {type(phase).__name__}, expected a float32 tensor [B, K, F]")
    n_fft, hop, host = _check_inversion("istft", magnitude, phase, window, hop_length, lengths)
    return _invert(magnitude, phase, window, n_fft, hop, host, None, 0.0)


def griffin_lim(magnitude, *, window, hop_length, n_iters=32, momentum=0.0, phase=None, seed=0, lengths=None):
    """``griffin_lim(magnitudes, stft_fn, n_iters)`` of `dataloaders/stft.py:66-82` in ``dws_griffin_lim``: the waveform
    [B, (F - 1) * hop_length] whose STFT magnitudes approach ``magnitude`` [B, K, F] (cuda, float32).  ``phase`` is the
    start: None draws uniform phases in [-pi, pi) from a ``torch.Generator`` on the device seeded with ``seed`` (a call is
    reproducible; every clip draws its own [K, frames] from the seed, so its result does not depend on the batch around
    it), ``"zero"`` is phase 0, a tensor [B, K, F] is taken as given.  ``momentum`` in [0, 1) is Fast
    Griffin-Lim's (Perraudin et al. 2013; 0.99 is the usual choice), 0 the reference's loop.  ``n_iters = 0`` is
    ``istft(magnitude, phase)``, bit for bit.  ``lengths`` as in ``istft``.  Bad arguments raise ValueError before
    anything runs."""
    what = "griffin_lim"
    if not (phase is None or isinstance(phase, torch.Tensor) or (isinstance(phase, str) and phase == "zero")):
        raise ValueError(f"{what}: phase = {phase!r} (None for seeded random phases, \"zero\", or a tensor [B, K, F])")
    n_iters, momentum = check_griffin_lim(n_iters, momentum, what)
    if not _is_int(seed) or seed < 0:
        raise ValueError(f"{what}: seed = {seed!r} (needs a non-negative integer)")
    n_fft, hop, host = _check_inversion(what, magnitude, phase, window, hop_length, lengths)
    if phase is None:
        B, K, F = (int(v) for v in magnitude.shape)
        g = torch.Generator(device=magnitude.device)
        phase = torch.zeros_like(magnitude)
        for b in range(B):      # every clip from the seed itself: its [K, frames] phases do not depend on the batch around it
            g.manual_seed(int(seed))
            f = F if host is None else host[b] // hop + 1
            phase[b, :, :f] = (torch.rand(K, f, device=magnitude.device, dtype=torch.float32, generator=g) * 2.0 - 1.0) * np.pi
    elif isinstance(phase, str):
        phase = None
    return _invert(magnitude, phase, window, n_fft, hop, host, n_iters, momentum)


# ---- time-varying spectral filter: dws_tv_filter (csrc/tvfilter_kernels.hip; DESIGN.md section 4, "Spectral prior")
def _tv_filter_call(x, fr, fi, window, n_fft, hop, host, adjoint):
    lib = _lib.load()
    B, T = (int(v) for v in x.shape)
    F = T // hop + 1
    out = torch.empty_like(x)
    ws = torch.empty(lib.dws_griffin_lim_workspace(B, F, n_fft, hop, 0) // 4, device=x.device, dtype=torch.float32)
    dev_len = None if host is None else torch.tensor(host, dtype=torch.int32).to(x.device)
    host_len = None if host is None else (ctypes.c_int32 * B)(*host)
    with torch.cuda.device(x.device):
        _lib.check(lib.dws_tv_filter(x.data_ptr(), B, F, _lib.ptr(dev_len), host_len, fr.data_ptr(), _lib.ptr(fi),
                                     window.data_ptr(), n_fft, hop, int(adjoint), out.data_ptr(), ws.data_ptr(),
                                     _lib.current_stream()))
    return out


class _TvFilter(torch.autograd.Function):
    """``dws_tv_filter`` on ``x`` [B, T] (cuda, float32, contiguous); the backward is the same call with ``adjoint``
    flipped, as a node that cannot be differentiated again."""

    @staticmethod
    def forward(ctx, x, fr, fi, window, n_fft, hop, host, adjoint, again):
        ctx.save_for_backward(fr, fi, window)
        ctx.args = (n_fft, hop, host, adjoint, again)
        return _tv_filter_call(x, fr, fi, window, n_fft, hop, host, adjoint)

    @staticmethod
    def backward(ctx, g):
        n_fft, hop, host, adjoint, again = ctx.args
        if not again:
            raise RuntimeError("tv_filter: the second derivative is not built (the backward of dws_tv_filter is a "
                               "first-order adjoint; there is no double backward)")
        fr, fi, window = ctx.saved_tensors
        dx = _TvFilter.apply(g.to(torch.float32).contiguous(), fr, fi, window, n_fft, hop, host, not adjoint, False)
        return dx, None, None, None, None, None, None, None, None


def tv_filter(x, filt, *, window, hop_length, lengths=None, adjoint=False):
    """The time-varying spectral filter ``G+ (filt . G x)`` in ``dws_tv_filter``: ``x`` [B, T] (cuda, float32, T a multiple
    of ``hop_length``) is framed as ``mel_spectrogram`` frames it (centred, reflected about each clip's own ends), every
    frame's spectrum is multiplied by ``filt`` [B, K, T // hop_length + 1] (complex64, or float32 for a real filter;
    ``K = n_fft/2 + 1``, torch.stft's sign convention) and the frames go back through ``istft``'s normalised overlap-add
    -> [B, T].  ``adjoint=True`` is the exact transpose of that linear map (with the same ``filt``), not its inverse.
    ``window`` [n_fft] on the same device; ``lengths`` as in ``istft`` (filter frames behind a clip's own are not read).
    Differentiable in ``x``: the backward is this call with ``adjoint`` flipped; first order only (a second derivative
    is a RuntimeError).  No filter gradient is built: ``filt.requires_grad`` is a ValueError.  Bad arguments raise
    ValueError before anything runs; there is no CPU path."""
    what = "tv_filter"
    if not isinstance(filt, torch.Tensor) or filt.dim() != 3 or filt.dtype not in (torch.complex64, torch.float32):
        raise ValueError(f"{what}: filt has shape {tuple(getattr(filt, 'shape', ()))!r} and dtype "
                         f"{getattr(filt, 'dtype', type(filt).__name__)}, expected a complex64 or float32 tensor [B, K, F]")
    if filt.requires_grad:
        raise ValueError(f"{what}: filt requires grad: no gradient with respect to the filter is built (detach it)")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"{what}: x has shape {tuple(getattr(x, 'shape', ()))!r} and dtype "
                         f"{getattr(x, 'dtype', type(x).__name__)}, expected a float32 tensor [B, T]")
    if x.device.type != "cuda" or filt.device != x.device:
        raise ValueError(f"{what}: x is on {x.device}, filt on {filt.device}: libdws runs on the GPU only, on one device "
                         "(there is no CPU path)")
    if not isinstance(adjoint, (bool, np.bool_)):
        raise ValueError(f"{what}: adjoint = {adjoint!r} (needs True or False)")
    if _is_int(hop_length) and hop_length >= 1 and (x.shape[1] % hop_length or
                                                    tuple(filt.shape[::2]) != (x.shape[0], x.shape[1] // hop_length + 1)):
        raise ValueError(f"{what}: x {tuple(x.shape)} at hop_length {hop_length} needs T a multiple of the hop and filt "
                         f"[B, K, T // hop_length + 1], got {tuple(filt.shape)}")
    fr = torch.view_as_real(filt.contiguous()) if filt.is_complex() else None
    fi = None if fr is None else fr[..., 1].contiguous()
    fr = filt.contiguous() if fr is None else fr[..., 0].contiguous()
    n_fft, hop, host = _check_inversion(what, fr, None, window, hop_length, lengths, name="filt")
    window = window.contiguous()
    if x.requires_grad and torch.is_grad_enabled():
        return _TvFilter.apply(x.contiguous(), fr, fi, window, n_fft, hop, host, bool(adjoint), True)
    return _tv_filter_call(x.detach().contiguous(), fr, fi, window, n_fft, hop, host, bool(adjoint))


def _check_filter_design(ref, floor, lifter, n_fft):
    try:
        r, fl = float(ref), float(floor)
    except (TypeError, ValueError):
        raise ValueError(f"spectral_filter: ref = {ref!r}, floor = {floor!r} (need numbers)")
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"spectral_filter: ref = {ref!r} (needs a finite magnitude > 0: the one that maps to gain 1)")
    if not 0.0 < fl <= 1.0:
        raise ValueError(f"spectral_filter: floor = {floor!r} (needs 0 < floor <= 1)")
    if not _is_int(lifter) or not 1 <= lifter <= n_fft // 2 - 1:
        raise ValueError(f"spectral_filter: lifter = {lifter!r} (needs an integer in 1 .. n_fft/2 - 1 = {n_fft // 2 - 1})")
    return r, fl, int(lifter)


def minimum_phase_filter(magnitude, n_frames=None, *, ref, floor=0.01, lifter=24):
    """The filter design of ``TacotronSTFT.spectral_filter`` on linear magnitudes [B, K, frames] (any device; taken in
    float64): ``P = max(M, floor ref)^2 / ref^2``, ``c = irfft(log P, n_fft)``, ``c_mp[0] = c[0]``, ``c_mp[n] = 2 c[n]``
    for 1 <= n <= lifter, 0 elsewhere, ``F = exp(rfft(c_mp) / 2)`` -> complex64 [B, K, n_frames].  Frame f of the result
    comes from frame ``min(f, frames - 1)`` of the magnitudes (default ``n_frames = frames``)."""
    if not isinstance(magnitude, torch.Tensor) or magnitude.dim() != 3 or not magnitude.dtype.is_floating_point:
        raise ValueError(f"spectral_filter: magnitudes of shape {tuple(getattr(magnitude, 'shape', ()))!r}, expected a "
                         "float tensor [B, K, frames]")
    B, K, frames = (int(v) for v in magnitude.shape)
    n_fft = 2 * (K - 1)
    if B < 1 or frames < 1 or K < 3:
        raise ValueError(f"spectral_filter: empty magnitudes {tuple(magnitude.shape)}")
    r, fl, lifter = _check_filter_design(ref, floor, lifter, n_fft)
    n_frames = frames if n_frames is None else n_frames
    if not _is_int(n_frames) or n_frames < 1:
        raise ValueError(f"spectral_filter: {n_frames!r} frames (needs an integer >= 1)")
    m = magnitude.detach().to(torch.float64).transpose(1, 2)                # [B, frames, K]
    logp = 2.0 * torch.log(m.clamp(min=fl * r) / r)
    c = torch.fft.irfft(logp, n=n_fft, dim=-1)
    c_mp = torch.zeros_like(c)
    c_mp[..., 0] = c[..., 0]
    c_mp[..., 1:lifter + 1] = 2.0 * c[..., 1:lifter + 1]
    F = torch.exp(0.5 * torch.fft.rfft(c_mp, dim=-1))
    F.imag[..., 0] = 0.0                # exactly real at DC and Nyquist (rfft leaves rounding there at most)
    F.imag[..., -1] = 0.0
    idx = torch.arange(int(n_frames), device=F.device).clamp(max=frames - 1)
    return F[:, idx].transpose(1, 2).to(torch.complex64).contiguous()


def spectral_prior_ref(mel, stft):
    """The largest linear magnitude ``stft.mel_to_magnitude(mel)`` holds (``stft`` a ``TacotronSTFT``), as a float:
    scanned over a dataset it is the ``ref`` of ``TacotronSTFT.spectral_filter`` (the magnitude that maps to gain 1)."""
    return float(stft.mel_to_magnitude(mel).max())


class _MelBackward(torch.autograd.Function):
    """``dws_mel_spectrogram_backward`` as a node of its own, so that differentiating it (a second-order request) is
    an error with a name instead of a silent zero."""

    @staticmethod
    def forward(ctx, g, y, win, basis, n_fft, hop, n_mels):
        B, T = y.shape
        g = g.to(torch.float32).contiguous()
        dy = torch.empty_like(y)
        ws = torch.empty(B, T // hop + 1, n_fft, device=y.device, dtype=torch.float32)      # the engine allocates nothing
        with torch.cuda.device(y.device):
            _lib.check(_lib.load().dws_mel_spectrogram_backward(y.data_ptr(), B, T, win.data_ptr(), basis.data_ptr(), n_fft,
                                                                hop, n_mels, MEL_CLIP, g.data_ptr(), dy.data_ptr(),
                                                                ws.data_ptr(), _lib.current_stream()))
        return dy

    @staticmethod
    def backward(ctx, *_):
        raise RuntimeError("mel_spectrogram: the second derivative is not built (dws_mel_spectrogram_backward is a "
                           "first-order adjoint; there is no double backward)")


class _MelSpectrogram(torch.autograd.Function):
    """log-mel of ``y`` [B, T] (cuda, float32, contiguous): ``dws_mel_spectrogram`` forwards,
    ``dws_mel_spectrogram_backward`` (include/dws.h: zero gradient where a DFT magnitude is exactly 0, where torch
    autograd through sqrt gives NaN) backwards."""

    @staticmethod
    def forward(ctx, y, win, basis, n_fft, hop, n_mels):
        ctx.save_for_backward(y, win, basis)
        ctx.dims = (n_fft, hop, n_mels)
        return _mel_forward(y, win, basis, n_fft, hop, n_mels)

    @staticmethod
    def backward(ctx, g):
        y, win, basis = ctx.saved_tensors
        return _MelBackward.apply(g, y, win, basis, *ctx.dims), None, None, None, None, None


class TacotronSTFT:
    """``dataloaders/stft.py:196-244``; ``mel_spectrogram(y)`` runs on the GPU ``y`` lives on."""

    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80, sampling_rate=22050,
                 mel_fmin=0.0, mel_fmax=8000.0):
        assert filter_length >= win_length
        self.filter_length, self.hop_length, self.win_length = filter_length, hop_length, win_length
        self.n_mel_channels, self.sampling_rate = n_mel_channels, sampling_rate
        self.mel_basis = torch.from_numpy(mel_filterbank(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax))
        self.window = torch.from_numpy(padded_hann(win_length, filter_length))
        self._dev = {}
        self._pinv, self._pinv_dev = None, {}

    def _tables(self, device):
        if device not in self._dev:
            self._dev[device] = (self.window.to(device), self.mel_basis.to(device))
        return self._dev[device]

    def differentiable_mel(self, y):
        """``y`` [B, T] (cuda, any range) -> log-mel [B, n_mel_channels, T // hop + 1] through ``_MelSpectrogram``:
        differentiable in ``y`` where it requires grad, the plain kernel call (the same bits) where it does not."""
        if y.device.type != "cuda":
            raise RuntimeError("libdws runs on the GPU only: move the waveform to cuda (there is no CPU fallback)")
        if y.dim() != 2:
            raise ValueError(f"mel_spectrogram: the waveform has shape {tuple(y.shape)}, expected [B, T]")
        win, basis = self._tables(y.device)
        dims = (self.filter_length, self.hop_length, self.n_mel_channels)
        if y.requires_grad and torch.is_grad_enabled():
            return _MelSpectrogram.apply(y.to(torch.float32).contiguous(), win, basis, *dims)
        return _mel_forward(y.detach().to(torch.float32).contiguous(), win, basis, *dims)

    def mel_spectrogram(self, y):
        """``y`` [B, T] in [-1, 1] (cuda) -> log-mel [B, n_mel_channels, T // hop + 1].  Where ``y`` requires grad the
        result carries a ``grad_fn`` (the reference detaches; the adjoint is ``dws_mel_spectrogram_backward``: first
        order only, and a zero gradient where torch autograd through ``sqrt(0)`` would give NaN); otherwise this is the
        plain kernel call."""
        if y.device.type != "cuda":
            raise RuntimeError("libdws runs on the GPU only: move the waveform to cuda (there is no CPU fallback)")
        assert float(y.min()) >= -1 and float(y.max()) <= 1            # `stft.py:233-234`
        return self.differentiable_mel(y)

    # ---- the other direction (`stft.py:66-82,165-194`): istft / griffin_lim of this module at the object's STFT keys
    def inverse(self, magnitude, phase):
        """``STFT.inverse(magnitude, phase)``: [B, K, F] (cuda, float32) twice -> [B, (F - 1) * hop_length]."""
        _check_spectrum("inverse", "magnitude", magnitude)
        return istft(magnitude, phase, window=self._tables(magnitude.device)[0], hop_length=self.hop_length)

    def griffin_lim(self, magnitude, n_iters=32, momentum=0.0, phase=None, seed=0, lengths=None):
        """``griffin_lim`` of this module on linear magnitudes [B, K, F] at the object's own STFT keys."""
        _check_spectrum("griffin_lim", "magnitude", magnitude)
        return griffin_lim(magnitude, window=self._tables(magnitude.device)[0], hop_length=self.hop_length, n_iters=n_iters,
                           momentum=momentum, phase=phase, seed=seed, lengths=lengths)

    def mel_pinv(self):
        """``numpy.linalg.pinv`` of the filterbank in float64: [K, n_mel_channels]."""
        if self._pinv is None:
            self._pinv = np.linalg.pinv(self.mel_basis.numpy().astype(np.float64))
        return self._pinv

    def mel_to_magnitude(self, mel):
        """Log-mel [B, n_mel_channels, F] (cuda, float32; ``mel_spectrogram``'s output) -> linear magnitudes [B, K, F]:
        ``clamp(P @ exp(mel), min=0)`` with ``P = mel_pinv()``, the least-squares inverse of the filterbank (cached per
        device in float64).  One torch matmul per call, taken in float64 and rounded to float32 once; NNLS inversion is
        not built."""
        if not isinstance(mel, torch.Tensor) or mel.dim() != 3 or mel.dtype != torch.float32 or \
                mel.shape[1] != self.n_mel_channels:
            raise ValueError(f"mel_to_magnitude: the mel has shape {tuple(getattr(mel, 'shape', ()))!r} and dtype "
                             f"{getattr(mel, 'dtype', type(mel).__name__)}, expected a float32 tensor "
                             f"[B, {self.n_mel_channels}, frames]")
        if mel.device.type != "cuda":
            raise ValueError(f"mel_to_magnitude: the mel is on {mel.device}: libdws runs on the GPU only (there is no CPU path)")
        if mel.requires_grad:
            raise ValueError("mel_to_magnitude: the mel requires grad: no adjoint of the inversion is built (detach it)")
        if mel.device not in self._pinv_dev:
            self._pinv_dev[mel.device] = torch.from_numpy(self.mel_pinv()).to(mel.device)
        # the product in float64, rounded once: a float32 GEMM adds the bands in an order that depends on the batch's
        # shape, and a clip's magnitudes (so its inversion) must not depend on the batch around it
        return torch.matmul(self._pinv_dev[mel.device], torch.exp(mel).double()).clamp_(min=0.0).float()

    def spectral_filter(self, mel, L=None, *, ref, floor=0.01, lifter=24):
        """The noise-shaping filter of the spectral prior (SpecGrad: Koizumi et al., Interspeech 2022) from a clip's own
        log-mel [B, n_mel_channels, frames] (cuda, float32): complex64 [B, K, L // hop_length + 1] on the mel's device
        (default ``L = frames * hop_length``, a multiple of the hop), the ``filt`` of ``tv_filter``.  Per frame, with
        ``M = mel_to_magnitude(mel)``::

            P    = max(M, floor * ref)^2 / ref^2                 the envelope, 1 at the magnitude ``ref``
            c    = irfft(log P, n_fft)                           its cepstrum
            c_mp = c[0], 2 c[1 .. lifter], 0 elsewhere           liftered and folded: the minimum-phase cepstrum
            F    = exp(rfft(c_mp) / 2)

        so ``|F|^2`` is the cepstrally smoothed envelope, F is minimum phase and its imaginary part is 0 at DC and
        Nyquist.  Frame f of the filter comes from mel frame ``min(f, frames - 1)``: a training segment's mel has L / hop
        frames, the framing L / hop + 1.  Everything runs in float64 torch and is rounded to complex64 once (a
        ``torch.fft`` over [B, frames, n_fft]: not the hot path).  ``ref`` is required: the magnitude that maps to gain
        1, a property of the dataset (``spectral_prior_ref`` scans for it); ``floor`` in (0, 1] keeps ``1 / F`` finite,
        ``lifter`` in 1 .. n_fft/2 - 1 is the number of cepstral coefficients kept.  The inverse filter of the training
        loss is ``1 / F``: ``tv_filter(., 1 / F)`` stands for the inverse of ``tv_filter(., F)`` as in the paper -- an
        approximation (frames overlap and the window is not flat), not an exact inverse.  Bad arguments raise
        ValueError."""
        r, fl, lifter = _check_filter_design(ref, floor, lifter, self.filter_length)
        mag = self.mel_to_magnitude(mel)
        frames = int(mag.shape[-1])
        L = frames * self.hop_length if L is None else L
        if not _is_int(L) or L < self.hop_length or L % self.hop_length or L > frames * self.hop_length:
            raise ValueError(f"spectral_filter: L = {L!r} (needs a multiple of hop_length = {self.hop_length} in "
                             f"{self.hop_length} .. frames * hop_length = {frames * self.hop_length})")
        return minimum_phase_filter(mag, int(L) // self.hop_length + 1, ref=r, floor=fl, lifter=lifter)

    def spectral_prior_ref(self, mel):
        """``spectral_prior_ref(mel, self)``."""
        return spectral_prior_ref(mel, self)

    def mel_to_audio(self, mel, n_iters=32, momentum=0.0, seed=0, lengths=None):
        """``griffin_lim(mel_to_magnitude(mel))`` from seeded random phases: log-mel [B, n_mel_channels, F] ->
        [B, (F - 1) * hop_length].  ``lengths`` (samples, multiples of the hop) as in ``griffin_lim``."""
        check_griffin_lim(n_iters, momentum, "mel_to_audio")
        return self.griffin_lim(self.mel_to_magnitude(mel), n_iters=n_iters, momentum=momentum, seed=seed, lengths=lengths)


def load_wav_to_torch(full_path):
    """``dataloaders/mel2samp.py:51-56``: raw sample values as float32 (int16 range), and the rate."""
    from scipy.io.wavfile import read
    sampling_rate, data = read(full_path)
    return torch.from_numpy(np.ascontiguousarray(data)).float(), sampling_rate


class Mel2Samp:
    """The ``get_mel`` half of ``dataloaders/mel2samp.py:59-82`` (the dataset half is not built)."""

    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, sampling_rate=22050, mel_fmin=0.0,
                 mel_fmax=8000.0, **_ignored):
        self.stft = TacotronSTFT(filter_length=filter_length, hop_length=hop_length, win_length=win_length,
                                 sampling_rate=sampling_rate, mel_fmin=mel_fmin, mel_fmax=mel_fmax)
        self.sampling_rate = sampling_rate

    def get_mel(self, audio):
        audio_norm = (audio / MAX_WAV_VALUE).unsqueeze(0)
        return self.stft.mel_spectrogram(audio_norm.cuda()).squeeze(0)

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

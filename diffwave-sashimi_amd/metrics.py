"""Objective audio metrics between generated and reference waveforms on the HIP engine (not in the reference).

``spectral_metrics(x, y)`` compares two batches of time-aligned waveforms and returns, per clip,

* ``mr_stft``: Parallel WaveGAN's multi-resolution STFT distance (Yamamoto et al., ICASSP 2020), the mean over the
  resolutions of spectral convergence + log-magnitude L1 -- and both terms per resolution, ``sc_{n_fft}_{hop}_{win}`` /
  ``mag_{n_fft}_{hop}_{win}``;
* ``ls_mae``: the mean absolute difference of the engine's log-mel spectrograms (PriorGrad's LS-MAE);
* ``lsd``: the log-spectral distance, the mean over frames of ``sqrt(mean_k (log10|Y|^2 - log10|X|^2)^2)``;
* ``mcd``: a mel-cepstral distortion in dB (Kubichek 1993), see ``spectral_metrics``.

The transform and every sum run in ``dws_spectral_distance`` (``csrc/spectral_kernels.hip``), one fused launch per
resolution; this module builds the constant tables, checks the arguments and divides the sums.  There is no CPU path.

``mr_stft_loss(x, y)`` is ``mr_stft`` as a training loss: float32 [B] on the device, differentiable in ``x`` through
``dws_spectral_loss_backward`` (the hand-written adjoint of the two terms; DESIGN.md section 4, "Spectral loss").

``pitch_metrics(x, y)`` is the pitch family (YIN tracks of both signals, ``dws_pitch_distance``) and ``stoi(x, y)`` the
intelligibility family: STOI and ESTOI at 10 kHz (``dws_stoi`` on top of ``audio.resample``; DESIGN.md section 4,
"Pitch metrics" and "Intelligibility metrics").
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .mel import MEL_CLIP, TacotronSTFT, padded_hann

# (n_fft, hop, win) of Parallel WaveGAN's multi-resolution STFT loss
MR_STFT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
N_FFT_MIN, N_FFT_MAX = 64, 2048
SUMS = ("sc_num", "sc_den", "mag_abs", "lsd_sum", "mel_abs", "mcd_sum")      # the columns of ``spectral_sums``
MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)

_default = None
_windows = {}       # (device, n_fft, win) -> window [n_fft]
_ceps = {}          # (device, n_cep, n_mels) -> D [n_cep, n_mels] (float64)


def default_stft():
    """The ``TacotronSTFT()`` of the defaults (LJSpeech's transform), built once."""
    global _default
    if _default is None:
        _default = TacotronSTFT()
    return _default


def cepstral_table(n_cep, n_mels):
    """``D[d-1, k] = sqrt(2 / K) cos(pi d (k + 1/2) / K)``, ``d = 1 .. n_cep``, ``K = n_mels``: rows 1 .. n_cep of the
    orthonormal DCT-II (row 0, the frame's level, is left out as in every MCD).  float64 ``[n_cep, n_mels]``."""
    d = torch.arange(1, n_cep + 1, dtype=torch.float64)[:, None]
    k = torch.arange(n_mels, dtype=torch.float64)[None, :]
    return math.sqrt(2.0 / n_mels) * torch.cos(math.pi * d * (k + 0.5) / n_mels)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_resolution(n_fft, hop, win, lengths):
    """ValueError unless ``(n_fft, hop, win)`` is a resolution the kernel runs on clips of these ``lengths`` (host
    integers): ``n_fft`` a power of two in 64 .. 2048, ``1 <= win <= n_fft``, ``hop >= 1``, every clip at least
    ``n_fft / 2 + 1`` samples long (reflect padding; nothing is clamped)."""
    res = f"resolution (n_fft={n_fft!r}, hop={hop!r}, win={win!r})"
    if not (_is_int(n_fft) and _is_int(hop) and _is_int(win)):
        raise ValueError(f"spectral_metrics: {res}: expected three integers")
    if not (N_FFT_MIN <= n_fft <= N_FFT_MAX) or n_fft & (n_fft - 1):
        raise ValueError(f"spectral_metrics: {res}: n_fft must be a power of two in {N_FFT_MIN} .. {N_FFT_MAX}")
    if not 1 <= win <= n_fft:
        raise ValueError(f"spectral_metrics: {res}: win must be in 1 .. n_fft")
    if hop < 1:
        raise ValueError(f"spectral_metrics: {res}: hop must be at least 1")
    for b, n in enumerate(lengths):
        if n < n_fft // 2 + 1:
            raise ValueError(f"spectral_metrics: {res}: clip {b} has {n} samples, reflect padding needs at least "
                             f"n_fft/2 + 1 = {n_fft // 2 + 1}")


def _pair(x, y, lengths, what="spectral_metrics"):
    """Shape checks of a pair of batches (ValueError): the two as [B, T] views and the host lengths."""
    for name, t in (("x", x), ("y", y)):
        if not isinstance(t, torch.Tensor) or not t.dtype.is_floating_point or t.dim() not in (2, 3) or \
                (t.dim() == 3 and t.shape[1] != 1):
            raise ValueError(f"{what}: {name} has shape {tuple(getattr(t, 'shape', ()))!r}, expected a float "
                             "tensor [B, T] or [B, 1, T]")
    x = x[:, 0] if x.dim() == 3 else x
    y = y[:, 0] if y.dim() == 3 else y
    if x.shape != y.shape or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{what}: x {tuple(x.shape)} and y {tuple(y.shape)} must be two equal non-empty batches")
    B, T = (int(v) for v in x.shape)
    if lengths is None:
        return x, y, None, [T] * B
    host = lengths.detach().cpu().tolist() if isinstance(lengths, torch.Tensor) else list(lengths)
    if len(host) != B or (isinstance(lengths, torch.Tensor) and lengths.dim() != 1):
        raise ValueError(f"{what}: lengths has {len(host)} entries for a batch of {B} clips")
    if any(not _is_int(n) or not 1 <= n <= T for n in host):
        raise ValueError(f"{what}: lengths = {host!r}: expected integers in 1 .. T = {T}")
    return x, y, [int(n) for n in host], [int(n) for n in host]


def _need_gpu(x, y):
    if x.device.type != "cuda" or y.device != x.device:
        raise RuntimeError("libdws runs on the GPU only: move both waveforms to one cuda device (there is no CPU fallback)")


def _f32(*waves):
    """The waveforms detached, float32 and contiguous, as a tuple: what the kernels read."""
    return tuple(w.detach().to(torch.float32).contiguous() for w in waves)


def _length_args(host, dev, B, dev_len=None):
    """The ``(lengths, lengths_host)`` pair of a C entry point from the host integers (``(None, None)`` without them):
    an int32 tensor on ``dev`` -- ``dev_len`` where the caller already holds one -- and a ctypes array."""
    if host is None:
        return None, None
    return (torch.tensor(host, dtype=torch.int32).to(dev) if dev_len is None else dev_len), (ctypes.c_int32 * B)(*host)


def _window(device, n_fft, win):
    key = (device, n_fft, win)
    if key not in _windows:
        _windows[key] = torch.from_numpy(padded_hann(win, n_fft)).to(device)
    return _windows[key]


def _cep(device, n_cep, n_mels):
    key = (device, n_cep, n_mels)
    if key not in _ceps:
        _ceps[key] = cepstral_table(n_cep, n_mels).to(device).contiguous()
    return _ceps[key]


def _run(x, y, host, n_fft, hop, win, basis, cep, dev_len=None):
    """One ``dws_spectral_distance`` call on checked arguments: float64 [B, 6] on the device.  ``dev_len``: ``host`` as an
    int32 device tensor where the caller already holds one."""
    lib = _lib.load()
    B, T = x.shape
    dev = x.device
    out = torch.empty(B, len(SUMS), device=dev, dtype=torch.float64)
    ws = torch.empty(lib.dws_spectral_distance_workspace(B, T, hop) // 8, device=dev, dtype=torch.float64)
    dev_len, host_len = _length_args(host, dev, B, dev_len)
    n_mels = 0 if basis is None else int(basis.shape[0])
    n_cep = 0 if cep is None else int(cep.shape[0])
    with torch.cuda.device(dev):
        _lib.check(lib.dws_spectral_distance(x.data_ptr(), y.data_ptr(), B, T, _lib.ptr(dev_len), host_len,
                                             _window(dev, n_fft, win).data_ptr(), n_fft, hop, _lib.ptr(basis), n_mels,
                                             MEL_CLIP, _lib.ptr(cep), n_cep, ws.data_ptr(), out.data_ptr(),
                                             _lib.current_stream()))
    return out


def spectral_sums(x, y, lengths=None, *, n_fft, hop, win, mel_basis=None, n_cep=0):
    """The six sums of ``dws_spectral_distance`` (include/dws.h) at one resolution, columns ``SUMS``: float64 [B, 6] on
    the CPU.  ``mel_basis`` [n_mels, n_fft/2 + 1] adds ``mel_abs`` and, with ``n_cep`` > 0, ``mcd_sum``.  A clip's row
    depends on its own samples and length alone, bit for bit.  Arguments are checked first (ValueError), then the
    device (RuntimeError)."""
    x, y, host, lens = _pair(x, y, lengths)
    check_resolution(n_fft, hop, win, lens)
    if mel_basis is not None and tuple(mel_basis.shape) != (mel_basis.shape[0], n_fft // 2 + 1):
        raise ValueError(f"spectral_sums: mel_basis {tuple(mel_basis.shape)} does not have n_fft/2 + 1 = {n_fft // 2 + 1} columns")
    if not _is_int(n_cep) or n_cep < 0 or n_cep > 256 or (n_cep and mel_basis is None):
        raise ValueError(f"spectral_sums: n_cep = {n_cep!r} (0 .. 256, and a mel_basis with it)")
    _need_gpu(x, y)
    x, y = _f32(x, y)
    basis = None if mel_basis is None else mel_basis.to(device=x.device, dtype=torch.float32).contiguous()
    cep = _cep(x.device, n_cep, int(basis.shape[0])) if n_cep else None
    return _run(x, y, host, n_fft, hop, win, basis, cep).cpu()


def resolution_key(res):
    return "{}_{}_{}".format(*res)


def spectral_metrics(x, y, lengths=None, *, stft=None, resolutions=MR_STFT_RESOLUTIONS, n_cep=13):
    """Objective distances of generated ``x`` from reference ``y`` ([B, T] or [B, 1, T], cuda), clip by clip; ``lengths``
    (B integers) marks ragged batches: clip b is its first ``lengths[b]`` samples, nothing behind them is read.  Returns a
    dict of float64 [B] CPU tensors:

    ``sc_{n_fft}_{hop}_{win}``, ``mag_{n_fft}_{hop}_{win}`` for each of ``resolutions`` (default: Parallel WaveGAN's three):
    spectral convergence ``sqrt(sum (|Y|-|X|)^2 / sum |Y|^2)`` and the mean ``|ln|Y| - ln|X||`` over bins and frames,
    magnitudes floored at ``sqrt(1e-7)``; ``mr_stft``: the mean over the resolutions of ``sc + mag``.

    From one more pass at ``stft``'s own ``filter_length / hop_length / win_length`` with its mel filterbank (default
    ``TacotronSTFT()``): ``ls_mae``, the mean ``|logmel(Y) - logmel(X)|`` over bands and frames (what
    ``generate.report_mel`` prints, for pairs of waveforms); ``lsd``, the mean over frames of the root mean square over bins
    of ``log10|Y|^2 - log10|X|^2``; ``mcd = (10 sqrt 2 / ln 10) mean_f ||D (logmel(Y)_f - logmel(X)_f)||`` in dB with
    ``D = cepstral_table(n_cep, n_mels)``.

    ``mcd`` is an MFCC-style distortion of TIME-ALIGNED signals on the engine's own log-mel: there is no dynamic time
    warping and no SPTK mel-cepstral analysis, so its absolute values are not those of the papers that report MCD (PriorGrad
    among them); it orders systems evaluated with this function.  Every frame of a clip counts (``f = 0 .. len // hop``).

    Arguments are checked before anything runs: a resolution the kernel does not build or a clip shorter than
    ``n_fft / 2 + 1`` raises ValueError naming the resolution and the clip; CPU tensors raise RuntimeError."""
    stft = default_stft() if stft is None else stft
    x, y, host, lens = _pair(x, y, lengths)
    resolutions = check_resolutions(resolutions, lens)
    own = (stft.filter_length, stft.hop_length, stft.win_length)
    check_resolution(*own, lens)
    if not _is_int(n_cep) or not 1 <= n_cep <= min(256, stft.n_mel_channels - 1):
        raise ValueError(f"spectral_metrics: n_cep = {n_cep!r} (1 .. min(256, n_mel_channels - 1))")
    _need_gpu(x, y)
    x, y = _f32(x, y)
    out = {}
    total = 0.0
    for r in resolutions:
        n_fft, hop, _ = r
        s = _run(x, y, host, *r, None, None).cpu()
        frames = torch.tensor([n // hop + 1 for n in lens], dtype=torch.float64)
        sc = torch.sqrt(s[:, 0] / s[:, 1])
        mag = s[:, 2] / (frames * (n_fft // 2 + 1))
        out["sc_" + resolution_key(r)], out["mag_" + resolution_key(r)] = sc, mag
        total = total + sc + mag
    out["mr_stft"] = total / len(resolutions)
    _, basis = stft._tables(x.device)
    s = _run(x, y, host, *own, basis, _cep(x.device, n_cep, stft.n_mel_channels)).cpu()
    frames = torch.tensor([n // own[1] + 1 for n in lens], dtype=torch.float64)
    out["ls_mae"] = s[:, 4] / (frames * stft.n_mel_channels)
    out["lsd"] = s[:, 3] / frames
    out["mcd"] = MCD_DB * s[:, 5] / frames
    return out


METRICS = ("mr_stft", "ls_mae", "lsd", "mcd")       # the four headline numbers, in the order they are printed


# ---- pitch: dws_pitch_track / dws_pitch_distance (csrc/pitch_kernels.hip; DESIGN.md section 4, "Pitch metrics")
PITCH_METRICS = ("f0_rmse", "f0_cents", "gpe", "vuv_error", "vuv_f1", "periodicity_rmse")      # in print order
PITCH_SUMS = ("voiced_both", "f0_sq", "cents_sq", "voiced_y", "voiced_x", "vuv_differ", "periodicity_sq", "gross")
PITCH_DEFAULTS = dict(sampling_rate=22050, hop=256, win=1024, fmin=50.0, fmax=550.0, threshold=0.15)
PITCH_WIN_MIN, PITCH_WIN_MAX, PITCH_LAG_MAX = 64, 2048, 2048


def _is_real(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(float(v))


def pitch_lags(sampling_rate, fmin, fmax):
    """``(tau_lo, tau_hi) = (floor(sr / fmax), ceil(sr / fmin))``: the lags the tracker searches."""
    return int(math.floor(sampling_rate / fmax)), int(math.ceil(sampling_rate / fmin))


def check_pitch(lengths, sampling_rate=22050, hop=256, win=1024, fmin=50.0, fmax=550.0, threshold=0.15,
                what="pitch_metrics"):
    """``(tau_lo, tau_hi)`` of parameters the kernel runs on clips of these ``lengths`` (host integers), or ValueError
    naming the parameter (and the clip): ``win`` in 64 .. 2048, ``M = tau_hi + 1 <= 2048``, ``2 <= tau_lo < tau_hi``,
    ``hop >= 1``, ``threshold`` inside (0, 1), every clip at least ``(win + M + 1) // 2 + 1`` samples long (reflect
    padding; nothing is clamped)."""
    if not _is_real(sampling_rate) or sampling_rate <= 0:
        raise ValueError(f"{what}: sampling_rate = {sampling_rate!r}: expected a number > 0")
    if not _is_int(win) or not PITCH_WIN_MIN <= win <= PITCH_WIN_MAX:
        raise ValueError(f"{what}: win = {win!r}: expected an integer in {PITCH_WIN_MIN} .. {PITCH_WIN_MAX}")
    if not _is_int(hop) or hop < 1:
        raise ValueError(f"{what}: hop = {hop!r}: expected an integer >= 1")
    if not _is_real(threshold) or not 0.0 < float(np.float32(threshold)) < 1.0:
        raise ValueError(f"{what}: threshold = {threshold!r}: expected a number inside (0, 1)")
    if not _is_real(fmin) or not _is_real(fmax) or fmin <= 0 or fmax <= 0:
        raise ValueError(f"{what}: fmin = {fmin!r}, fmax = {fmax!r}: expected two numbers > 0")
    tau_lo, tau_hi = pitch_lags(sampling_rate, fmin, fmax)
    if tau_hi + 1 > PITCH_LAG_MAX:
        raise ValueError(f"{what}: fmin = {fmin!r} at sampling_rate = {sampling_rate!r} needs lags up to M = {tau_hi + 1}: "
                         f"the kernel computes at most {PITCH_LAG_MAX}")
    if tau_lo < 2:
        raise ValueError(f"{what}: fmax = {fmax!r} at sampling_rate = {sampling_rate!r} gives tau_lo = {tau_lo}: the "
                         "smallest lag must be at least 2")
    if tau_lo >= tau_hi:
        raise ValueError(f"{what}: fmin = {fmin!r}, fmax = {fmax!r} give lags {tau_lo} .. {tau_hi}: tau_lo must lie below tau_hi")
    need = (win + tau_hi + 2) // 2 + 1
    for b, n in enumerate(lengths):
        if n < need:
            raise ValueError(f"{what}: clip {b} has {n} samples, reflect padding at win = {win} and lags up to "
                             f"{tau_hi + 1} needs at least (win + M + 1) // 2 + 1 = {need}")
    return tau_lo, tau_hi


def pitch_track(x, lengths=None, *, sampling_rate=22050, hop=256, win=1024, fmin=50.0, fmax=550.0, threshold=0.15):
    """YIN pitch track (de Cheveigne & Kawahara, 2002; fixed threshold) of ``x`` ([B, T] or [B, 1, T], cuda):
    ``(f0, periodicity)``, both float32 [B, T // hop + 1] on the device.  Frame ``f`` is centred on sample ``f hop`` (the
    frames of ``spectral_metrics`` at that hop, ``f = 0 .. len // hop``); ``f0`` is in Hz and 0 on an unvoiced frame,
    ``periodicity`` is ``1 - d'`` at the chosen lag (at the smallest ``d'`` of the search range on an unvoiced frame),
    clamped to [0, 1].  ``lengths`` as in ``spectral_metrics``; frames behind a clip's last are exactly (0, 0).  The
    definitions are those of ``dws_pitch_track`` (include/dws.h).  Arguments are checked first (ValueError naming the
    parameter and the clip), then the device (RuntimeError)."""
    x, _, host, lens = _pair(x, x, lengths, "pitch_track")
    tau_lo, tau_hi = check_pitch(lens, sampling_rate, hop, win, fmin, fmax, threshold, "pitch_track")
    _need_gpu(x, x)
    (x,) = _f32(x)
    lib = _lib.load()
    B, T = x.shape
    track = torch.empty(B, T // hop + 1, 2, device=x.device, dtype=torch.float32)
    dev_len, host_len = _length_args(host, x.device, B)
    with torch.cuda.device(x.device):
        _lib.check(lib.dws_pitch_track(x.data_ptr(), B, T, _lib.ptr(dev_len), host_len, hop, win, tau_lo, tau_hi,
                                       float(threshold), float(sampling_rate), track.data_ptr(), _lib.current_stream()))
    return track[:, :, 0].contiguous(), track[:, :, 1].contiguous()


def _pitch_sums(what, x, y, lengths, sampling_rate, hop, win, fmin, fmax, threshold):
    """``pitch_sums`` and the host lengths of the clips."""
    x, y, host, lens = _pair(x, y, lengths, what)
    tau_lo, tau_hi = check_pitch(lens, sampling_rate, hop, win, fmin, fmax, threshold, what)
    _need_gpu(x, y)
    x, y = _f32(x, y)
    return _pitch_run(x, y, host, sampling_rate, hop, win, tau_lo, tau_hi, threshold).cpu(), lens


def _pitch_run(x, y, host, sampling_rate, hop, win, tau_lo, tau_hi, threshold):
    """One ``dws_pitch_distance`` call on checked arguments: float64 [B, 8] on the device."""
    lib = _lib.load()
    B, T = x.shape
    dev = x.device
    out = torch.empty(B, len(PITCH_SUMS), device=dev, dtype=torch.float64)
    ws = torch.empty(lib.dws_pitch_distance_workspace(B, T, hop) // 4, device=dev, dtype=torch.float32)
    dev_len, host_len = _length_args(host, dev, B)
    with torch.cuda.device(dev):
        _lib.check(lib.dws_pitch_distance(x.data_ptr(), y.data_ptr(), B, T, _lib.ptr(dev_len), host_len, hop, win, tau_lo,
                                          tau_hi, float(threshold), float(sampling_rate), ws.data_ptr(), out.data_ptr(),
                                          _lib.current_stream()))
    return out


def pitch_sums(x, y, lengths=None, *, sampling_rate=22050, hop=256, win=1024, fmin=50.0, fmax=550.0, threshold=0.15):
    """The eight sums of ``dws_pitch_distance`` (include/dws.h), columns ``PITCH_SUMS``: float64 [B, 8] on the CPU.  A
    clip's row depends on its own samples and length alone, bit for bit.  Arguments are checked first (ValueError), then
    the device (RuntimeError)."""
    return _pitch_sums("pitch_sums", x, y, lengths, sampling_rate, hop, win, fmin, fmax, threshold)[0]


def pitch_metrics(x, y, lengths=None, *, sampling_rate=22050, hop=256, win=1024, fmin=50.0, fmax=550.0, threshold=0.15):
    """Pitch distances of generated ``x`` from reference ``y`` ([B, T] or [B, 1, T], cuda), clip by clip, from the YIN
    tracks of the two (``pitch_track``).  Returns a dict of float64 [B] CPU tensors; with ``vv`` the frames voiced in both:

    ``f0_rmse``: ``sqrt(mean_vv (f0x - f0y)^2)`` in Hz (PriorGrad's F0 RMSE); ``f0_cents``: the same of
    ``1200 log2(f0x / f0y)``; ``gpe``: the share of ``vv`` frames with ``|f0x / f0y - 1| > 0.2`` (gross pitch errors);
    ``vuv_error``: the share of ALL frames on which the voicing decisions differ; ``vuv_f1``:
    ``2 #vv / (#voiced_x + #voiced_y)``; ``periodicity_rmse``: ``sqrt(mean (p_x - p_y)^2)`` over all frames; ``frames``
    (``len // hop + 1``) and ``voiced_both`` (``#vv``).

    NaN: ``f0_rmse``, ``f0_cents`` and ``gpe`` of a clip with no frame voiced in both signals, ``vuv_f1`` where neither
    signal has a voiced frame.  ``vuv_error`` and ``periodicity_rmse`` are always finite.

    This is plain YIN with a fixed threshold: no pYIN / Viterbi smoothing, not CREPE or WORLD, so the absolute values are
    not those of the papers that report these metrics; it orders systems evaluated with this function.  Arguments are
    checked before anything runs (ValueError naming the parameter and the clip); CPU tensors raise RuntimeError."""
    s, lens = _pitch_sums("pitch_metrics", x, y, lengths, sampling_rate, hop, win, fmin, fmax, threshold)
    frames = torch.tensor([n // hop + 1 for n in lens], dtype=torch.float64)
    return {"f0_rmse": torch.sqrt(s[:, 1] / s[:, 0]), "f0_cents": torch.sqrt(s[:, 2] / s[:, 0]), "gpe": s[:, 7] / s[:, 0],
            "vuv_error": s[:, 5] / frames, "vuv_f1": 2.0 * s[:, 0] / (s[:, 3] + s[:, 4]),
            "periodicity_rmse": torch.sqrt(s[:, 6] / frames), "frames": frames, "voiced_both": s[:, 0].clone()}


# ---- intelligibility: dws_stoi on top of dws_resample (csrc/stoi_kernels.hip; DESIGN.md section 4, "Intelligibility metrics")
STOI_METRICS = ("stoi", "estoi")
STOI_SUMS = ("stoi_sum", "estoi_sum", "segments", "frames_kept")
# Taal's constants (Taal et al. 2011): 10 kHz, 256-sample frames at hop 128, a 512-point DFT, 15 third-octave bands from
# 150 Hz, segments of 30 frames (384 ms), clipping at beta = -15 dB, 40 dB of dynamic range for the silent-frame removal
STOI_DEFAULTS = dict(fs=10000, frame=256, hop=128, n_fft=512, n_bands=15, f_min=150.0, segment=30, beta=-15.0, dyn_range=40.0)

_stoi_tables = {}   # device -> (window [frame], obm [n_bands, n_fft/2 + 1]) float32


def third_octave_bands(fs=10000, n_fft=512, n_bands=15, f_min=150.0):
    """``(obm, centres)``: the 0 / 1 band matrix float64 ``[n_bands, n_fft/2 + 1]`` and the centre frequencies
    ``f_min 2^(k/3)``.  Band k has the edges ``centre 2^(-1/6)`` and ``centre 2^(+1/6)``, each moved to the nearest DFT bin
    (bin q is ``q fs / n_fft`` Hz), and holds the bins ``[lo, hi)``."""
    f = np.linspace(0.0, fs, n_fft + 1)[:n_fft // 2 + 1]
    centres = f_min * 2.0 ** (np.arange(n_bands, dtype=np.float64) / 3.0)
    obm = np.zeros((n_bands, len(f)), dtype=np.float64)
    for k, c in enumerate(centres):
        lo = int(np.argmin((f - c * 2.0 ** (-1.0 / 6.0)) ** 2))
        hi = int(np.argmin((f - c * 2.0 ** (1.0 / 6.0)) ** 2))
        obm[k, lo:hi] = 1.0
    return obm, centres


def stoi_window(frame=256):
    """``hanning(frame + 2)[1:-1]``: the Hann window without its two zeros, float64 [frame]."""
    return np.hanning(frame + 2)[1:-1]


def _stoi_constants(device):
    if device not in _stoi_tables:
        d = STOI_DEFAULTS
        obm, _ = third_octave_bands(d["fs"], d["n_fft"], d["n_bands"], d["f_min"])
        _stoi_tables[device] = (torch.from_numpy(stoi_window(d["frame"]).astype(np.float32)).to(device),
                                torch.from_numpy(obm.astype(np.float32)).to(device).contiguous())
    return _stoi_tables[device]


def stoi_lengths(lengths, sampling_rate, what="stoi"):
    """The lengths of clips of ``lengths`` samples at ``sampling_rate`` once they are at 10 kHz, or ValueError: a rate
    ``audio.resample`` refuses, or a clip shorter than one frame (256 samples at 10 kHz) after the conversion."""
    from . import audio
    fs, frame = STOI_DEFAULTS["fs"], STOI_DEFAULTS["frame"]
    U, D = audio.check_ratio(sampling_rate, fs, what=what)
    out = [audio.output_length(n, U, D) for n in lengths]
    for b, (n, m) in enumerate(zip(lengths, out)):
        if m < frame:
            raise ValueError(f"{what}: clip {b} has {n} samples at {sampling_rate} Hz, {m} at {fs} Hz: one frame is {frame}")
    return out


def stoi_sums(x, y, lengths=None):
    """The four numbers of ``dws_stoi`` (include/dws.h) for two batches ALREADY at 10 kHz, columns ``STOI_SUMS``: float64
    [B, 4] on the CPU, with Taal's constants (``STOI_DEFAULTS``).  A clip's row depends on its own samples and length
    alone, bit for bit.  Arguments are checked first (ValueError), then the device (RuntimeError)."""
    x, y, host, lens = _pair(x, y, lengths, "stoi_sums")
    stoi_lengths(lens, STOI_DEFAULTS["fs"], "stoi_sums")
    _need_gpu(x, y)
    return _stoi_run(*_f32(x, y), host).cpu()


def _stoi_run(x, y, host):
    """One ``dws_stoi`` call on checked arguments at 10 kHz: float64 [B, 4] on the device."""
    lib = _lib.load()
    d = STOI_DEFAULTS
    B, T = x.shape
    dev = x.device
    window, obm = _stoi_constants(dev)
    out = torch.empty(B, len(STOI_SUMS), device=dev, dtype=torch.float64)
    ws = torch.empty(lib.dws_stoi_workspace(B, T, d["frame"], d["hop"], d["n_bands"]) // 8, device=dev, dtype=torch.float64)
    dev_len, host_len = _length_args(host, dev, B)
    with torch.cuda.device(dev):
        _lib.check(lib.dws_stoi(x.data_ptr(), y.data_ptr(), B, T, _lib.ptr(dev_len), host_len, window.data_ptr(), d["frame"],
                                d["hop"], d["n_fft"], obm.data_ptr(), d["n_bands"], d["segment"], d["beta"], d["dyn_range"],
                                ws.data_ptr(), out.data_ptr(), _lib.current_stream()))
    return out


def stoi(x, y, lengths=None, *, sampling_rate=22050):
    """Short-time objective intelligibility of generated ``x`` against the clean reference ``y`` ([B, T] or [B, 1, T],
    cuda, time-aligned, at ``sampling_rate``), clip by clip.  Returns a dict of float64 [B] CPU tensors: ``stoi`` (Taal et
    al. 2011), ``estoi`` (Jensen & Taal 2016), ``frames_kept`` (the frames left after the silent frames of ``y`` are
    removed) and ``segments`` (``frames_kept - 29`` or 0).

    Both signals are converted to 10 kHz with ``audio.resample`` (not at all where ``sampling_rate`` is 10000), then
    ``dws_stoi`` (include/dws.h) with Taal's constants (``STOI_DEFAULTS``) and the bands of ``third_octave_bands``.  A clip
    that keeps fewer than 30 frames has no segment: its ``stoi`` and ``estoi`` are NaN.  ``lengths`` as in
    ``spectral_metrics``.

    The filter of the rate conversion and the frame count are this project's, not pystoi's or the Matlab original's, and
    the values have not been compared with either.  Arguments are checked before anything runs (ValueError naming the
    ratio or the clip: a rate ``audio.resample`` refuses, a clip shorter than one frame at 10 kHz); CPU tensors raise
    RuntimeError."""
    from . import audio
    x, y, host, lens = _pair(x, y, lengths, "stoi")
    lens10 = stoi_lengths(lens, sampling_rate)
    _need_gpu(x, y)
    x, y = _f32(x, y)
    fs = STOI_DEFAULTS["fs"]
    if sampling_rate != fs:
        x, _ = audio.resample(x, sampling_rate, fs, host)
        y, _ = audio.resample(y, sampling_rate, fs, host)
    s = _stoi_run(x, y, None if host is None else lens10).cpu()
    m = s[:, 2]
    nan = torch.full_like(m, float("nan"))
    return {"stoi": torch.where(m > 0, s[:, 0] / (m * STOI_DEFAULTS["n_bands"]), nan),
            "estoi": torch.where(m > 0, s[:, 1] / m, nan), "frames_kept": s[:, 3].clone(), "segments": m.clone()}


def nanmean(values):
    """The mean of the finite entries of ``values`` (NaN where there is none): a clip whose metric is undefined is left
    out of that metric's mean."""
    v = np.asarray(list(values), dtype=np.float64)
    v = v[np.isfinite(v)]
    return float(v.mean()) if len(v) else float("nan")


def check_resolutions(resolutions, lengths, what="spectral_metrics"):
    """``resolutions`` as a list of checked (n_fft, hop, win) triples (``check_resolution`` on clips of these host
    ``lengths``), or ValueError."""
    try:
        resolutions = [tuple(r) for r in resolutions]
    except TypeError:
        raise ValueError(f"{what}: resolutions = {resolutions!r}: expected (n_fft, hop, win) triples")
    if not resolutions or any(len(r) != 3 for r in resolutions):
        raise ValueError(f"{what}: resolutions = {resolutions!r}: expected (n_fft, hop, win) triples")
    for r in resolutions:
        check_resolution(*r, lengths)
    return resolutions


def check_loss_weights(sc_weight, mag_weight, what="mr_stft_loss"):
    """(sc_weight, mag_weight) as floats: both finite and >= 0, not both 0; or ValueError."""
    out = []
    for name, v in (("sc_weight", sc_weight), ("mag_weight", mag_weight)):
        if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)) or \
                not math.isfinite(float(v)) or float(v) < 0.0:
            raise ValueError(f"{what}: {name} = {v!r} (needs a finite number >= 0)")
        out.append(float(v))
    if out[0] == 0.0 and out[1] == 0.0:
        raise ValueError(f"{what}: sc_weight and mag_weight are both 0: there is nothing to compute")
    return out[0], out[1]


def _loss_value(x, y, host, dev_len, frames, resolutions, sc_weight, mag_weight):
    """The loss per clip (float32 [B], device) and the float64 sums [R][B, 6] behind it.  Divided on the device in double,
    in ``spectral_metrics``' order: nothing goes to the host."""
    sums, total = [], 0.0
    for r, fr in zip(resolutions, frames):
        s = _run(x, y, host, *r, None, None, dev_len=dev_len)
        sums.append(s)
        sc = torch.sqrt(s[:, 0] / s[:, 1])
        mag = s[:, 2] / (fr * (r[0] // 2 + 1))
        total = total + sc_weight * sc + mag_weight * mag
    return (total / len(resolutions)).to(torch.float32), sums


class _MrStftBackward(torch.autograd.Function):
    """``dws_spectral_loss_backward`` over the resolutions as a node of its own, so that differentiating it (a
    second-order request) is an error with a name instead of a silent zero."""

    @staticmethod
    def forward(ctx, g, x, y, dev_len, sums, cfg):
        host, frames, resolutions, sc_weight, mag_weight = cfg
        lib = _lib.load()
        B, T = x.shape
        dev = x.device
        dev_len, host_len = _length_args(host, dev, B, dev_len)
        g = g.to(torch.float64) / len(resolutions)
        dx = torch.empty_like(x)
        sums = sums.unbind(0)
        with torch.cuda.device(dev):
            for n, (r, fr, s) in enumerate(zip(resolutions, frames, sums)):
                n_fft, hop, win = r
                # sc = sqrt(num / den): d sc / d|X| = -(|Y| - |X|) / sqrt(num den); an exact match (num == 0) gets 0, not
                # the NaN of 0 / 0 -- as the mel adjoint does for a zero magnitude
                root = torch.sqrt(s[:, 0] * s[:, 1])
                c_sc = torch.where(s[:, 0] == 0, torch.zeros_like(root), g * sc_weight / root)
                c_mag = g * mag_weight / (fr * (n_fft // 2 + 1))
                coef = torch.stack((c_sc, c_mag), dim=1).contiguous()
                ws = torch.empty(lib.dws_spectral_loss_backward_workspace(B, T, n_fft, hop) // 4, device=dev,
                                 dtype=torch.float32)                                  # the engine allocates nothing
                _lib.check(lib.dws_spectral_loss_backward(x.data_ptr(), y.data_ptr(), B, T, _lib.ptr(dev_len), host_len,
                                                          _window(dev, n_fft, win).data_ptr(), n_fft, hop, coef.data_ptr(),
                                                          dx.data_ptr(), int(n > 0), ws.data_ptr(), _lib.current_stream()))
        return dx

    @staticmethod
    def backward(ctx, *_):
        raise RuntimeError("mr_stft_loss: the second derivative is not built (dws_spectral_loss_backward is a first-order "
                           "adjoint; there is no double backward)")


class _MrStftLoss(torch.autograd.Function):
    """The loss of ``x`` [B, T] (cuda, float32, contiguous) against ``y``: ``dws_spectral_distance`` per resolution
    forwards, ``dws_spectral_loss_backward`` backwards (the first resolution overwrites, the others accumulate)."""

    @staticmethod
    def forward(ctx, x, y, dev_len, cfg):
        host, frames, resolutions, sc_weight, mag_weight = cfg
        value, sums = _loss_value(x, y, host, dev_len, frames, resolutions, sc_weight, mag_weight)
        ctx.save_for_backward(x, y, dev_len, torch.stack(sums))
        ctx.cfg = cfg
        return value

    @staticmethod
    def backward(ctx, g):
        x, y, dev_len, sums = ctx.saved_tensors
        return _MrStftBackward.apply(g, x, y, dev_len, sums, ctx.cfg), None, None, None


def mr_stft_loss(x, y, lengths=None, *, resolutions=MR_STFT_RESOLUTIONS, sc_weight=1.0, mag_weight=1.0):
    """Parallel WaveGAN's multi-resolution STFT loss of generated ``x`` against reference ``y`` ([B, T] or [B, 1, T],
    cuda), per clip: the mean over ``resolutions`` of ``sc_weight * sc + mag_weight * mag`` with ``sc`` / ``mag`` as in
    ``spectral_metrics`` (whose ``mr_stft`` this is at weights 1).  float32 [B] on x's device, differentiable in ``x``:
    the adjoint is ``dws_spectral_loss_backward`` (include/dws.h), first order only.  ``lengths`` as in
    ``spectral_metrics``: the gradient behind a clip's length is exactly 0, and nothing there is read.

    Zero-gradient conventions (torch autograd gives NaN in the first case): a clip whose spectral-convergence numerator
    is exactly 0 (``x`` equal to ``y``) gets no gradient from that term; a bin of X below the magnitude floor passes none.

    ``y.requires_grad`` is a ValueError (the gradient with respect to the reference is not built), as are weights that are
    negative, not finite or both 0.  Arguments are checked first (ValueError), then the device (RuntimeError).  Where
    ``x`` does not require grad this is the plain forward."""
    x, y, host, lens = _pair(x, y, lengths)
    resolutions = check_resolutions(resolutions, lens, "mr_stft_loss")
    sc_weight, mag_weight = check_loss_weights(sc_weight, mag_weight)
    if y.requires_grad:
        raise ValueError("mr_stft_loss: y requires grad, and the gradient with respect to the reference is not built "
                         "(pass y.detach())")
    _need_gpu(x, y)
    (y,) = _f32(y)
    dev = x.device
    dev_len, _ = _length_args(host, dev, len(lens))
    if host is None:
        frames = [float(lens[0] // r[1] + 1) for r in resolutions]
    else:
        frames = [torch.tensor([n // r[1] + 1 for n in lens], dtype=torch.float64).to(dev) for r in resolutions]
    cfg = (host, frames, resolutions, sc_weight, mag_weight)
    if x.requires_grad and torch.is_grad_enabled():
        return _MrStftLoss.apply(x.to(torch.float32).contiguous(), y, dev_len, cfg)
    return _loss_value(*_f32(x), y, host, dev_len, frames, resolutions, sc_weight, mag_weight)[0]

"""Training-step pieces around the network (``train.py:198-222``): q-sample and the epsilon loss.  ``net`` is
any differentiable module of the reference surface; with the engine modules the call goes through
``models.engine._EngineTrainFn`` (``dws_model_forward_train`` / ``dws_model_backward``), which keeps the
activations of exactly one forward per module -- pair every forward with its backward."""
import math

import torch


class _PinnedStager:
    """Host-to-device copies that do not block the host: the CPU tensor goes through a page-locked staging buffer
    (one per call site) and an asynchronous copy; an event guards the buffer's reuse.  A pageable ``.to(device)``
    makes the host wait until the GPU has drained everything queued before it -- once per training step that
    serialises the step's Python overhead (state-dict walk, ~2000 launches' worth of enqueueing) with the GPU."""

    def __init__(self):
        self._slots = {}

    def __call__(self, t, device, slot):
        device = torch.device(device)
        if device.type != "cuda" or t.device.type != "cpu":
            return t.to(device)
        ent = self._slots.get(slot)
        if ent is None or ent[0].shape != t.shape or ent[0].dtype != t.dtype:
            ent = [torch.empty(t.shape, dtype=t.dtype).pin_memory(), None]
            self._slots[slot] = ent
        if ent[1] is not None:
            ent[1].synchronize()          # the previous copy out of this buffer has run (a step ago)
        ent[0].copy_(t)
        out = ent[0].to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        ent[1] = ev
        return out


_stage = _PinnedStager()
_alpha_bar_on = {}   # (id of the CPU tensor, device) -> device copy of Alpha_bar


def _alpha_bar(Alpha_bar, device):
    device = torch.device(device)
    if Alpha_bar.device == device:
        return Alpha_bar
    key = (id(Alpha_bar), Alpha_bar._version, str(device))
    hit = _alpha_bar_on.get(key)
    if hit is None:
        _alpha_bar_on.clear()
        hit = _alpha_bar_on[key] = (Alpha_bar, Alpha_bar.to(device))   # keeps the CPU tensor alive: the id stays unique
    return hit[1]


def q_sample(audio, diffusion_steps, Alpha_bar, z, prior_std=None):
    """x_t ~ q(x_t | x_0): ``sqrt(abar_t) x_0 + sqrt(1 - abar_t) z`` (``train.py:220``).  ``prior_std`` (adaptive prior,
    [B, 1, L] or [B, C, L]): ``z`` stays standard normal and the process ends in N(0, diag(prior_std^2)):
    ``sqrt(abar_t) x_0 + sqrt(1 - abar_t) (prior_std * z)``."""
    ab = _alpha_bar(Alpha_bar, audio.device)[diffusion_steps]
    if prior_std is not None:
        z = prior_std * z
    return torch.sqrt(ab) * audio + torch.sqrt(1 - ab) * z


def _check_prior_std(prior_std, audio):
    B, C, L = audio.shape
    if not isinstance(prior_std, torch.Tensor) or tuple(prior_std.shape) not in ((B, 1, L), (B, C, L)) \
            or not prior_std.dtype.is_floating_point:
        raise ValueError(f"training_loss: prior_std must be a float tensor [{B}, 1, {L}] or [{B}, {C}, {L}] (got "
                         f"{tuple(getattr(prior_std, 'shape', ()))!r})")
    if prior_std.device.type == "cpu" and not bool((torch.isfinite(prior_std) & (prior_std > 0)).all()):
        raise ValueError("training_loss: prior_std must be finite and > 0 at every position")
    return prior_std.detach().to(device=audio.device, dtype=torch.float32)


def stft_loss_options(stft_weight=None, stft_max_step=None, stft_resolutions=None, T=None, where="training_loss"):
    """The spectral-loss arguments, checked: ``stft_weight`` a finite number > 0, ``stft_max_step`` an integer >= 0 (at
    most ``T`` where that is given; default: every step), ``stft_resolutions`` (n_fft, hop, win) triples the kernel
    builds (default: Parallel WaveGAN's three).  Returns None without ``stft_weight`` (the other two then need it), else
    a dict of the three values."""
    from .metrics import MR_STFT_RESOLUTIONS, check_resolutions
    if stft_weight is None:
        if stft_max_step is not None or stft_resolutions is not None:
            raise ValueError(f"{where}: stft_max_step / stft_resolutions need stft_weight")
        return None
    if isinstance(stft_weight, (bool, str)) or not isinstance(stft_weight, (int, float)) or \
            not math.isfinite(float(stft_weight)) or not float(stft_weight) > 0.0:
        raise ValueError(f"{where}: stft_weight = {stft_weight!r} (needs a finite number > 0)")
    if stft_max_step is not None:
        if isinstance(stft_max_step, bool) or not isinstance(stft_max_step, int) or stft_max_step < 0 or \
                (T is not None and stft_max_step > T):
            raise ValueError(f"{where}: stft_max_step = {stft_max_step!r} (needs an integer in 0 .. T"
                             + (f" = {T})" if T is not None else ")"))
    resolutions = MR_STFT_RESOLUTIONS if stft_resolutions is None else stft_resolutions
    resolutions = check_resolutions(resolutions, (), where)      # (the clips' lengths: mr_stft_loss, or the caller)
    return dict(weight=float(stft_weight), max_step=stft_max_step, resolutions=[list(r) for r in resolutions])


def training_loss(net, loss_fn, audio, diffusion_hyperparams, mel_spec=None, generator=None, labels=None,
                  label_dropout=0.0, prior_std=None, stft_weight=None, stft_max_step=None, stft_resolutions=None,
                  parts=None, pqmf=None, prior_filter=None, prior_stft=None):
    """``train.py:198-222``: ``t ~ U{0..T-1}``, ``z ~ N(0, I)``, ``loss_fn(net((x_t, t), mel), z)``.
    Steps and noise are drawn on the CPU generator exactly like the reference (then moved, through pinned staging
    buffers so the host does not stall), so a seeded call consumes the RNG stream in the same order.

    ``labels`` (class-conditional models; not in the reference): integer tensor [B], handed to ``net(..., labels=)``.
    ``label_dropout = p > 0`` trains the null class for classifier-free guidance: the clips where
    ``torch.rand(B, generator=generator) < p`` get the null class ``net.n_classes``.  The mask is drawn after the draws
    above and only when ``labels is not None and p > 0``: an unlabelled seeded run consumes the RNG as before.

    ``prior_std`` (adaptive prior, PriorGrad: Lee et al., ICLR 2022; not in the reference): float tensor [B, 1, L] or
    [B, C, L], finite and > 0 (``mel.prior_std_from_mel`` of the batch's own mel; the values of a CPU tensor are checked,
    those of a device tensor are not -- that would make the host wait for the GPU once per step -- and a zero or NaN there
    shows as an inf / NaN loss).  ``z`` is drawn exactly as without it;
    the forward process noises with ``eps = prior_std * z`` and the loss is the paper's Sigma^-1-weighted norm with mean
    reduction, ``mean(((eps_theta - eps) / prior_std)^2)``.  ``loss_fn`` is ignored then.  Without ``prior_std`` not one
    operation changes.

    ``stft_weight`` = lambda > 0 (spectral loss on the denoised estimate, as InferGrad, WaveFit and FastDiff train with;
    not in the reference; one channel only) adds Parallel WaveGAN's multi-resolution STFT loss of the estimate

        x0_hat = (x_t - sqrt(1 - abar_t) eps_theta) / sqrt(abar_t)           (eps = prior_std * z under a prior)
        aux    = (1 / B) sum_b [t_b < stft_max_step] mr_stft_loss(x0_hat, audio)_b
        loss   = base + lambda * aux

    against the clean audio (``metrics.mr_stft_loss``: ``dws_spectral_distance`` forwards, ``dws_spectral_loss_backward``
    backwards; no gradient goes to ``audio`` through the reference side).  ``stft_max_step`` (default T: every step) keeps
    the term to the low-noise steps, where the estimate resembles audio; the mask is a product on the device and the
    divisor is B, not the number of clips that pass, so nothing waits for the GPU and the scale does not jump from batch
    to batch.  ``stft_resolutions``: (n_fft, hop, win) triples, default ``metrics.MR_STFT_RESOLUTIONS``; a clip too short
    for one is ``check_resolution``'s ValueError, raised before anything is drawn.  ``parts`` (a dict) receives the two
    detached device scalars ``eps`` (the base loss) and ``stft`` (aux).  Without ``stft_weight`` not one operation or
    RNG draw changes.

    ``pqmf`` (multi-band runs; a ``pqmf.PQMF`` of K sub-bands; not in the reference): ``audio`` stays the waveform
    [B, 1, L]; its sub-bands ``pqmf.analysis(audio)`` [B, K, L / K] are what is noised and predicted by a ``net`` of K
    channels, everything else being the call above on the sub-bands -- a seeded call equals the one that is handed
    ``pqmf.analysis(audio)`` as its audio, bit for bit.  With ``stft_weight`` the spectral term stays a full-band one,
    ``mr_stft_loss(pqmf.synthesis(x0_hat), audio)``: its gradient reaches eps_theta through the synthesis bank's adjoint.
    ``prior_std`` with ``pqmf`` is a ValueError (sigma is a full-band quantity; its sub-band form is not built).  Without
    ``pqmf`` not one operation changes.

    ``prior_filter`` (spectral prior, SpecGrad: Koizumi et al., Interspeech 2022; not in the reference): the complex64
    filter F [B, K, L // hop + 1] of ``prior_stft.spectral_filter`` on the batch's own mel, with ``prior_stft`` the
    ``mel.TacotronSTFT`` whose window and hop frame it (L a multiple of the hop; one audio channel).  ``z`` is drawn
    exactly as without it; with T_F = ``mel.tv_filter(., F)`` (``dws_tv_filter``) the forward process noises with
    ``eps = T_F(z)`` -- N(0, Sigma), Sigma = T_F T_F^T -- and the loss is ``mean(T_{1/F}(eps_theta - eps)^2)``, the
    paper's Sigma^-1 norm with its approximation of the inverse of T_F by the filter 1 / F.  Its gradient reaches
    eps_theta through the kernel's adjoint.  ``loss_fn`` is ignored then.  It works with ``labels`` and ``stft_weight``
    (eps = T_F(z) there too); with ``prior_std``, with ``pqmf`` or on more than one channel it is a ValueError.  Without
    ``prior_filter`` not one operation or RNG draw changes."""
    T, Alpha_bar = diffusion_hyperparams["T"], diffusion_hyperparams["Alpha_bar"]
    full = None
    if (prior_filter is None) != (prior_stft is None):
        raise ValueError("training_loss: prior_filter (the filter) and prior_stft (the TacotronSTFT that frames it) come "
                         "together")
    if prior_filter is not None:
        if prior_std is not None:
            raise ValueError("training_loss: prior_filter (spectral prior) and prior_std (energy prior) exclude each other")
        if pqmf is not None:
            raise ValueError("training_loss: pqmf does not combine with prior_filter (the spectral prior is a full-band "
                             "quantity; its sub-band form is not built)")
        if not isinstance(audio, torch.Tensor) or audio.dim() != 3 or audio.shape[1] != 1:
            raise ValueError(f"training_loss: prior_filter needs one audio channel, [B, 1, L] (got "
                             f"{tuple(getattr(audio, 'shape', ()))!r})")
    if pqmf is not None:
        if prior_std is not None:
            raise ValueError("training_loss: pqmf does not combine with prior_std (the adaptive prior is a full-band "
                             "quantity; its sub-band form is not built)")
        if not isinstance(audio, torch.Tensor) or audio.dim() != 3:
            raise ValueError(f"training_loss: with pqmf the audio is the waveform [B, 1, L] (got "
                             f"{tuple(getattr(audio, 'shape', ()))!r})")
        pqmf.check_analysis_input(audio, "training_loss (pqmf)")
        full = audio
    B, C, L = audio.shape
    stft = stft_loss_options(stft_weight, stft_max_step, stft_resolutions, T)
    if stft is not None:
        from .metrics import check_resolutions
        if C != 1:
            raise ValueError(f"training_loss: stft_weight needs one audio channel (audio has {C})")
        check_resolutions(stft["resolutions"], [L] * B, "training_loss")
        if parts is not None and not isinstance(parts, dict):
            raise ValueError("training_loss: parts must be a dict")
    if prior_std is not None:
        prior_std = _check_prior_std(prior_std, audio)
    if pqmf is not None:
        audio = pqmf.analysis(full.detach())        # [B, K, L / K]: what the network sees
    diffusion_steps = _stage(torch.randint(T, size=(B, 1, 1), generator=generator), audio.device, "steps")
    z = _stage(torch.normal(0, 1, size=audio.shape, generator=generator), audio.device, "z")
    if prior_std is not None:
        z = prior_std * z           # eps: the target, and what the forward process adds
    if prior_filter is not None:
        from .mel import tv_filter
        tv = dict(window=prior_stft._tables(audio.device)[0], hop_length=prior_stft.hop_length)
        prior_filter = prior_filter.to(audio.device)
        z = tv_filter(z.view(B, L), prior_filter, **tv).view(B, 1, L)      # eps = T_F(z)
    x_t = q_sample(audio, diffusion_steps, Alpha_bar, z)
    if labels is not None:
        labels = torch.as_tensor(labels).detach().cpu().reshape(-1)     # (host side: the engine takes them from the host)
        if label_dropout > 0:
            drop = torch.rand(B, generator=generator) < label_dropout
            labels = torch.where(drop, torch.full_like(labels, int(net.n_classes)), labels)
        epsilon_theta = net((x_t, diffusion_steps.view(B, 1)), mel_spec=mel_spec, labels=labels)
    else:
        epsilon_theta = net((x_t, diffusion_steps.view(B, 1)), mel_spec=mel_spec)
    if prior_std is not None:
        loss = (((epsilon_theta - z) / prior_std) ** 2).mean()
    elif prior_filter is not None:
        loss = (tv_filter((epsilon_theta - z).reshape(B, L).float(), 1.0 / prior_filter, **tv) ** 2).mean()
    else:
        loss = loss_fn(epsilon_theta, z)
    if stft is None:
        return loss
    from .metrics import mr_stft_loss
    ab = _alpha_bar(Alpha_bar, audio.device)[diffusion_steps]
    x0_hat = (x_t - torch.sqrt(1 - ab) * epsilon_theta) / torch.sqrt(ab)
    if pqmf is not None:
        per_clip = mr_stft_loss(pqmf.synthesis(x0_hat), full.detach(), resolutions=stft["resolutions"])
    else:
        per_clip = mr_stft_loss(x0_hat, audio.detach(), resolutions=stft["resolutions"])
    if stft["max_step"] is not None:
        per_clip = per_clip * (diffusion_steps.view(B) < stft["max_step"]).to(per_clip.dtype)
    aux = per_clip.sum() / B
    if parts is not None:
        parts["eps"], parts["stft"] = loss.detach(), aux.detach()
    return loss + stft["weight"] * aux

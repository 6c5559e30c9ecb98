"""Training-step pieces around the network (``train.py:198-222``): q-sample and the epsilon loss.  ``net`` is
any differentiable module of the reference surface; with the engine modules the call goes through
``models.engine._EngineTrainFn`` (``dws_model_forward_train`` / ``dws_model_backward``), which keeps the
activations of exactly one forward per module -- pair every forward with its backward."""
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


def training_loss(net, loss_fn, audio, diffusion_hyperparams, mel_spec=None, generator=None, labels=None,
                  label_dropout=0.0, prior_std=None):
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
    operation changes."""
    T, Alpha_bar = diffusion_hyperparams["T"], diffusion_hyperparams["Alpha_bar"]
    B, C, L = audio.shape
    if prior_std is not None:
        prior_std = _check_prior_std(prior_std, audio)
    diffusion_steps = _stage(torch.randint(T, size=(B, 1, 1), generator=generator), audio.device, "steps")
    z = _stage(torch.normal(0, 1, size=audio.shape, generator=generator), audio.device, "z")
    if prior_std is not None:
        z = prior_std * z           # eps: the target, and what the forward process adds
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
        return (((epsilon_theta - z) / prior_std) ** 2).mean()
    return loss_fn(epsilon_theta, z)

"""Reverse-diffusion driver with the reference's surface (``generate.py:23-55``,
``utils.py:121-151``) on top of ``dws_sampler_run`` (one step captured as a
hipGraph and replayed T times; schedule, step index and RNG on the device)."""
import contextlib
import ctypes

import numpy as np
import torch

from . import _lib


def calc_diffusion_hyperparams(T, beta_0, beta_T, beta=None, fast=False):
    """``utils.py:121-151``: fp32 tables, sequential in-place recurrences.  All
    tables stay on the host (the engine uploads what it needs once)."""
    if fast and beta is not None:
        Beta = torch.tensor(beta)
        T = len(beta)
    else:
        Beta = torch.linspace(beta_0, beta_T, T)
    Alpha = 1 - Beta
    Alpha_bar = Alpha + 0
    Beta_tilde = Beta + 0
    for t in range(1, T):
        Alpha_bar[t] *= Alpha_bar[t - 1]
        Beta_tilde[t] *= (1 - Alpha_bar[t - 1]) / (1 - Alpha_bar[t])
    Sigma = torch.sqrt(Beta_tilde)
    return {"T": T, "Beta": Beta, "Alpha": Alpha, "Alpha_bar": Alpha_bar, "Sigma": Sigma}


def _host_table(t):
    a = np.ascontiguousarray(t.detach().cpu().to(torch.float32).numpy())
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _check_labels(net, size, labels, cfg_scale, edit=None, resample=None):
    """Argument checks of ``labels=`` / ``cfg_scale=`` before anything runs (ValueError).  Returns the labels as a tuple
    of ints (() = none) and the guidance scale as a float (None = no classifier-free guidance)."""
    if labels is None and cfg_scale is None:
        return (), None         # (an unlabelled call: the network is not looked at here)
    B = int(size[0])
    n_classes = int(getattr(net, "n_classes", 0) or 0)
    if labels is not None and not n_classes:
        raise ValueError("sampler: labels= on a model without classes (set model.n_classes)")
    key = net._label_list(labels, B) if labels is not None else ()
    if cfg_scale is None:
        return key, None
    try:
        scale = float(cfg_scale)
    except (TypeError, ValueError):
        raise ValueError(f"sampler: cfg_scale = {cfg_scale!r} (needs a number)")
    if not np.isfinite(scale):
        raise ValueError(f"sampler: cfg_scale = {cfg_scale!r} (needs a finite number)")
    if labels is None:
        raise ValueError("sampler: cfg_scale= needs labels= (classifier-free guidance steers towards a class)")
    if resample is not None:
        raise ValueError("sampler: cfg_scale= is not built for resampling runs (resample=)")
    if edit is not None and any(v is not None for v in edit.values()):
        raise ValueError("sampler: cfg_scale= is not built for editing runs (known / mask / x_start ...)")
    return key, scale


_MASK64 = (1 << 64) - 1
_GOLDEN64 = 0x9E3779B97F4A7C15


def _check_lengths(net, size, lengths, cfg_scale):
    """Argument checks of ``lengths=`` before anything runs (ValueError).  Returns the lengths as a tuple of ints, or
    None.  The values themselves (1 .. L, one per clip) are checked by the engine."""
    if lengths is None:
        return None
    if cfg_scale is not None:
        raise ValueError("sampler: lengths= (ragged batches) is not built for classifier-free guidance (cfg_scale=)")
    if not hasattr(net, "_set_lengths"):
        raise ValueError("sampler: lengths= needs an engine model")
    key = net._lengths_checked(lengths)      # (SaShiMi: a multiple of the pooling factors' product, NotImplementedError)
    if len(key) != size[0]:
        raise ValueError(f"sampler: lengths holds {len(key)} entries for a batch of {size[0]}")
    return key


def _check_prior(size, prior_std, cfg_scale=None, lengths=None):
    """Argument checks of ``prior_std=`` before anything runs (ValueError).  Returns the table as a detached float32
    tensor expanded to ``size`` (on the device it came on), or None.  With ``lengths`` only the positions of each clip
    below its own length are looked at; the padding of the returned table holds 1."""
    if prior_std is None:
        return None
    if cfg_scale is not None:
        raise ValueError("sampler: prior_std= (adaptive prior) is not built for classifier-free guidance (cfg_scale=)")
    B, C, L = (int(v) for v in size)
    if not isinstance(prior_std, torch.Tensor):
        prior_std = torch.as_tensor(np.asarray(prior_std, dtype=np.float32))
    t = prior_std.detach()
    if tuple(t.shape) not in ((B, 1, L), (B, C, L)) or not t.dtype.is_floating_point:
        raise ValueError(f"sampler: prior_std of shape {tuple(t.shape)} and dtype {t.dtype} (needs a float tensor "
                         f"[{B}, 1, {L}] or [{B}, {C}, {L}])")
    t = t.to(torch.float32).expand(B, C, L)
    if lengths is not None:
        valid = torch.arange(L, device=t.device)[None, None, :] < torch.as_tensor(list(lengths), device=t.device)[:, None, None]
        t = torch.where(valid, t, torch.ones_like(t))
    if not bool((torch.isfinite(t) & (t > 0)).all()):
        raise ValueError("sampler: prior_std must be finite and > 0 at every position (a standard deviation; "
                         "prior_std_from_mel clamps at std_min)")
    return t.contiguous()


def _set_prior(net, sigma):
    """Install (a cuda float32 tensor [B, C, L]) or drop (None) the engine's prior table on the current stream."""
    lib = _lib.load()
    if sigma is None:
        _lib.check(lib.dws_sampler_set_prior(net._handle, None, 0, 0, _lib.current_stream()))
    else:
        _lib.check(lib.dws_sampler_set_prior(net._handle, sigma.data_ptr(), sigma.shape[0], sigma.shape[1] * sigma.shape[2],
                                             _lib.current_stream()))


SPECTRAL_NOISE_LIMIT = 4 << 30      # bytes of injected noise a spectral-prior run may hold: the cap of the CFG step table


def philox_normal(size, seed, stream_id, device="cuda"):
    """The standard-normal numbers a seeded run draws, as a float32 tensor of shape ``size = (B, C, L)`` on ``device``:
    Philox stream ``stream_id`` of the scalar ``seed`` over the whole batch (``dws_philox_normal``), or, with a list of B
    seeds, of every clip's own seed over its C L elements (``dws_philox_normal_clips``).  Stream ids as include/dws.h
    numbers them: s for the update noise of step s, S for x_T."""
    B, C, L = (int(v) for v in size)
    z = torch.empty(B, C, L, device=device, dtype=torch.float32)
    with torch.cuda.device(z.device):
        if isinstance(seed, (list, tuple)):
            _lib.check(_lib.load().dws_philox_normal_clips(z.data_ptr(), B, C * L, (ctypes.c_uint64 * B)(*seed), stream_id,
                                                           _lib.current_stream()))
        else:
            _lib.check(_lib.load().dws_philox_normal(z.data_ptr(), z.numel(), seed, stream_id, _lib.current_stream()))
    return z


def _spectral_prior_run(who, size, S, noisy, prior_filter, prior_stft, x_T, noise, seed, lengths, refused):
    """The spectral prior (``prior_filter=`` / ``prior_stft=``) of a sampler: checks (ValueError), then the run's
    standard-normal numbers -- drawn here from the documented Philox streams, or injected -- through
    ``mel.tv_filter(., prior_filter)``.  Returns ``(x_T, noise, seed)`` to hand to the plain run: ``x_T`` [B, 1, L] (an
    injected one is a state and is returned as given), ``noise`` [S, B, 1, L] (None where ``noisy`` is false: the run
    consumes no update noise; row 0 is never read and holds 0) and the seed that was drawn where none was given."""
    from .mel import tv_filter
    if prior_stft is None or prior_filter is None:
        raise ValueError(f"{who}: prior_filter (the filter) and prior_stft (the TacotronSTFT that frames it) come together")
    for name, v in refused.items():
        if v is not None:
            raise ValueError(f"{who}: prior_filter= (spectral prior) is not built together with {name}= (its noise sites "
                             "are not shaped)")
    B, C, L = (int(v) for v in size)
    if C != 1:
        raise ValueError(f"{who}: prior_filter= needs one audio channel (size = {tuple(size)})")
    if noisy and S * B * L * 4 > SPECTRAL_NOISE_LIMIT:
        raise ValueError(f"{who}: prior_filter= holds the shaped update noise of the whole run, [{S}, {B}, 1, {L}] float32 = "
                         f"{S * B * L * 4 / 1e9:.2f} GB (limit {SPECTRAL_NOISE_LIMIT / 1e9:.2f} GB): sample fewer steps or "
                         "clips at a time")
    if not isinstance(prior_filter, torch.Tensor) or prior_filter.device.type != "cuda":
        raise ValueError(f"{who}: prior_filter must be a cuda tensor [B, K, L // hop + 1] (TacotronSTFT.spectral_filter)")
    dev = prior_filter.device
    tv = dict(window=prior_stft._tables(dev)[0], hop_length=prior_stft.hop_length,
              lengths=None if lengths is None else list(lengths))
    seeds = seed_list(seed, B)
    if seeds is None and seed is None:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    draw = seeds if seeds is not None else int(seed)
    with torch.no_grad():
        if x_T is None:
            x_T = tv_filter(philox_normal(size, draw, S, dev).view(B, L), prior_filter, **tv).view(B, 1, L)
        if not noisy:
            return x_T, None, seed
        if noise is not None and tuple(noise.shape) != (S, B, C, L):
            raise ValueError(f"{who}: noise has shape {tuple(noise.shape)}, expected {(S, B, C, L)}")
        shaped = torch.zeros(S, B, 1, L, device=dev, dtype=torch.float32)
        for s in range(1, S):       # a chunk of B clips per call; noise[0] is not read by any sampler
            z = philox_normal(size, draw, s, dev) if noise is None else noise[s].detach().to(device=dev, dtype=torch.float32)
            shaped[s] = tv_filter(z.reshape(B, L).contiguous(), prior_filter, **tv).view(B, 1, L)
    return x_T, shaped, seed


def spectral_prior_noise(size, steps, prior_filter, prior_stft, *, seed=None, lengths=None, x_T=None, noise=None,
                         update_noise=True):
    """What a sampler with ``prior_filter=`` hands to the plain run, as a call of its own: ``(x_T, noise, seed)`` with
    ``x_T = T_F(z_S)`` [B, 1, L], ``noise[s] = T_F(z_s)`` [steps, B, 1, L] (None with ``update_noise=False``: DDIM at
    eta = 0, DPM-Solver++) and the seed that was drawn where none was given -- the shaped noise of a run of ``steps``
    steps at ``size = (B, 1, L)``, for holding it across runs or timing it."""
    return _spectral_prior_run("spectral_prior_noise", size, int(steps), bool(update_noise), prior_filter, prior_stft, x_T,
                               noise, seed, lengths, {})


def _splitmix64(z):
    """The splitmix64 finaliser (Steele, Lea & Flood, 2014) of a 64-bit integer, in host integer arithmetic."""
    z = (z + _GOLDEN64) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def clip_seeds(seed, first, count):
    """Per-clip seeds of a run: a list of ``count`` ints in 0 .. 2^64-1; entry j, for the global clip ``k = first + j``,
    is ``splitmix64((seed + 0x9E3779B97F4A7C15 (k + 1)) mod 2^64)``.  A clip's seed depends on the run's seed and the
    clip's global number alone, and runs with neighbouring seeds do not share clip streams (``seed + 1000 r + i`` would).
    Pass the list as ``seed=`` to any sampler of this module."""
    if not _is_int(seed) or not _is_int(first) or not _is_int(count) or int(first) < 0 or int(count) < 0:
        raise ValueError(f"clip_seeds: seed = {seed!r}, first = {first!r}, count = {count!r} (needs integers, "
                         "first >= 0, count >= 0)")
    seed, first = int(seed), int(first)
    return [_splitmix64((seed + _GOLDEN64 * (first + j + 1)) & _MASK64) for j in range(int(count))]


def seed_list(seed, B):
    """The per-clip form of ``seed=``, checked on the host (ValueError): None for None or an int (the scalar seed of the
    whole batch), otherwise a list of ``B`` ints in 0 .. 2^64-1 from a sequence or a 1-D integer tensor / array."""
    if seed is None or isinstance(seed, (int, np.integer)) and not isinstance(seed, bool):
        return None
    if isinstance(seed, (torch.Tensor, np.ndarray)):
        if seed.ndim != 1 or (seed.dtype.is_floating_point if isinstance(seed, torch.Tensor) else seed.dtype.kind not in "iu"):
            raise ValueError(f"sampler: seed= of shape {tuple(seed.shape)} and dtype {seed.dtype} (a per-clip seed table "
                             "is a 1-D integer tensor)")
        seed = seed.tolist()
    try:
        vals = list(seed)
    except TypeError:
        raise ValueError(f"sampler: seed = {seed!r} (needs an int, or a sequence of one int per clip)")
    if len(vals) != int(B):
        raise ValueError(f"sampler: {len(vals)} clip seeds for a batch of {int(B)} clips")
    for b, v in enumerate(vals):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= _MASK64:
            raise ValueError(f"sampler: clip seed {b} = {v!r} (needs an integer in 0 .. 2^64-1)")
    return [int(v) for v in vals]


def _set_clip_seeds(net, seeds):
    """Install (a list) or drop (None) the engine's per-clip seed table on the current stream."""
    lib = _lib.load()
    if seeds is None:
        _lib.check(lib.dws_sampler_set_clip_seeds(net._handle, None, 0, _lib.current_stream()))
    else:
        table = (ctypes.c_uint64 * len(seeds))(*seeds)
        _lib.check(lib.dws_sampler_set_clip_seeds(net._handle, table, len(seeds), _lib.current_stream()))


def _prepare_run(net, size, steps, condition, x_T, noise, seed, labels=(), cfg=False, lengths=None):
    """Shared set-up of the sampler entry points: the engine's parameters / shape / condition / labels, the state tensor
    x (x_T, or to be drawn on the device: init = 1), the injected noise [steps, B, C, L] and the seed.  ``cfg``: the
    engine is prepared for 2 B clips -- the labels in the first half, the null class in the second -- while x and the
    noise keep the caller's B."""
    B, C, L = size
    dev = torch.device("cuda")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    net._train_generation += 1     # the sampler's forwards overwrite the activations of a pending training forward
    net._sync_params(L)
    nB = 2 * B if cfg else B
    net._prepare(nB, L)
    if cfg:
        labels = tuple(labels) + (net.n_classes,) * B
        if condition is not None and condition.dim() == 3 and condition.shape[0] == B and B > 1:
            condition = torch.cat([condition, condition], dim=0)
    net._set_labels(list(labels) if labels else None, nB)
    net._set_lengths(lengths, condition)     # (None: off -- lengths hold for the run they are given to)
    net._set_condition(condition)
    if x_T is None:
        x = torch.empty(size, device=dev, dtype=torch.float32)
        init = 1
    else:
        x = x_T.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
        init = 0
    nz = None
    if noise is not None:
        nz = noise.detach().to(device=dev, dtype=torch.float32).contiguous()
        assert tuple(nz.shape) == (steps, B, C, L)
    return x, init, nz, seed


def edit_coefficients(levels):
    """Tables of the editing modes over the S steps of a run: float32 [4][S] = q1, q2, n1, n2 with ``level[s]`` the
    cumulative alpha_bar of step s (DDPM: the run's ``Alpha_bar``; DDIM: ``Alpha_bar_train[tau]``) and
    ``p_s = level[s-1]`` (``p_0 = 1``) the level the state is at after step s: ``q1 = sqrt(p)``, ``q2 = sqrt(1-p)``,
    ``n1 = sqrt(level)``, ``n2 = sqrt(1-level)``, in float64 from the float32 levels, rounded once (the convention of
    ``ddim_coefficients``, whose k3 row q1 equals)."""
    if isinstance(levels, torch.Tensor):
        levels = levels.detach().cpu().numpy()
    lv = np.asarray(levels, dtype=np.float32).astype(np.float64).reshape(-1)
    if lv.shape[0] < 1:
        raise ValueError("edit_coefficients: no levels")
    p = np.concatenate([[1.0], lv[:-1]])
    return np.stack([np.sqrt(p), np.sqrt(1.0 - p), np.sqrt(lv), np.sqrt(1.0 - lv)]).astype(np.float32)


def spans_to_mask(size, spans):
    """Bool mask ``[1, 1, L]`` (broadcastable to ``size = (B, C, L)``) that is True inside the ``[start, end)`` sample
    spans; overlapping spans unite, no span gives an all-False mask.  A continuation keeps one span ``[0, n)``."""
    L = int(size[-1])
    m = torch.zeros(1, 1, L, dtype=torch.bool)
    for sp in spans:
        if len(sp) != 2 or any(int(v) != v for v in sp) or not 0 <= sp[0] <= sp[1] <= L:
            raise ValueError(f"spans_to_mask: span {list(sp)} is not [start, end) with 0 <= start <= end <= {L}")
        m[..., int(sp[0]):int(sp[1])] = True
    return m


def _is_int(v):
    if isinstance(v, bool):
        return False
    return isinstance(v, (int, np.integer)) or (isinstance(v, (float, np.floating)) and float(v).is_integer())


def _start_position(S, start_step):
    S = int(S)
    if start_step is None:
        return S
    if not _is_int(start_step) or not 0 <= start_step <= S - 1:
        raise ValueError(f"sampler: start_step = {start_step!r} (needs an integer in 0..{S - 1})")
    return int(start_step) + 1


def repaint_program(S, jump, resamples, start_step=None):
    """RePaint's schedule (Lugmayr et al., CVPR 2022) as the ``visit_step`` array of ``dws_sampler_run_program``: int32
    [V] in execution order, ``s >= 0`` a reverse visit at step s, ``-jump`` a jump visit up by ``jump`` positions.

    The state starts at position ``K = S`` (``start_step + 1`` with a partial start); reverse step s takes it from
    position s + 1 to s.  Jump points are the positions ``k = 0, jump, 2 jump, ...`` with ``k + jump <= K - 1``, each with
    a counter ``resamples - 1`` that never refills.  After every reverse visit: if the position reached is a jump point
    whose counter is above zero, the counter goes down by one and the state jumps up to ``k + jump``; the walk ends with
    the reverse visit that reaches position 0 with no jump left there.  ``K + (resamples-1) * jump * #jump points``
    network evaluations (``program_evaluations``).  ``S = 6, jump = 2, resamples = 2`` gives
    ``[5, 4, 3, 2, -2, 3, 2, 1, 0, -2, 1, 0]``; ``resamples = 1`` gives ``K-1 .. 0``."""
    if not _is_int(S) or S < 1:
        raise ValueError(f"repaint_program: S = {S!r} (needs an integer >= 1)")
    K = _start_position(S, start_step)
    if not _is_int(jump) or jump < 1:
        raise ValueError(f"sampler: resample jump = {jump!r} (needs an integer >= 1)")
    if not _is_int(resamples) or resamples < 1:
        raise ValueError(f"sampler: resamples = {resamples!r} (needs an integer >= 1)")
    j, r = int(jump), int(resamples)
    if r > 1 and j > K - 1:
        raise ValueError(f"sampler: resample jump = {j} leaves no jump point below the start position {K} "
                         f"(needs jump <= {K - 1})")
    left = {k: r - 1 for k in range(0, K - j, j)}
    prog, pos = [], K
    while True:
        pos -= 1
        prog.append(pos)
        if left.get(pos, 0) > 0:
            left[pos] -= 1
            prog.append(-j)
            pos += j
        elif pos == 0:
            break
    return np.asarray(prog, dtype=np.int32)


def program_evaluations(S, jump, resamples, start_step=None):
    """Network evaluations of ``repaint_program(S, jump, resamples, start_step)``: K + (r-1) j (number of jump points)."""
    K = _start_position(S, start_step)
    return K + (int(resamples) - 1) * int(jump) * len(range(0, K - int(jump), int(jump)))


def _walk(S, visit_step, start_step=None):
    """(visit number v, position before, position after) of every entry of a program; ValueError when it is no walk."""
    K = _start_position(S, start_step)
    vs = np.asarray(visit_step).reshape(-1)
    V, pos, out = len(vs), K, []
    for i, a in enumerate(int(a) for a in vs):
        new = a if a >= 0 else pos - a
        if (a >= 0 and a != pos - 1) or new > K:
            raise ValueError(f"sampler: program entry {i} = {a} is no move from position {pos} (start position {K})")
        out.append((V - 1 - i, pos, new))
        pos = new
    if V < 1 or pos != 0 or vs[-1] != 0:
        raise ValueError("sampler: a program ends in reverse step 0")
    return out


def jump_coefficients(levels, visit_step, start_step=None):
    """Jump tables of a program over a run with ``levels`` (as ``edit_coefficients``): float32 [2][V] = ja, jb indexed by
    the visit number ``v = V-1-i`` of entry i.  With ``P[0] = 1``, ``P[k] = level[k-1]`` the level of position k, a jump
    from k to k+j has ``ja = sqrt(P[k+j] / P[k])``, ``jb = sqrt(1 - P[k+j] / P[k])`` -- the forward process' marginal
    ``q(x_{k+j} | x_k)`` -- in float64 from the float32 levels, rounded once.  Reverse visits hold zeros."""
    if isinstance(levels, torch.Tensor):
        levels = levels.detach().cpu().numpy()
    lv = np.asarray(levels, dtype=np.float32).astype(np.float64).reshape(-1)
    P = np.concatenate([[1.0], lv])
    walk = _walk(lv.shape[0], visit_step, start_step)
    out = np.zeros((2, len(walk)), dtype=np.float32)
    for v, k, kj in walk:
        if kj > k:
            out[0, v] = np.sqrt(P[kj] / P[k])
            out[1, v] = np.sqrt(1.0 - P[kj] / P[k])
    return out


def program_streams(visit_step):
    """Philox stream ids of a program run: ``visit`` [V] (stream v: the update noise of reverse visit v, z of jump visit
    v), ``known`` [V] (stream V + 1 + v after reverse visit v; -1 for a jump visit, which draws none), ``x_T`` = V (a
    drawn initial state) and ``start`` = 2V + 1 (the q-sample).  With the program ``K-1 .. 0`` of a whole run these are
    ``dws_sampler_run_edit``'s: s, S + 1 + s, S and 2S + 1."""
    vs = np.asarray(visit_step).reshape(-1)
    V = len(vs)
    v = np.arange(V)
    return dict(visit=v, known=np.where(vs[::-1] >= 0, V + 1 + v, -1), x_T=V, start=2 * V + 1)


def _check_resample(size, S, resample, noise, known=None, mask=None, x_start=None, start_step=None, **_):
    """Argument checks of ``resample=(jump, resamples)`` before any GPU work (ValueError).  Returns the program."""
    if known is None or mask is None:
        raise ValueError("sampler: resample= needs known= and mask= (resampling harmonises an inpainting run)")
    try:
        jump, resamples = resample
    except (TypeError, ValueError):
        raise ValueError(f"sampler: resample = {resample!r} (needs (jump, resamples))")
    if x_start is None:
        start_step = None
    elif start_step is None:
        start_step = S - 1
    prog = repaint_program(S, jump, resamples, start_step)
    if noise is not None and tuple(torch.as_tensor(noise).shape) != (len(prog),) + tuple(int(v) for v in size):
        raise ValueError(f"sampler: noise has shape {tuple(noise.shape)}, a program of {len(prog)} visits needs "
                         f"{(len(prog),) + tuple(size)}")
    return prog


def _check_edit(size, S, x_T, known=None, mask=None, known_noise=None, x_start=None, start_step=None,
                start_noise=None, rows=None):
    """Argument checks of the editing modes, all on the host and before any GPU work (ValueError).  Returns
    (known [B,C,L] float32 | None, mask [B,C,L] uint8 | None, known_noise | None, x_start [B,C,L] | None, start_step,
    start_noise tensor | None, q-sample?).  ``rows``: leading dimension of known_noise (default S; V in a program run)."""
    size = tuple(int(v) for v in size)

    def expand(name, t, dtype=None):
        t = torch.as_tensor(t).detach()
        try:
            ok = torch.broadcast_shapes(tuple(t.shape), size) == size
        except RuntimeError:
            ok = False
        if not ok:
            raise ValueError(f"sampler: {name} of shape {tuple(t.shape)} does not broadcast to {size}")
        return t.expand(size)

    def exact(name, t, shape):
        t = torch.as_tensor(t).detach()
        if tuple(t.shape) != shape:
            raise ValueError(f"sampler: {name} has shape {tuple(t.shape)}, expected {shape}")
        return t

    if (known is None) != (mask is None):
        raise ValueError("sampler: known= and mask= come together")
    if known_noise is not None and known is None:
        raise ValueError("sampler: known_noise= without known= / mask=")
    if known is not None:
        known = expand("known", known)
        mask = expand("mask", mask)
        if mask.dtype != torch.bool and not bool(((mask == 0) | (mask == 1)).all()):
            raise ValueError("sampler: mask must be bool or hold only 0 and 1 (soft masks are not built)")
        mask = mask != 0
        if known_noise is not None:
            known_noise = exact("known_noise", known_noise, (S if rows is None else rows,) + size)
    if x_start is None:
        if start_step is not None or start_noise is not None:
            raise ValueError("sampler: start_step= / start_noise= without x_start=")
        return known, mask, known_noise, None, S - 1, None, False
    if x_T is not None:
        raise ValueError("sampler: x_start= and x_T= are two initial states; give one")
    x_start = expand("x_start", x_start)
    start_step = S - 1 if start_step is None else start_step
    if isinstance(start_step, bool) or int(start_step) != start_step or not 0 <= start_step <= S - 1:
        raise ValueError(f"sampler: start_step = {start_step!r} (needs an integer in 0..{S - 1})")
    qsample = start_noise is not False
    if start_noise is None or start_noise is False:
        start_noise = None
    else:
        start_noise = exact("start_noise", start_noise, size)
    return known, mask, known_noise, x_start, int(start_step), start_noise, qsample


def sampling(net, size, diffusion_hyperparams, condition=None, *, x_T=None, noise=None, seed=None,
             use_graph=True, net_steps=None, known=None, mask=None, known_noise=None, x_start=None, start_step=None,
             start_noise=None, resample=None, labels=None, cfg_scale=None, lengths=None, prior_std=None,
             prior_filter=None, prior_stft=None):
    """``x_0 = sampling(net, (B, C, L), dh, condition)`` as in ``generate.py:23-55``.

    Spectral prior (SpecGrad: Koizumi et al., Interspeech 2022; ``dws_tv_filter``), on ``sampling``, ``sampling_aligned``,
    ``sampling_ddim`` and ``sampling_dpmpp``:
      prior_filter, prior_stft  the complex64 filter F [B, K, L // hop + 1] of ``prior_stft.spectral_filter`` on the
             conditioning mel, and that ``mel.TacotronSTFT`` (its window and hop frame the filter; L a multiple of the
             hop, one channel).  The run ends in N(0, Sigma), Sigma = T_F T_F^T with T_F = ``mel.tv_filter(., F)``.
             Nothing in the engine's sampler changes: this wrapper draws the run's standard-normal numbers itself
             (``philox_normal``: stream S for x_T, stream s for the update noise of step s, of the scalar seed or of
             every clip's own), filters them B clips at a time ahead of the loop and hands them over as the injected
             ``x_T`` and ``noise``.  The contract: the run is bit-equal to the plain run (no ``prior_filter``) that is
             handed ``x_T = T_F(z_S)`` and ``noise[s] = T_F(z_s)``.  An injected ``x_T`` is a state and is taken as
             given; an injected ``noise`` stays standard normal and is filtered.  DDIM at eta = 0 and DPM-Solver++
             consume no update noise: only ``x_T`` is shaped.  The shaped noise of the whole run, [S, B, 1, L], is held
             at once: above 4 GB it is a ValueError naming the size.  The network must have been trained for it
             (``training_loss(prior_filter=)``).  Combines with ``seed=[...]``, ``labels`` and ``lengths`` (multiples
             of the hop); refused (ValueError) with ``prior_std``, ``cfg_scale``, the editing / start / resample
             arguments and on ``sampling_guided``, whose noise sites are not shaped.

    Adaptive prior (PriorGrad: Lee et al., ICLR 2022; ``dws_sampler_set_prior``), on every sampler of this module:
      prior_std  float tensor [B, 1, L] or [B, C, L], finite and > 0 (``mel.prior_std_from_mel``): the run ends in
             N(0, diag(prior_std^2)) instead of N(0, I).  Every standard-normal number the run consumes -- drawn from
             Philox or injected (``noise``, ``known_noise``, ``start_noise`` stay standard normal) -- is multiplied by
             ``prior_std`` at its position, one fp32 product of its own, before the unchanged update reads it; an
             injected ``x_T`` is a state and is taken as given.  The network must have been trained for it
             (``training_loss(prior_std=)``).  Combines with ``seed=[...]``, ``lengths``, ``labels``, the editing
             arguments and ``resample``; refused with ``cfg_scale``.  Goes through the schedule entry with
             ``net_steps = 0..T-1``; the table holds for this run and is dropped behind it.

    Class-conditional models (``model.n_classes``; not in the reference), on every sampler of this module:
      labels     integer tensor / list [B] in 0..K (K = the null class); default: the null class for every clip
      cfg_scale  classifier-free guidance (Ho & Salimans, 2021): every step evaluates the network on the labelled and
             on the null-class copy of the state and continues with ``eps_c + cfg_scale * (eps_c - eps_u)`` (0 = the
             conditional run; costs a network of twice the batch).  Needs ``labels``; not built for the editing and
             resampling arguments.  Goes through the schedule entry with ``net_steps = 0..T-1`` (bit-identical to
             ``dws_sampler_run``).

    Ragged batches (both backbones; ``dws_model_set_lengths``), on ``sampling``, ``sampling_aligned``, ``sampling_ddim`` and
    ``sampling_dpmpp``:
      lengths    int sequence / tensor [B] with 1 <= lengths[b] <= L: clip b is that long, the rest of its row is
             padding.  Over ``[0, lengths[b])`` the run is the clip's own run at that length (the network never sees the
             padding: of the state, of ``condition`` behind ``ceil(lengths[b] / hop)`` mel frames, of injected noise);
             the returned ``x`` holds 0.0 in the padding.  Combines with per-clip ``seed=[...]``, ``labels``,
             ``known`` / ``mask``, ``x_start`` / ``start_step`` and ``resample``; refused together with ``cfg_scale`` and
             on ``sampling_guided``.  With a SCALAR seed a clip's noise depends on L (the Philox element index runs over
             the whole padded batch), so a short clip is reproducible across batch compositions only with per-clip
             seeds, whose numbering is the position inside the clip.  A padded position still costs its full time.

    Extra keyword-only arguments (not in the reference):
      x_T    initial state [B,C,L]; default: drawn on the device from the Philox stream
      noise  injected variance noise [T,B,C,L] (``noise[t]`` is added after step t>0) -- parity mode
      seed   Philox seed for the on-device RNG (default: a fresh draw from torch's CPU generator per call, so
             successive unseeded calls differ -- as the reference's do -- and ``torch.manual_seed`` still governs).
             A sequence / 1-D integer tensor of B values in 0 .. 2^64-1 (``clip_seeds``) seeds every clip on its own:
             clip b is then bit-equal to the B = 1 run with ``seed = seed[b]``, whatever the batch around it (with
             ``cfg_scale`` B is the caller's B).  Goes through the schedule entry with ``net_steps = 0..T-1``.
      net_steps  float[T]: the network sees ``net_steps[t]`` at step t instead of t, with the DDPM update of ``dh``
             unchanged (e.g. ``align_steps`` for DiffWave's fast schedule; ``dws_sampler_run_schedule``).  Not the
             reference's loop.
    Editing (``dws_sampler_run_edit``; all off by default, and then this is exactly the path above):
      known, mask  inpainting / continuation by replacement: ``known`` audio and ``mask`` (bool or 0/1, non-zero =
             known), both broadcastable to [B,C,L].  After every step the known region of the state is overwritten
             with ``known`` noised to the level the state is at; the result holds ``known`` exactly where mask is set.
      known_noise  injected noise of that replacement, [T,B,C,L] (parity mode; default Philox)
      x_start, start_step  partial start: run steps ``start_step .. 0`` only (default T-1) from ``x_start``
      start_noise  None: ``x_start`` is clean audio, noised to step ``start_step`` with Philox noise first (q-sample);
             a [B,C,L] tensor: the same with this noise; False: ``x_start`` is the state at ``start_step`` as given.
      Without ``net_steps`` an edited run goes through the schedule entry with ``net_steps = 0..T-1`` (bit-identical
      to ``dws_sampler_run``).
    Resampling (``dws_sampler_run_program``; needs ``known`` / ``mask``):
      resample  ``(jump, resamples)``: RePaint's schedule (``repaint_program``) -- at every ``jump``-th position the
             chain goes back up ``jump`` steps and down again, ``resamples`` times in all, so that the generated part
             is harmonised with the kept part.  ``noise`` and ``known_noise`` are then [V,B,C,L], indexed by the visit.
             ``resamples = 1`` is the edited run above, bit for bit.
    """
    dh = diffusion_hyperparams
    T, Alpha, Alpha_bar, Sigma = dh["T"], dh["Alpha"], dh["Alpha_bar"], dh["Sigma"]
    assert len(Alpha) == T and len(Alpha_bar) == T and len(Sigma) == T and len(size) == 3
    edit = dict(known=known, mask=mask, known_noise=known_noise, x_start=x_start, start_step=start_step,
                start_noise=start_noise)
    if prior_filter is not None or prior_stft is not None:
        S = T if net_steps is None else len(np.asarray(net_steps).reshape(-1))
        x_T, noise, seed = _spectral_prior_run("sampling", size, S, True, prior_filter, prior_stft, x_T, noise, seed, lengths,
                                               dict(edit, resample=resample, cfg_scale=cfg_scale, prior_std=prior_std))
    lengths = _check_lengths(net, size, lengths, cfg_scale)
    if prior_std is not None and cfg_scale is not None:      # (the table itself is checked by _run_schedule, where it goes)
        _check_prior(size, prior_std, cfg_scale)
    lab, scale = _check_labels(net, size, labels, cfg_scale, edit, resample)
    per_clip = seed_list(seed, size[0]) is not None
    if resample is None and all(v is None for v in edit.values()):
        edit = None
        if (scale is not None or per_clip or prior_std is not None) and net_steps is None:
            net_steps = np.arange(T, dtype=np.float32)
    elif net_steps is None:
        net_steps = np.arange(T, dtype=np.float32)
    if net_steps is not None:
        coef = np.stack([_host_table(Alpha)[0], _host_table(Alpha_bar)[0], _host_table(Sigma)[0]])
        return _run_schedule(net, size, _lib.DWS_SAMPLER_DDPM, net_steps, coef, condition, x_T, noise, seed, use_graph,
                             edit=edit, levels=coef[1], resample=resample, labels=labels, cfg_scale=cfg_scale,
                             lengths=lengths, prior_std=prior_std)
    lib = _lib.load()
    with torch.no_grad():
        x, init, nz, seed = _prepare_run(net, size, T, condition, x_T, noise, seed, labels=lab, lengths=lengths)
        a, pa = _host_table(Alpha)
        ab, pab = _host_table(Alpha_bar)
        sg, psg = _host_table(Sigma)
        _lib.check(lib.dws_sampler_run(net._handle, x.data_ptr(), pa, pab, psg, T, _lib.ptr(nz), seed, init,
                                       1 if use_graph else 0, _lib.current_stream()))
        torch.cuda.current_stream().synchronize()  # nz / tables must outlive the enqueued work
    return x


def _run_schedule(net, size, kind, net_steps, coef, condition, x_T, noise, seed, use_graph, edit=None, levels=None,
                  resample=None, labels=None, cfg_scale=None, lengths=None, prior_std=None):
    """``dws_sampler_run_schedule``: S steps s = S-1..0, the network at ``net_steps[s]``, update tables ``coef``.
    ``edit``: the editing arguments of ``sampling`` (-> ``dws_sampler_run_edit``), ``levels`` the run's alpha_bar.
    ``resample``: (jump, resamples) on top of ``edit`` (-> ``dws_sampler_run_program``)."""
    assert len(size) == 3
    lengths = _check_lengths(net, size, lengths, cfg_scale)
    prior = _check_prior(size, prior_std, cfg_scale, lengths)
    lab, scale = _check_labels(net, size, labels, cfg_scale, edit, resample)
    seeds = seed_list(seed, size[0])
    steps = np.ascontiguousarray(np.asarray(net_steps, dtype=np.float32).reshape(-1))
    S = steps.shape[0]
    coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float32))
    if S < 1 or coef.shape != ((3 if kind == _lib.DWS_SAMPLER_DDPM else 5), S):
        raise ValueError(f"sampler: {S} net steps with coefficient tables of shape {coef.shape}")
    prog = None
    if resample is not None:
        prog = _check_resample(size, S, resample, noise, **(edit or {}))
    if edit is not None:
        known, mask, known_noise, x_start, start_step, start_noise, qsample = _check_edit(
            size, S, x_T, rows=None if prog is None else len(prog), **edit)
        if x_start is not None:
            x_T = x_start
    lib = _lib.load()
    fp = ctypes.POINTER(ctypes.c_float)
    with torch.no_grad(), contextlib.ExitStack() as cleanup:
        x, init, nz, seed = _prepare_run(net, size, S if prog is None else len(prog), condition, x_T, noise,
                                         seed if seeds is None else 0, labels=lab, cfg=scale is not None,
                                         lengths=lengths)
        if seeds is not None:     # per-clip seeds hold for this run alone: the engine's table is dropped behind it
            _set_clip_seeds(net, seeds)
            cleanup.callback(_set_clip_seeds, net, None)
        if prior is not None:     # and so does the prior
            prior = prior.to(x.device)
            _set_prior(net, prior)
            cleanup.callback(_set_prior, net, None)
        if edit is None and scale is not None:
            _lib.check(lib.dws_sampler_set_cfg(net._handle, 1, scale))
            try:
                _lib.check(lib.dws_sampler_run_schedule(net._handle, x.data_ptr(), kind, S, steps.ctypes.data_as(fp),
                                                        coef.ctypes.data_as(fp), _lib.ptr(nz), seed, init,
                                                        1 if use_graph else 0, _lib.current_stream()))
            finally:
                _lib.check(lib.dws_sampler_set_cfg(net._handle, 0, 0.0))
        elif edit is None:
            _lib.check(lib.dws_sampler_run_schedule(net._handle, x.data_ptr(), kind, S, steps.ctypes.data_as(fp),
                                                    coef.ctypes.data_as(fp), _lib.ptr(nz), seed, init,
                                                    1 if use_graph else 0, _lib.current_stream()))
        else:
            dev = x.device
            q = np.ascontiguousarray(edit_coefficients(levels))
            on_dev = lambda t, dt: None if t is None else t.to(device=dev, dtype=dt).contiguous()
            known, known_noise, start_noise = (on_dev(t, torch.float32) for t in (known, known_noise, start_noise))
            mask = on_dev(mask, torch.uint8)
            ed = _lib.SamplerEdit(q.ctypes.data_as(fp), _lib.ptr(known), _lib.ptr(mask), _lib.ptr(known_noise),
                                  _lib.ptr(start_noise), start_step,
                                  _lib.DWS_START_QSAMPLE if qsample else _lib.DWS_START_AS_GIVEN)
            if prog is None:
                _lib.check(lib.dws_sampler_run_edit(net._handle, x.data_ptr(), kind, S, steps.ctypes.data_as(fp),
                                                    coef.ctypes.data_as(fp), _lib.ptr(nz), seed, init,
                                                    1 if use_graph else 0, ctypes.byref(ed), _lib.current_stream()))
            else:
                prog = np.ascontiguousarray(prog, dtype=np.int32)
                jc = np.ascontiguousarray(jump_coefficients(levels, prog, start_step))
                _lib.check(lib.dws_sampler_run_program(
                    net._handle, x.data_ptr(), kind, S, steps.ctypes.data_as(fp), coef.ctypes.data_as(fp), len(prog),
                    prog.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), jc.ctypes.data_as(fp), _lib.ptr(nz), seed, init,
                    1 if use_graph else 0, ctypes.byref(ed), _lib.current_stream()))
        torch.cuda.current_stream().synchronize()  # nz (and the editing tensors) must outlive the enqueued work
    return x


# --------------------------------------------------------------------------- few-step schedules (not the reference's)
def align_steps(T, beta_0, beta_T, infer_betas):
    """DiffWave's step alignment (Kong et al., ICLR 2021, App. B): the fractional training step whose noise level
    matches each step of a short inference schedule ``infer_betas``.  float64 throughout: training
    ``abar_t = prod_{i<=t} (1 - beta_i)`` over ``linspace(beta_0, beta_T, T)``, inference
    ``gamma_s = prod_{i<=s} (1 - beta'_i)``; for the first t in 0..T-2 with ``abar_{t+1} <= gamma_s <= abar_t``,
    ``t_s = t + (sqrt(abar_t) - sqrt(gamma_s)) / (sqrt(abar_t) - sqrt(abar_{t+1}))``, rounded to float32 once.
    A gamma_s outside ``[abar_{T-1}, abar_0]`` by a relative 1e-9 at most is clamped to that end; further out ->
    ValueError.  ``infer_betas = linspace(beta_0, beta_T, T)`` gives exactly 0, 1, ..., T-1."""
    T = int(T)
    if T < 1:
        raise ValueError(f"align_steps: T = {T}")
    abar = np.cumprod(1.0 - np.linspace(beta_0, beta_T, T, dtype=np.float64))
    gamma = np.cumprod(1.0 - np.asarray(infer_betas, dtype=np.float64).reshape(-1))
    sab = np.sqrt(abar)
    lo, hi = abar[-1], abar[0]
    out = np.empty(gamma.shape[0], dtype=np.float64)
    for s, g in enumerate(gamma):
        if g > hi or g < lo:
            end = hi if g > hi else lo
            if not abs(g - end) <= 1e-9 * end:
                raise ValueError(f"align_steps: gamma_{s} = {g!r} is outside the training range "
                                 f"[abar_{T - 1}, abar_0] = [{lo!r}, {hi!r}]")
            g = end
        if T == 1:
            out[s] = 0.0
            continue
        t = int(np.flatnonzero((abar[1:] <= g) & (g <= abar[:-1]))[0])
        out[s] = t + (sab[t] - np.sqrt(g)) / (sab[t] - sab[t + 1])
    return out.astype(np.float32)


def ddim_steps(T, S):
    """DDIM's sub-sequence of the T training steps: ``tau_i = rint(i (T-1) / (S-1))``, i = 0..S-1 (``[T-1]`` for
    S = 1).  ``S`` may also be an explicit increasing list of steps in 0..T-1."""
    T = int(T)
    if isinstance(S, (list, tuple, np.ndarray)):
        tau = [int(t) for t in S]
        if len(tau) < 1 or any(float(a) != b for a, b in zip(tau, S)):
            raise ValueError(f"ddim_steps: steps must be a non-empty list of integers, got {list(S)}")
        if tau[0] < 0 or tau[-1] > T - 1 or any(b <= a for a, b in zip(tau, tau[1:])):
            raise ValueError(f"ddim_steps: steps must increase strictly within 0..{T - 1}, got {tau}")
        return tau
    S = int(S)
    if S < 1 or S > T:
        raise ValueError(f"ddim_steps: S = {S} steps out of T = {T} (needs 1 <= S <= T)")
    if S == 1:
        return [T - 1]
    tau = [int(np.rint(i * (T - 1) / (S - 1))) for i in range(S)]
    assert all(b > a for a, b in zip(tau, tau[1:]))
    return tau


def ddim_coefficients(alpha_bar, tau, eta):
    """Update tables of DDIM (Song et al., ICLR 2021) over the steps ``tau``: float32 [5][S] = k1..k5 with
    ``a_s = abar[tau_s]``, ``p_s = abar[tau_{s-1}]`` (``p_0 = 1``), ``sigma_s = eta sqrt((1-p_s)/(1-a_s))
    sqrt(1 - a_s/p_s)``; ``k1 = sqrt(1-a)``, ``k2 = sqrt(a)``, ``k3 = sqrt(p)``, ``k4 = sqrt(max(0, 1-p-sigma^2))``,
    ``k5 = sigma``, in float64 from the float32 ``Alpha_bar`` of ``calc_diffusion_hyperparams``, rounded once.  The
    engine's step is then ``u = (x - k1 eps) / k2; x = k3 u + k4 eps (+ k5 z for s > 0)``."""
    if isinstance(alpha_bar, torch.Tensor):
        alpha_bar = alpha_bar.detach().cpu().numpy()
    ab = np.asarray(alpha_bar, dtype=np.float32).astype(np.float64)
    tau = np.asarray(tau, dtype=np.int64).reshape(-1)
    a = ab[tau]
    p = np.concatenate([[1.0], ab[tau[:-1]]])
    sigma = float(eta) * np.sqrt((1.0 - p) / (1.0 - a)) * np.sqrt(1.0 - a / p)
    k = np.stack([np.sqrt(1.0 - a), np.sqrt(a), np.sqrt(p), np.sqrt(np.maximum(0.0, 1.0 - p - sigma * sigma)), sigma])
    return k.astype(np.float32)


def sampling_ddim(net, size, dh_train, steps, eta=0.0, condition=None, *, x_T=None, noise=None, seed=None,
                  use_graph=True, known=None, mask=None, known_noise=None, x_start=None, start_step=None,
                  start_noise=None, resample=None, labels=None, cfg_scale=None, lengths=None, prior_std=None,
                  prior_filter=None, prior_stft=None):
    """DDIM over ``ddim_steps(T, steps)`` of the training schedule ``dh_train`` (``steps``: S or an explicit list),
    deterministic for ``eta = 0``.  ``noise``: injected z, [S, B, C, L] (``noise[s]`` is used after step s > 0).
    The editing arguments, ``resample``, ``labels``, ``cfg_scale`` and ``prior_std`` are those of ``sampling`` (levels:
    ``Alpha_bar[tau]``); ``prior_filter`` / ``prior_stft`` (spectral prior) as there too: at ``eta = 0`` only ``x_T``
    is shaped.  Not the reference's loop."""
    tau = ddim_steps(dh_train["T"], steps)
    coef = ddim_coefficients(dh_train["Alpha_bar"], tau, eta)
    edit = dict(known=known, mask=mask, known_noise=known_noise, x_start=x_start, start_step=start_step,
                start_noise=start_noise)
    if prior_filter is not None or prior_stft is not None:
        x_T, noise, seed = _spectral_prior_run("sampling_ddim", size, len(tau), float(eta) != 0.0, prior_filter, prior_stft,
                                               x_T, noise, seed, lengths,
                                               dict(edit, resample=resample, cfg_scale=cfg_scale, prior_std=prior_std))
    if resample is None and all(v is None for v in edit.values()):
        edit = None
    return _run_schedule(net, size, _lib.DWS_SAMPLER_DDIM, np.asarray(tau, dtype=np.float32), coef, condition, x_T,
                         noise, seed, use_graph, edit=edit, levels=_host_table(dh_train["Alpha_bar"])[0][tau],
                         resample=resample, labels=labels, cfg_scale=cfg_scale, lengths=lengths, prior_std=prior_std)


def logsnr_steps(alpha_bar, S):
    """Sub-sequence of the T training steps spaced uniformly in log-SNR, the spacing a multistep solver needs (uniform
    in t, ``ddim_steps``, leaves a huge log-SNR gap to the last steps): with ``lam_t = 0.5 log(abar_t / (1 - abar_t))`` in
    float64 from the float32 ``Alpha_bar``, the sorted, de-duplicated ``argmin_t |lam_t - target|`` over the targets
    ``linspace(lam_0, lam_{T-1}, S)``.  Contains 0 and T-1 for S >= 2 and may be shorter than S where targets collide:
    its length is the number of network evaluations.  ``[T-1]`` for S = 1.  ``S`` may also be an explicit increasing
    list of steps in 0..T-1 (checked as ``ddim_steps`` checks it)."""
    if isinstance(alpha_bar, torch.Tensor):
        alpha_bar = alpha_bar.detach().cpu().numpy()
    ab = np.asarray(alpha_bar, dtype=np.float32).astype(np.float64).reshape(-1)
    T = ab.shape[0]
    if isinstance(S, (list, tuple, np.ndarray)):
        return ddim_steps(T, S)
    if not _is_int(S) or S < 1 or S > T:
        raise ValueError(f"logsnr_steps: S = {S!r} steps out of T = {T} (needs an integer in 1..{T})")
    S = int(S)
    if S == 1:
        return [T - 1]
    lam = 0.5 * np.log(ab / (1.0 - ab))
    tau = sorted({int(np.argmin(np.abs(lam - target))) for target in np.linspace(lam[0], lam[-1], S)})
    assert tau[0] == 0 and tau[-1] == T - 1
    return tau


def dpmpp_coefficients(alpha_bar, tau):
    """Update tables of DPM-Solver++(2M) (Lu et al., 2022: the second-order multistep solver in the data prediction)
    over the steps ``tau``: float32 [5][S] = m1..m5 with ``a_s = abar[tau_s]``, ``p_s = abar[tau_{s-1}]`` (``p_0 = 1``),
    ``lam(v) = log(sqrt(v) / sqrt(1 - v))`` and ``h_s = lam(p_s) - lam(a_s)`` (``h_0 = +inf``): ``m1 = sqrt(1-a)``,
    ``m2 = sqrt(a)``, ``m3 = sqrt((1-p)/(1-a))`` (``m3[0] = 0``), ``m4 = sqrt(p) (-expm1(-h))`` (``m4[0] = 1``),
    ``m5[s] = h_s / (2 h_{s+1})`` for 1 <= s <= S-2 and 0 otherwise -- the first step of a run (s = S-1) has no history,
    the last (s = 0) goes to sigma = 0, where the extrapolation is undefined, so both are first order.  float64 from the
    float32 ``Alpha_bar``, rounded once (the convention of ``ddim_coefficients``).  The engine's step is then
    ``x0 = (x - m1 eps) / m2; D = x0 + m5 (x0 - x0_prev) where there is history and m5 != 0, else x0; x = m3 x + m4 D``;
    with ``m5 = 0`` it is DDIM's at eta = 0."""
    if isinstance(alpha_bar, torch.Tensor):
        alpha_bar = alpha_bar.detach().cpu().numpy()
    ab = np.asarray(alpha_bar, dtype=np.float32).astype(np.float64)
    tau = np.asarray(tau, dtype=np.int64).reshape(-1)
    S = tau.shape[0]
    a = ab[tau]
    p = np.concatenate([[1.0], ab[tau[:-1]]])
    lam = lambda v: np.log(np.sqrt(v) / np.sqrt(1.0 - v))
    h = np.concatenate([[np.inf], lam(p[1:]) - lam(a[1:])])
    m5 = np.zeros(S)
    m5[1:S - 1] = h[1:S - 1] / (2.0 * h[2:S])
    m = np.stack([np.sqrt(1.0 - a), np.sqrt(a), np.sqrt((1.0 - p) / (1.0 - a)), np.sqrt(p) * -np.expm1(-h), m5])
    return m.astype(np.float32)


def sampling_dpmpp(net, size, dh_train, steps, condition=None, *, spacing="logsnr", x_T=None, seed=None,
                   use_graph=True, known=None, mask=None, known_noise=None, x_start=None, start_step=None,
                   start_noise=None, resample=None, noise=None, labels=None, cfg_scale=None, lengths=None,
                   prior_std=None, prior_filter=None, prior_stft=None):
    """DPM-Solver++(2M) over ``logsnr_steps(Alpha_bar, steps)`` of the training schedule ``dh_train``
    (``spacing="uniform"``: over ``ddim_steps(T, steps)``; ``steps``: S or an explicit list).  Second order at the cost
    of DDIM: one network evaluation per step, the previous step's data prediction kept on the device.  Deterministic:
    ``seed`` drives only a drawn ``x_T``, the known-region noise, the start noise and the jump noise; ``noise`` is
    accepted only together with ``resample`` ([V, B, C, L], of which the rows of jump visits are read).  The editing
    arguments and ``resample`` are those of ``sampling`` (levels: ``Alpha_bar[tau]``); the step after a jump and the
    first step of a partial start are first order.  ``labels`` / ``cfg_scale`` as in ``sampling``; ``prior_std`` as
    there too: with no update noise it scales a drawn ``x_T`` and the known-region, start and jump noise;
    ``prior_filter`` / ``prior_stft`` (spectral prior) as in ``sampling``: only ``x_T`` is shaped.  Not the reference's
    loop."""
    if spacing not in ("logsnr", "uniform"):
        raise ValueError(f"sampling_dpmpp: spacing = {spacing!r} (expected 'logsnr' or 'uniform')")
    if noise is not None and resample is None:
        raise ValueError("sampling_dpmpp: the solver is deterministic; noise= is read only by the jump visits of "
                         "resample=")
    ab = _host_table(dh_train["Alpha_bar"])[0]
    tau = logsnr_steps(ab, steps) if spacing == "logsnr" else ddim_steps(dh_train["T"], steps)
    coef = dpmpp_coefficients(ab, tau)
    edit = dict(known=known, mask=mask, known_noise=known_noise, x_start=x_start, start_step=start_step,
                start_noise=start_noise)
    if prior_filter is not None or prior_stft is not None:
        x_T, _, seed = _spectral_prior_run("sampling_dpmpp", size, len(tau), False, prior_filter, prior_stft, x_T, None,
                                           seed, lengths, dict(edit, resample=resample, cfg_scale=cfg_scale,
                                                               prior_std=prior_std, noise=noise))
    if resample is None and all(v is None for v in edit.values()):
        edit = None
    return _run_schedule(net, size, _lib.DWS_SAMPLER_DPMPP2M, np.asarray(tau, dtype=np.float32), coef, condition, x_T,
                         noise, seed, use_graph, edit=edit, levels=ab[tau], resample=resample, labels=labels,
                         cfg_scale=cfg_scale, lengths=lengths, prior_std=prior_std)


def sampling_aligned(net, size, diffusion_cfg, condition=None, **kw):
    """DiffWave's fast sampling with step alignment from a ``diffusion:`` config block with a short ``beta`` list:
    the reference's update tables of that list (``calc_diffusion_hyperparams(..., fast=True)``), the network at the
    aligned fractional steps (``align_steps``).  Keyword arguments as ``sampling``."""
    beta = diffusion_cfg.get("beta")
    if beta is None:
        raise ValueError("aligned sampling needs diffusion.beta (the short inference schedule, e.g. "
                         "[0.0001, 0.001, 0.01, 0.05, 0.2, 0.5])")
    T, b0, bT = diffusion_cfg["T"], diffusion_cfg["beta_0"], diffusion_cfg["beta_T"]
    dh = calc_diffusion_hyperparams(T, b0, bT, beta=beta, fast=True)
    return sampling(net, size, dh, condition, net_steps=align_steps(T, b0, bT, beta), **kw)


# --------------------------------------------------------------------------- guided runs (not the reference's)
def declip_operator(c):
    """Measurement operator of a clipped recording: ``A(x) = x.clamp(-c, c)`` (``c > 0``)."""
    c = float(c)
    if not c > 0:
        raise ValueError(f"declip_operator: c = {c!r} (needs a clipping level > 0)")
    return lambda x: x.clamp(-c, c)


def lowpass_taps(factor, taps=33):
    """float64 [taps]: sinc of cutoff ``1/factor`` (of Nyquist) under a Hann window without its zero end points,
    normalised to unit sum."""
    if not _is_int(factor) or factor < 1:
        raise ValueError(f"lowpass_operator: factor = {factor!r} (needs an integer >= 1)")
    if not _is_int(taps) or taps < 1 or int(taps) % 2 == 0:
        raise ValueError(f"lowpass_operator: taps = {taps!r} (needs an odd integer >= 1)")
    taps = int(taps)
    k = np.arange(taps, dtype=np.float64)
    h = np.sinc((k - (taps - 1) / 2) / int(factor)) * (0.5 - 0.5 * np.cos(2 * np.pi * (k + 1) / (taps + 1)))
    return h / h.sum()


def lowpass_operator(factor, taps=33):
    """Measurement operator of a band-limited recording: ``A(x)[..., j] = sum_k h[k] x[..., j factor + k - (taps-1)/2]``
    with ``h = lowpass_taps(factor, taps)`` and zeros outside the clip ("same" padding), i.e. low-pass then decimation by
    ``factor``: [..., L] -> [..., ceil(L / factor)].  Written with strided slices and sums (differentiable, any device,
    no convolution library on the path)."""
    h = lowpass_taps(factor, taps)
    factor, half = int(factor), (len(h) - 1) // 2

    def A(x):
        L = x.shape[-1]
        xp = torch.cat([x.new_zeros(x.shape[:-1] + (half,)), x, x.new_zeros(x.shape[:-1] + (half,))], dim=-1)
        y = None
        for k, hk in enumerate(h):
            term = xp[..., k:k + L:factor] * float(hk)
            y = term if y is None else y + term
        return y
    return A


def mel_operator(stft=None, **stft_kwargs):
    """Measurement operator of a mel spectrogram: ``A(x) = log-mel(x)`` on the engine (``dws_mel_spectrogram``, adjoint
    ``dws_mel_spectrogram_backward``), [B, 1, L] or [B, L] -> [B, n_mel_channels, L // hop_length + 1].  ``stft`` is a
    ``mel.TacotronSTFT``, or give the keywords it takes (``filter_length``, ``hop_length``, ``win_length``,
    ``n_mel_channels``, ``sampling_rate``, ``mel_fmin``, ``mel_fmax``).  Unlike ``TacotronSTFT.mel_spectrogram`` there is
    no [-1, 1] assertion: x0 estimates leave that range, and the check would be a host synchronisation per step.  GPU
    tensors only (no CPU fallback).  Where a DFT magnitude is exactly zero its gradient is taken as 0 (torch autograd
    through a restated transform returns NaN there); first order only."""
    from .mel import TacotronSTFT
    if stft is None:
        stft = TacotronSTFT(**stft_kwargs)
    elif stft_kwargs:
        raise ValueError(f"mel_operator: give a TacotronSTFT or its keywords, not both (got {sorted(stft_kwargs)} too)")
    elif not isinstance(stft, TacotronSTFT):
        raise ValueError(f"mel_operator: stft = {type(stft).__name__} (needs a mel.TacotronSTFT or its keywords)")

    def A(x):
        if x.dim() == 3:
            if x.shape[1] != 1:
                raise ValueError(f"mel_operator: the waveform has shape {tuple(x.shape)}, expected [B, 1, L] or [B, L]")
            x = x[:, 0]
        elif x.dim() != 2:
            raise ValueError(f"mel_operator: the waveform has shape {tuple(x.shape)}, expected [B, 1, L] or [B, L]")
        return stft.differentiable_mel(x)
    A.stft = stft
    return A


def guided_coefficients(dh, sampler, steps=None, eta=0.0):
    """Tables of ``sampling_guided``: (net_steps float32 [S], float32 [6][S] = k1, k2, a, b, c, 0/1) with the x0
    estimate ``u = (x - k1 eps) / k2`` and the unguided update written for both samplers as
    DDIM ``x = a u + b eps + c z`` (a, b, c = k3, k4, k5 of ``ddim_coefficients``; last row 1) and
    DDPM ``x = (x - a eps) / b + c z`` (``a = (1 - Alpha) / sqrt(1 - Alpha_bar)``, ``b = sqrt(Alpha)``, ``c = Sigma`` in
    float32 as the reference's loop forms them; ``k1 = sqrt(1 - Alpha_bar)``, ``k2 = sqrt(Alpha_bar)`` in float64 from the
    float32 table, rounded once; last row 0)."""
    T = int(dh["T"])
    if sampler == "ddim":
        if steps is None:
            raise ValueError("sampling_guided: sampler='ddim' needs steps= (the number of DDIM steps, or a list)")
        tau = ddim_steps(T, steps)
        k = ddim_coefficients(dh["Alpha_bar"], tau, eta)
        return np.asarray(tau, dtype=np.float32), np.concatenate([k, np.ones((1, len(tau)), np.float32)])
    if sampler != "ddpm":
        raise ValueError(f"sampling_guided: sampler = {sampler!r} (guided runs are built for 'ddpm' and 'ddim'; "
                         "'dpmpp2m' and 'aligned' are not)")
    if steps is not None and (not _is_int(steps) or int(steps) != T):
        raise ValueError(f"sampling_guided: sampler='ddpm' runs the {T} steps of its schedule (steps = {steps!r}); "
                         "pass a short diffusion.beta schedule or use sampler='ddim'")
    if float(eta) != 0.0:
        raise ValueError("sampling_guided: eta is DDIM's")
    Alpha, Alpha_bar, Sigma = (dh[k].detach().cpu().to(torch.float32) for k in ("Alpha", "Alpha_bar", "Sigma"))
    ab = Alpha_bar.numpy().astype(np.float64)
    a = ((1 - Alpha) / torch.sqrt(1 - Alpha_bar)).numpy()
    k = np.stack([np.sqrt(1.0 - ab).astype(np.float32), np.sqrt(ab).astype(np.float32), a, torch.sqrt(Alpha).numpy(),
                  Sigma.numpy(), np.zeros(T, np.float32)])
    return np.arange(T, dtype=np.float32), k.astype(np.float32)


def sampling_guided(net, size, diffusion_hyperparams, *, measurement, operator, scale, sampler="ddpm", steps=None,
                    eta=0.0, condition=None, x_T=None, noise=None, seed=None, residuals=None, labels=None,
                    prior_std=None, **unsupported):
    """Restoration with a trained model by Diffusion Posterior Sampling (Chung et al., ICLR 2023): a reverse run whose
    every step is pulled towards a degraded recording ``measurement = operator(x0)``.  ``operator`` is any differentiable
    torch callable ``A(x0) -> measurement-shaped tensor`` (``declip_operator``, ``lowpass_operator``, or ``mel_operator``:
    the engine's own log-mel with its HIP adjoint, for a measurement that is a mel spectrogram -- e.g. the conditioning
    mel of a vocoder run; engine models / cuda tensors only).  Per step s
    (S-1 .. 0; tables: ``guided_coefficients``)::

        eps = net((x, t_s))                       # differentiable call, x.requires_grad
        u   = (x - k1 eps) / k2                   # x0 estimate
        n_b = || y_b - A(u)_b ||_2                # per clip
        g   = d(sum_b n_b) / dx                   # autograd through A and u, the network's input gradient through eps
        x   = update(x, eps, z_s) - scale * g     # update: the unguided step of ``sampling`` / ``sampling_ddim``

    i.e. DPS with zeta_s = (scale / 2) / ||r||.  A clip whose residual is exactly zero gets no guidance term; the
    guidance is applied at every step, s = 0 included.  ``scale`` must not be zero (that is ``sampling`` /
    ``sampling_ddim``); no default is offered -- it depends on the operator and the model.

    ``sampler``: ``"ddpm"`` (the loop of ``sampling`` over ``dh``, e.g. a short ``diffusion.beta`` schedule) or
    ``"ddim"`` (``steps`` of the training schedule ``dh`` with ``eta``).  ``noise``: injected z [S, B, C, L]
    (``noise[s]`` after step s > 0), ``x_T``: the initial state; otherwise both are drawn -- with an engine model from
    the Philox streams the plain samplers use (stream s for step s, stream S for ``x_T``; ``seed`` as there), with any
    other ``net`` from a torch CPU generator seeded with ``seed``.  ``seed`` may be a list of B per-clip seeds as in
    ``sampling`` (``dws_philox_normal_clips``; with another ``net`` one generator per clip): clip b then draws the noise
    of the B = 1 run with ``seed[b]``.  ``residuals``: a list that receives ``n`` [B] of every step (diagnostics).

    ``net`` is any differentiable callable of the reference surface on any device.  With an engine model every step is
    a training forward and a DATA-ONLY backward (``dws_model_forward_input`` / ``dws_model_backward_input``): put the
    model in ``eval()`` mode, or the full backward runs.  In ``eval()`` mode ``L`` is free for both backbones: a SaShiMi
    model runs shorter and longer than its kernels' ``l_max`` (truncated / clamped taps) and on stages beyond 16384
    samples (the segmented convolution and its adjoint) -- a recording or a mel of any length, within the pooling
    factors' product.  In ``train()`` mode a SaShiMi model raises ``NotImplementedError`` at any other length than its
    kernels' own: parameter gradients are not built there.  Precision f32 / bf16x6; a mel ``[1, bands, Tmel]`` is
    expanded to the batch.  The loop runs eagerly, one step after the other with
    no graph capture: each step contains a backward.  Costs a forward plus a backward per step.  The editing arguments
    (``known`` / ``mask`` ..., ``resample``) and ``cfg_scale`` are not built for guided runs; ``labels`` ([B], a
    class-conditional model) are passed to every network call.  ``prior_std`` ([B, 1, L] or [B, C, L], finite, > 0): the
    adaptive prior of ``sampling`` -- every z, drawn or injected, is multiplied by it (one product of its own) before
    ``c z`` is formed, and so is a drawn initial state; it works with any ``net``.  Not the reference's loop."""
    if unsupported.get("prior_filter") is not None or unsupported.get("prior_stft") is not None:
        raise ValueError("sampling_guided: prior_filter= (spectral prior) is not built for guided runs (their noise sites "
                         "are not shaped)")
    unsupported.pop("prior_filter", None)
    unsupported.pop("prior_stft", None)
    if unsupported.get("cfg_scale") is not None and prior_std is not None:
        raise ValueError("sampling_guided: prior_std= (adaptive prior) is not built for classifier-free guidance (cfg_scale=)")
    if unsupported.get("lengths") is not None:
        raise ValueError("sampling_guided: lengths= (ragged batches) is not built for guided runs: every step is a "
                         "training forward")
    unsupported.pop("lengths", None)
    if unsupported.get("cfg_scale") is not None:
        raise ValueError("sampling_guided: cfg_scale= is not built for guided runs (labels= alone conditions the run)")
    unsupported.pop("cfg_scale", None)
    if labels is not None and not int(getattr(net, "n_classes", 0) or 0):
        raise ValueError("sampling_guided: labels= on a model without classes (set model.n_classes)")
    if unsupported:
        known = {"known", "mask", "known_noise", "x_start", "start_step", "start_noise", "resample", "net_steps", "spacing"}
        bad = sorted(unsupported)
        if set(bad) <= known:
            raise ValueError(f"sampling_guided: {', '.join(bad)}: editing, resampling and step alignment are not built "
                             "for guided runs")
        raise TypeError(f"sampling_guided: unexpected arguments {bad}")
    try:
        scale = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"sampling_guided: scale = {scale!r} (needs a number)")
    if scale == 0.0 or scale != scale:
        raise ValueError("sampling_guided: scale = 0 is the unguided run: call sampling / sampling_ddim")
    if not callable(operator):
        raise ValueError("sampling_guided: operator must be a differentiable callable A(x0)")
    if len(size) != 3:
        raise ValueError(f"sampling_guided: size = {tuple(size)!r} (needs (B, C, L))")
    net_steps, k = guided_coefficients(diffusion_hyperparams, sampler, steps, eta)
    S = len(net_steps)
    B, C, L = (int(v) for v in size)
    size = (B, C, L)
    if noise is not None and tuple(noise.shape) != (S,) + size:
        raise ValueError(f"sampling_guided: noise has shape {tuple(noise.shape)}, expected {(S,) + size}")
    if x_T is not None and tuple(x_T.shape) != size:
        raise ValueError(f"sampling_guided: x_T has shape {tuple(x_T.shape)}, expected {size}")
    prior = _check_prior(size, prior_std)
    from .models.engine import EngineModule
    engine = isinstance(net, EngineModule)
    if engine:
        dev = next(net.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("libdws runs on the GPU only: move the model to cuda (there is no CPU fallback)")
    else:
        p = next(iter(net.parameters()), None) if hasattr(net, "parameters") else None
        dev = p.device if p is not None else torch.as_tensor(measurement).device
    y = torch.as_tensor(measurement).detach().to(device=dev, dtype=torch.float32)
    if condition is not None:
        condition = condition.detach().to(dev)
    seeds = seed_list(seed, B)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    gen = None
    if prior is not None:
        prior = prior.to(dev)
    scaled = (lambda z: z) if prior is None else (lambda z: prior * z)     # n = sigma z stands where z stood

    def draw(stream_id):
        nonlocal gen
        if engine:
            z = torch.empty(size, device=dev, dtype=torch.float32)
            with torch.cuda.device(dev):
                if seeds is None:
                    _lib.check(_lib.load().dws_philox_normal(z.data_ptr(), z.numel(), seed, stream_id,
                                                             _lib.current_stream()))
                else:
                    _lib.check(_lib.load().dws_philox_normal_clips(z.data_ptr(), B, C * L, (ctypes.c_uint64 * B)(*seeds),
                                                                   stream_id, _lib.current_stream()))
            return z
        if seeds is not None:     # a generator per clip, each drawing its clip as the scalar form draws a B = 1 batch
            if gen is None:
                gen = [torch.Generator().manual_seed(k % (2 ** 63)) for k in seeds]
            return torch.cat([torch.randn((1, C, L), generator=g) for g in gen]).to(dev)
        if gen is None:
            gen = torch.Generator().manual_seed(seed % (2 ** 63))
        return torch.randn(size, generator=gen).to(dev)

    x = scaled(draw(S)) if x_T is None else x_T.detach().to(device=dev, dtype=torch.float32).clone()
    kw = {} if condition is None else {"mel_spec": condition}
    if labels is not None:      # class-conditional model: every step's network call carries the labels
        kw["labels"] = labels
    for s in range(S - 1, -1, -1):
        k1, k2, a, b, c, ddim = (float(v) for v in k[:, s])
        t = torch.full((B, 1), float(net_steps[s]), device=dev, dtype=torch.float32)
        with torch.enable_grad():
            xin = x.detach().requires_grad_(True)
            eps = net((xin, t), **kw)
            u = (xin - k1 * eps) / k2
            Au = operator(u)
            if Au.shape != y.shape:
                raise ValueError(f"sampling_guided: the operator gives {tuple(Au.shape)}, the measurement is "
                                 f"{tuple(y.shape)}")
            r = (y - Au).reshape(B, -1)
            sq = (r * r).sum(dim=1)
            live = sq > 0
            n = torch.where(live, torch.sqrt(torch.where(live, sq, torch.ones_like(sq))), torch.zeros_like(sq))
            g = torch.autograd.grad(n.sum(), xin)[0] if bool(live.any()) else torch.zeros_like(x)
        with torch.no_grad():
            eps = eps.detach()
            if residuals is not None:
                residuals.append(n.detach().cpu())
            x = a * ((x - k1 * eps) / k2) + b * eps if ddim else (x - a * eps) / b
            if s > 0:
                z = scaled(draw(s) if noise is None else noise[s].detach().to(device=dev, dtype=torch.float32))
                x = x + c * z
            x = x - scale * g
    return x

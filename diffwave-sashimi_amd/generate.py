"""``generate.py``-compatible driver on the HIP engine.

Same call surface and on-disk conventions as the reference (``generate.py:58-231``,
``utils.py:23-45,96-116``): Hydra-style config tree + ``key=value`` overrides,
``exp/<run>/checkpoint/<iter>.pkl`` holding ``{'model_state_dict': ...}``, run-directory
naming, ``<iter//1000>k_<n_samples*rank+i>.wav`` float32 files written with
``scipy.io.wavfile.write``, one process per GPU with no communication.

    python -m diffwave_sashimi_amd.generate --config-dir /path/to/configs experiment=sc09 model=wavenet \
        generate.n_samples=16 generate.ckpt_iter=max

hydra / omegaconf are not needed: ``load_config`` implements the subset the reference's
config tree uses (defaults lists, ``# @package _global_`` experiment files, ``${a.b}``
interpolation, dotted overrides).
"""
import argparse
import copy
import os
import re
import sys
import time

import numpy as np
import torch
import yaml


# --------------------------------------------------------------------------- config
class _Loader(yaml.SafeLoader):
    """SafeLoader with the YAML-1.2 float grammar OmegaConf/Hydra use: PyYAML (YAML 1.1) reads ``2e-4`` -- the
    reference's ``train.learning_rate`` (``configs/config.yaml``) -- as a string."""


_Loader.add_implicit_resolver(
    "tag:yaml.org,2002:float",
    re.compile(r"^[-+]?(?:\d[\d_]*\.[\d_]*(?:[eE][-+]?\d+)?|\.[\d_]+(?:[eE][-+]?\d+)?|\d[\d_]*[eE][-+]?\d+"
               r"|[-+]?\.(?:inf|Inf|INF)|\.(?:nan|NaN|NAN))$"),
    list("-+0123456789."))


def _yaml(text):
    return yaml.load(text, Loader=_Loader)


def _deep_merge(dst, src):
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _deep_merge(dst[k], v)
        else:
            dst[k] = copy.deepcopy(v)
    return dst


def _load_yaml(path):
    with open(path) as f:
        text = f.read()
    return (_yaml(text) or {}), ("@package _global_" in text.split("\n", 1)[0])


def _set_dotted(cfg, key, value):
    parts = key.split(".")
    d = cfg
    for p in parts[:-1]:
        d = d.setdefault(p, {})
    d[parts[-1]] = value


def _get_dotted(cfg, key):
    d = cfg
    for p in key.split("."):
        d = d[p]
    return d


def _resolve(cfg, node=None):
    node = cfg if node is None else node
    items = node.items() if isinstance(node, dict) else enumerate(node)
    for k, v in list(items):
        if isinstance(v, (dict, list)):
            _resolve(cfg, v)
        elif isinstance(v, str):
            m = re.fullmatch(r"\$\{([^}]+)\}", v.strip())
            if m:
                node[k] = _get_dotted(cfg, m.group(1))
    return cfg


def load_config(config_dir, overrides=(), config_name="config"):
    """Compose ``<config_dir>/<config_name>.yaml`` the way ``@hydra.main`` does for the reference's
    tree (``configs/config.yaml:1-31``): group selections (``experiment=ljspeech``, ``model=wavenet``)
    pick files, ``/group: name`` defaults inside a ``# @package _global_`` experiment file mount under
    ``group`` BEFORE the file's own keys (so ``experiment/ljspeech.yaml``'s ``model.unconditional: false``
    lands on whichever model file was chosen), then dotted overrides, then ``${a.b}`` interpolation."""
    groups, values = {}, []
    for ov in overrides:
        k, _, v = ov.lstrip("+").partition("=")
        if "." not in k and os.path.isdir(os.path.join(config_dir, k)):
            groups[k] = v
        else:
            values.append((k, _yaml(v)))
    root, _ = _load_yaml(os.path.join(config_dir, config_name + ".yaml"))
    cfg = {}

    def mount(group, name):
        sub, is_global = _load_yaml(os.path.join(config_dir, group, str(name) + ".yaml"))
        for d in sub.pop("defaults", []):
            if isinstance(d, dict):
                for g, n in d.items():
                    g = g.lstrip("/")
                    mount(g, groups.get(g, n))
        if is_global:
            _deep_merge(cfg, sub)
        else:
            _deep_merge(cfg.setdefault(group, {}), sub)

    defaults = root.pop("defaults", [])
    if "_self_" not in defaults:
        defaults = list(defaults) + ["_self_"]
    for d in defaults:
        if d == "_self_":
            _deep_merge(cfg, root)
        elif isinstance(d, dict):
            for g, n in d.items():
                mount(g, groups.get(g, n))
    for k, v in values:
        _set_dotted(cfg, k, v)
    return _resolve(cfg)


# --------------------------------------------------------------------------- run directories / checkpoints
def find_max_epoch(path):
    """``utils.py:23-45``: largest ``<n>.pkl`` in ``path`` (-1 if none)."""
    epoch = -1
    for f in os.listdir(path):
        if len(f) > 4 and f.endswith(".pkl"):
            try:
                epoch = max(epoch, int(f[:-4]))
            except ValueError:
                continue
    return epoch


def local_path_name(name, model_cfg, diffusion_cfg, dataset_cfg):
    """Run-directory name of ``utils.py:96-108``, e.g. ``wnet_h128_d30_T200_betaT0.02_uncond``."""
    from .models import model_identifier
    model_name = model_identifier(model_cfg)
    diffusion_name = f"_T{diffusion_cfg['T']}_betaT{diffusion_cfg['beta_T']}"
    data_name = "" if model_cfg["unconditional"] else f"_L{dataset_cfg['segment_length']}_hop{dataset_cfg['hop_length']}"
    local_path = model_name + diffusion_name + data_name + f"_{'uncond' if model_cfg['unconditional'] else 'cond'}"
    if name:
        local_path = name + "_" + local_path
    return local_path


def local_directory(name, model_cfg, diffusion_cfg, dataset_cfg, output_directory, root="exp"):
    local_path = local_path_name(name, model_cfg, diffusion_cfg, dataset_cfg)
    output_directory = os.path.join(root, local_path, output_directory)
    os.makedirs(output_directory, mode=0o775, exist_ok=True)
    return local_path, output_directory


def smooth_ckpt(path, min_ckpt, max_ckpt, priors=None, banks=None):
    """``utils.py:47-74,154-166`` (experimental in the reference): running arithmetic mean of the
    ``model_state_dict`` of every checkpoint with ``min_ckpt < iteration <= max_ckpt``.  ``priors``: a list that receives
    ``(iteration, prior entry or None)`` of every checkpoint that went into the mean; ``banks``: the same of the ``pqmf``
    entries."""
    ckpts = []
    for f in os.listdir(path):
        if len(f) > 4 and f.endswith(".pkl"):
            try:
                it = int(f[:-4])
            except ValueError:
                continue
            if min_ckpt < it <= max_ckpt:
                ckpts.append(it)
    state_dict = None
    for n, it in enumerate(sorted(ckpts)):
        model_path = os.path.join(path, f"{it}.pkl")
        try:
            checkpoint = torch.load(model_path, map_location="cpu")
            sd = checkpoint["model_state_dict"]
        except Exception:
            raise Exception(f"No valid model found at iteration {it}, path {model_path}")
        if priors is not None:
            priors.append((it, checkpoint.get("prior")))
        if banks is not None:
            banks.append((it, checkpoint.get("pqmf")))
        state_dict = sd if state_dict is None else {k: (state_dict[k] * n + sd[k]) / (n + 1) for k in sd}
    return state_dict


def weights_key(checkpoint, ema=None, ckpt_smooth=None):
    """Which entry of a loaded checkpoint dict ``generate`` samples from: ``ema_state_dict`` (written by training runs
    with ``train.ema_decay``) or ``model_state_dict``.  ``ema`` = None (default): the EMA when the checkpoint has one;
    True: the EMA, an error when it has none; False: the raw weights.  ``ckpt_smooth`` averages the raw weights of several
    checkpoints, which ``ema=True`` contradicts (refused); otherwise it takes ``model_state_dict``."""
    if ema is not None and not isinstance(ema, bool):
        raise ValueError(f"generate.ema={ema!r}: expected true or false")
    if ckpt_smooth is not None:
        if ema:
            raise ValueError("generate.ema=true does not combine with generate.ckpt_smooth (an average of raw checkpoints)")
        return "model_state_dict"
    has = checkpoint is not None and "ema_state_dict" in checkpoint
    if ema and not has:
        raise ValueError("generate.ema=true, but the checkpoint holds no ema_state_dict (train with train.ema_decay)")
    return "ema_state_dict" if (has and ema is not False) else "model_state_dict"


# --------------------------------------------------------------------------- generate
def clip_plan(n_samples, batch_size, rank=0, num_ranks=1, clip_seeds=False, clips=None, seed=None):
    """Which global clips one rank generates under ``generate.clip_seeds``, as a list of batches (lists of global clip
    numbers ``k``, the number in the wav's name).  Without ``clips``: clip i of rank r is ``k = n_samples r + i``, in
    batches of ``batch_size`` (which divides ``n_samples``).  With ``clips`` (a list of global clip numbers): rank r of N
    takes ``clips[r::N]`` in batches of up to ``batch_size`` -- the last may be smaller, a rank may get none.  Pure host
    arithmetic.  ``clips`` without ``clip_seeds`` and ``clip_seeds`` without ``seed`` are refused (ValueError)."""
    if isinstance(clip_seeds, str) or clip_seeds not in (None, False, True, 0, 1):
        raise ValueError(f"generate.clip_seeds={clip_seeds!r}: expected true or false")
    if clips is not None and not clip_seeds:
        raise ValueError("generate.clips needs generate.clip_seeds=true (only per-clip seeds make a clip reproducible on "
                         "its own)")
    if not clip_seeds:
        return None
    if seed is None or isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError("generate.clip_seeds needs generate.seed (an integer: the clips' seeds are derived from it)")
    rank, num_ranks = int(rank or 0), int(num_ranks or 1)
    if rank < 0 or (clips is not None and rank >= num_ranks):
        raise ValueError(f"clip_plan: rank {rank} of {num_ranks}")
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"generate.batch_size={batch_size!r}: expected an integer >= 1")
    if clips is None:
        if n_samples % batch_size != 0:
            raise ValueError(f"generate.batch_size={batch_size} does not divide generate.n_samples={n_samples}")
        mine = [n_samples * rank + i for i in range(n_samples)]
    else:
        clips = list(clips) if isinstance(clips, (list, tuple)) else [clips]
        if not clips or any(isinstance(k, bool) or not isinstance(k, int) or k < 0 for k in clips):
            raise ValueError(f"generate.clips={clips!r}: expected a list of global clip numbers (integers >= 0)")
        if len(set(clips)) != len(clips):
            raise ValueError(f"generate.clips={clips!r}: a clip is named twice")
        mine = clips[rank::num_ranks]
    return [mine[i:i + batch_size] for i in range(0, len(mine), batch_size)]


def ragged_plan(frame_counts, batch_size):
    """Batches of a list of utterances of different lengths (``generate.mel_names``): the indices ``k`` into
    ``frame_counts`` sorted by length, longest first (equal lengths keep their order in the list), cut into batches of at
    most ``batch_size`` -- a batch runs at the length of its first utterance, so sorting keeps the padded share small.
    Every index appears exactly once.  Pure host arithmetic."""
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"generate.batch_size={batch_size!r}: expected an integer >= 1")
    counts = list(frame_counts)
    if any(isinstance(f, bool) or not isinstance(f, (int, np.integer)) or f < 1 for f in counts):
        raise ValueError(f"ragged_plan: frame counts are integers >= 1, got {counts!r}")
    order = sorted(range(len(counts)), key=lambda k: -int(counts[k]))     # (sorted is stable)
    return [order[i:i + batch_size] for i in range(0, len(order), batch_size)]


def _check_mel_names(mel_names, mel_name, clip_seeds, seed, **others):
    """Argument checks of ``generate.mel_names`` before a model is built (ValueError).  Returns the list of stems."""
    if mel_name is not None:
        raise ValueError("generate.mel_names and generate.mel_name exclude each other (a list of utterances, or one)")
    names = list(mel_names) if isinstance(mel_names, (list, tuple)) else [mel_names]
    if not names or any(not isinstance(n, str) or not n for n in names):
        raise ValueError(f"generate.mel_names={mel_names!r}: expected a list of wav stems")
    if len(set(names)) != len(names):
        raise ValueError(f"generate.mel_names={mel_names!r}: an utterance is named twice")
    if isinstance(clip_seeds, str) or clip_seeds not in (None, False, True, 0, 1):
        raise ValueError(f"generate.clip_seeds={clip_seeds!r}: expected true or false")
    if clip_seeds and (seed is None or isinstance(seed, bool) or not isinstance(seed, int)):
        raise ValueError("generate.clip_seeds needs generate.seed (an integer: the clips' seeds are derived from it)")
    given = sorted(k for k, v in others.items() if v is not None)
    if given:
        raise ValueError(f"generate.mel_names does not combine with generate.{given[0]} (ragged batches run the plain "
                         "samplers: no editing, restoration, labels or clip selection)")
    return names


PRIOR_KEYS = ("energy_max", "energy_min", "std_min")       # the value keys of a {"kind": "energy"} entry
SPECTRAL_PRIOR_KEYS = ("ref", "floor", "lifter")            # and of a {"kind": "spectral"} one
PRIOR_KEYS_OF = {"energy": PRIOR_KEYS, "spectral": SPECTRAL_PRIOR_KEYS}


def prior_settings(prior, energy_max=None, energy_min=None, std_min=None, unconditional=False, where="generate", *,
                   ref=None, floor=None, lifter=None, n_fft=None):
    """The adaptive-prior keys of a CLI run, checked before a model is built (ValueError):
    ``+{where}.prior=energy +{where}.prior_energy_max=E [+{where}.prior_energy_min=0 +{where}.prior_std_min=0.1]``
    (PriorGrad) or ``+{where}.prior=spectral +{where}.prior_ref=R [+{where}.prior_floor=0.01 +{where}.prior_lifter=24]``
    (SpecGrad; ``n_fft``: ``dataset.filter_length``, which bounds the lifter).  Returns None (no key given), ``"none"``
    (``prior=none``: N(0, I) whatever the checkpoint says) or the dict
    ``{"kind": "energy", "energy_max", "energy_min", "std_min"}`` of ``mel.prior_std_from_mel``'s settings, or
    ``{"kind": "spectral", "ref", "floor", "lifter"}`` of ``TacotronSTFT.spectral_filter``'s."""
    from .mel import _check_filter_design, _check_prior_range
    given = [k for k, v in (("prior_energy_max", energy_max), ("prior_energy_min", energy_min), ("prior_std_min", std_min))
             if v is not None]
    given_s = [k for k, v in (("prior_ref", ref), ("prior_floor", floor), ("prior_lifter", lifter)) if v is not None]
    if prior is None or prior == "none":
        if given:
            raise ValueError(f"{where}.{given[0]} needs {where}.prior=energy")
        if given_s:
            raise ValueError(f"{where}.{given_s[0]} needs {where}.prior=spectral")
        return prior
    if prior not in PRIOR_KEYS_OF:
        raise ValueError(f"{where}.prior={prior!r}: expected energy or none (or spectral, the time-varying spectral prior)")
    if unconditional:
        raise ValueError(f"{where}.prior={prior} needs a mel-conditional model (model.unconditional=false): the prior is "
                         "read off the conditioning mel")
    if prior == "spectral":
        if given:
            raise ValueError(f"{where}.{given[0]} needs {where}.prior=energy (this run names {where}.prior=spectral)")
        if ref is None:
            raise ValueError(f"{where}.prior=spectral needs {where}.prior_ref (the magnitude that maps to gain 1: the largest "
                             "of the dataset, mel.spectral_prior_ref; no default is chosen: it depends on the dataset)")
        if any(isinstance(v, (bool, str)) for v in (ref, floor, lifter)):
            raise ValueError(f"{where}.prior_ref / prior_floor / prior_lifter: expected numbers")
        try:
            r, fl, lf = _check_filter_design(ref, 0.01 if floor is None else floor, 24 if lifter is None else lifter,
                                             1 << 30 if n_fft is None else int(n_fft))
        except ValueError as e:
            raise ValueError(f"{where}.prior=spectral: {e}")
        return {"kind": "spectral", "ref": r, "floor": fl, "lifter": lf}
    if given_s:
        raise ValueError(f"{where}.{given_s[0]} needs {where}.prior=spectral (this run names {where}.prior=energy)")
    if energy_max is None:
        raise ValueError(f"{where}.prior=energy needs {where}.prior_energy_max (the largest frame energy of the dataset, "
                         "mel.mel_energy; no default is chosen: it depends on the dataset)")
    if any(isinstance(v, (bool, str)) for v in (energy_max, energy_min, std_min)):
        raise ValueError(f"{where}.prior_energy_max / prior_energy_min / prior_std_min: expected numbers")
    e_min, e_max, s_min = _check_prior_range(energy_max, 0.0 if energy_min is None else energy_min,
                                             0.1 if std_min is None else std_min)
    return {"kind": "energy", "energy_max": e_max, "energy_min": e_min, "std_min": s_min}


def prior_hop(model_cfg, dataset_cfg):
    """Samples per mel frame of the prior: ``prod(model.mel_upsample)``, which must be ``dataset.hop_length`` (the run
    length is ``frames x hop_length``) -- ValueError otherwise."""
    hop = int(np.prod([int(v) for v in model_cfg.get("mel_upsample", [16, 16])]))
    if dataset_cfg.get("hop_length") != hop:
        raise ValueError(f"adaptive prior: dataset.hop_length={dataset_cfg.get('hop_length')!r} is not the product of "
                         f"model.mel_upsample={list(model_cfg.get('mel_upsample', [16, 16]))} = {hop} (sigma repeats a "
                         "frame's value over the samples the conditioner upsamples it to)")
    return hop


def same_prior(a, b):
    """Two ``prior`` entries (None: N(0, I)) name the same prior: the same kind with the same values (an energy entry and
    a spectral entry never do)."""
    if a is None or b is None:
        return a is None and b is None
    keys = PRIOR_KEYS_OF.get(a.get("kind"), PRIOR_KEYS)
    return a.get("kind") == b.get("kind") and all(k in a and k in b and float(a[k]) == float(b[k]) for k in keys)


def resolve_prior(settings, entry, given=()):
    """The prior a ``generate`` run uses: ``settings`` (``prior_settings``) against the checkpoint's ``prior`` entry (None:
    it has none).  ``"none"`` -> None; no keys -> the entry; another kind than the entry's, or keys that contradict it ->
    ValueError (``given``: the value keys the run spelled out; the others follow the entry)."""
    if settings == "none":
        return None
    if entry is not None and (not isinstance(entry, dict) or entry.get("kind") not in PRIOR_KEYS_OF
                              or any(k not in entry for k in PRIOR_KEYS_OF[entry["kind"]])):
        raise ValueError(f"the checkpoint's prior entry {entry!r} is not one this version writes")
    if settings is None:
        return None if entry is None else dict(entry)
    if entry is None:
        return settings
    if settings["kind"] != entry["kind"]:
        raise ValueError(f"generate.prior={settings['kind']} contradicts the checkpoint, which was trained with the "
                         f"{entry['kind']} prior {entry!r} (drop the key, or generate.prior=none for N(0, I))")
    for k in PRIOR_KEYS_OF[entry["kind"]]:
        if k in given and float(entry[k]) != float(settings[k]):
            raise ValueError(f"generate.prior_{k}={settings[k]!r} contradicts the checkpoint, which was trained with "
                             f"{k}={entry[k]!r} (drop the key, or generate.prior=none for N(0, I))")
    return dict(entry)


def _check_ragged_hop(model_cfg, dataset_cfg):
    """``generate.mel_names`` on SaShiMi, before a model is built (ValueError): an utterance is ``frames x hop_length``
    samples long, and SaShiMi takes per-clip lengths that are multiples of the product of its pooling factors only (a
    pooled stage holds length / factor samples) -- so the hop must be such a multiple.  WaveNet takes any hop."""
    if model_cfg.get("_name_") != "sashimi":
        return
    from .models.sashimi import pool_span
    span = pool_span(model_cfg.get("pool", [4, 4]))
    hop = dataset_cfg["hop_length"]
    if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or hop < 1 or hop % span:
        raise ValueError(f"generate.mel_names with model=sashimi: dataset.hop_length={hop!r} is not a multiple of {span}, "
                         f"the product of model.pool={list(model_cfg.get('pool', [4, 4]))} (utterances of frames x hop "
                         "samples must divide through every pooling stage)")


def _load_clip(dataset_cfg, stem, audio_length, conditional):
    """``<dataset.data_path>/<stem>.wav`` as a [1, 1, audio_length] clip in [-1, 1], read as ``train.SpeechCommands``
    reads one (int16 / 32768, int32 / 2^31, float as it is; first channel).  Unconditional: fitted to the segment the
    way ``train.fix_length`` fits a clip; conditional: the length must be the mel's."""
    from scipy.io import wavfile
    from .train import fix_length
    path = os.path.join(str(dataset_cfg["data_path"]), f"{stem}.wav")
    sr, x = wavfile.read(path)
    if sr != dataset_cfg["sampling_rate"]:
        raise ValueError("{} SR doesn't match target {} SR".format(sr, dataset_cfg["sampling_rate"]))
    if x.dtype == np.int16:
        x = x.astype(np.float32) / 32768.0
    elif x.dtype == np.int32:
        x = x.astype(np.float32) / 2147483648.0
    else:
        x = x.astype(np.float32)
    if x.ndim == 2:
        x = x[:, 0]
    t = torch.from_numpy(np.ascontiguousarray(x)).unsqueeze(0)
    if conditional:
        if t.shape[1] != audio_length:
            raise ValueError(f"{path} has {t.shape[1]} samples; the mel condition needs mel frames x hop_length = "
                             f"{audio_length}")
    else:
        t = fix_length(t, audio_length)
    return t.unsqueeze(0)


def _source_pairs(audio, stems, lens, dataset_cfg, sources):
    """``(x, y, n)``: the clips ``audio`` [B, 1, L] (clip b its first ``lens[b]`` samples) and the source wavs of
    ``stems`` as two [B, max(n)] batches, pair b trimmed to its shorter member ``n[b]``; y on the CPU.  ``sources``: the
    run's dict of the wavs read so far (stem -> [len] in [-1, 1]): each is read once, whichever report asks first."""
    from .mel import MAX_WAV_VALUE, load_wav_to_torch
    for s in set(stems) - set(sources):
        sources[s] = load_wav_to_torch(os.path.join(str(dataset_cfg["data_path"]), f"{s}.wav"))[0] / MAX_WAV_VALUE
    n = [min(int(lens[b]), int(sources[s].shape[0])) for b, s in enumerate(stems)]
    x = audio[:, 0, :max(n)].to(torch.float32)
    y = torch.zeros(len(stems), max(n), dtype=torch.float32)
    for b, s in enumerate(stems):
        y[b, :n[b]] = sources[s][:n[b]]
    return x, y, n


def _check_pitch_source(stem, samples, dataset_cfg):
    """``generate.report_pitch``, before anything is sampled: ValueError where the pair of ``stem`` -- ``samples`` long,
    the shorter of the clip to be generated and its source wav -- is one ``metrics.pitch_metrics`` refuses at
    ``dataset``'s sampling rate and hop (734 samples at 22050 Hz; nothing is clamped)."""
    from .metrics import check_pitch
    check_pitch([int(samples)], sampling_rate=dataset_cfg.get("sampling_rate", 22050), hop=dataset_cfg.get("hop_length", 256),
                what=f"generate.report_pitch ({stem}.wav)")


def _report_pitch(i, audio, stems, numbers, lens, dataset_cfg, rows, shared, sources):
    """``generate.report_pitch``: as ``_report_metrics`` with ``metrics.pitch_metrics`` at ``dataset``'s sampling rate and
    hop.  Prints the nan-means over the batch's clips; the keys go into the dicts ``_report_metrics`` just appended to
    ``rows`` where ``shared``, into new ones otherwise."""
    from .metrics import PITCH_METRICS, nanmean, pitch_metrics
    x, y, n = _source_pairs(audio, stems, lens, dataset_cfg, sources)
    m = pitch_metrics(x, y.to(x.device), n, sampling_rate=dataset_cfg.get("sampling_rate", 22050),
                      hop=dataset_cfg.get("hop_length", 256))
    mean = {k: nanmean(m[k].tolist()) for k in PITCH_METRICS}
    print(f"batch {i} pitch: f0_rmse = {mean['f0_rmse']:.4f} Hz  " +
          "  ".join(f"{k} = {mean[k]:.4f}" for k in PITCH_METRICS[1:]) +
          f"  (nan-means of {len(stems)} clips against their source wavs)")
    if rows is not None:
        for b, s in enumerate(stems):
            values = {k: float(m[k][b]) for k in PITCH_METRICS}
            if shared:
                rows[len(rows) - len(stems) + b].update(values)
            else:
                rows.append(dict(values, name=s, clip=numbers[b]))


def _check_stoi_source(stem, samples, dataset_cfg):
    """``generate.report_stoi``, before anything is sampled: ValueError where ``dataset``'s sampling rate is one
    ``audio.resample`` does not bring to 10 kHz, or the pair of ``stem`` (``samples`` long) is shorter than one frame
    there."""
    from .metrics import stoi_lengths
    stoi_lengths([int(samples)], dataset_cfg.get("sampling_rate", 22050), f"generate.report_stoi ({stem}.wav)")


def _report_stoi(i, audio, stems, numbers, lens, dataset_cfg, rows, shared, sources):
    """``generate.report_stoi``: as ``_report_pitch`` with ``metrics.stoi`` at ``dataset``'s sampling rate."""
    from .metrics import STOI_METRICS, nanmean, stoi
    x, y, n = _source_pairs(audio, stems, lens, dataset_cfg, sources)
    m = stoi(x, y.to(x.device), n, sampling_rate=dataset_cfg.get("sampling_rate", 22050))
    mean = {k: nanmean(m[k].tolist()) for k in STOI_METRICS}
    print(f"batch {i} intelligibility: " + "  ".join(f"{k} = {mean[k]:.4f}" for k in STOI_METRICS) +
          f"  (nan-means of {len(stems)} clips against their source wavs, at 10 kHz)")
    if rows is not None:
        for b, s in enumerate(stems):
            values = {k: float(m[k][b]) for k in STOI_METRICS}
            if shared:
                rows[len(rows) - len(stems) + b].update(values)
            else:
                rows.append(dict(values, name=s, clip=numbers[b]))


def _report_metrics(i, audio, stems, numbers, lens, dataset_cfg, rows, sources):
    """``generate.report_metrics``: the clips of batch ``i`` (``audio`` [B, 1, L] on the GPU, clip b its first
    ``lens[b]`` samples, made from the mel of ``stems[b]``) against their source wavs, each pair trimmed to its shorter
    member.  Prints the batch means and appends one dict per clip to ``rows`` where that is a list."""
    from .mel import TacotronSTFT
    from .metrics import METRICS, spectral_metrics
    keys = ("filter_length", "hop_length", "win_length", "sampling_rate", "mel_fmin", "mel_fmax")
    stft = TacotronSTFT(**{k: dataset_cfg[k] for k in keys if k in dataset_cfg})
    x, y, n = _source_pairs(audio, stems, lens, dataset_cfg, sources)
    m = spectral_metrics(x, y.to(x.device), n, stft=stft)
    print(f"batch {i} metrics: " + "  ".join(f"{k} = {float(m[k].mean()):.4f}" for k in METRICS) +
          f"  (mcd in dB; means of {len(stems)} clips against their source wavs)")
    if rows is not None:
        for b, s in enumerate(stems):
            rows.append(dict({k: float(v[b]) for k, v in m.items()}, name=s, clip=numbers[b]))


@torch.no_grad()
def generate(rank, diffusion_cfg, model_cfg, dataset_cfg, ckpt_iter="max", n_samples=1, name=None, batch_size=None,
             ckpt_smooth=None, mel_path=None, mel_name=None, dataloader=None, exp_root="exp", seed=None,
             written=None, precision=None, sampler="ddpm", steps=None, eta=0.0, known_name=None, keep=None,
             start_name=None, start_step=None, start_noise=True, resample_jump=None, resample_n=None, spacing=None,
             guide_name=None, guide_op=None, guide_clip=None, guide_factor=None, guide_scale=None, label=None,
             cfg_scale=None, ema=None, clip_seeds=None, clips=None, num_ranks=None, report_mel=None, mel_errors=None,
             mel_names=None, prior=None, prior_energy_max=None, prior_energy_min=None, prior_std_min=None,
             report_metrics=None, metric_rows=None, report_pitch=None, report_stoi=None, start_griffinlim=None,
             griffinlim_momentum=None, prior_ref=None, prior_floor=None, prior_lifter=None):
    """``generate.py:58-200``.  ``ckpt_iter`` may additionally be ``"init"``: seeded random weights
    (no checkpoint), for smoke runs without trained weights.  ``precision`` (not in the reference; CLI:
    ``+engine.precision=bf16x6|f16x3``): the engine's opt-in matrix arithmetic, see ``include/dws.h``.

    ``sampler`` (not in the reference; CLI ``generate.sampler=...``): ``ddpm`` (default) is the reference's loop,
    including its use of ``diffusion.beta``; ``aligned`` runs the short ``diffusion.beta`` schedule with the network at
    the aligned fractional training steps (``sampling.align_steps``); ``ddim`` runs DDIM over ``steps`` of the T
    training steps with ``eta`` (default 0); ``dpmpp2m`` runs DPM-Solver++(2M), the second-order multistep solver, over
    ``steps`` of the T training steps spaced uniformly in log-SNR (``spacing`` = ``logsnr``, the default; the count can
    come out below ``steps`` where targets collide) or as DDIM spaces them (``uniform``).  It is deterministic: a
    non-zero ``eta`` is refused.

    Editing (not in the reference; with any ``sampler``): ``known_name`` (a wav stem under ``dataset.data_path``) with
    ``keep`` (``[start, end)`` sample spans of it that are kept) inpaints the rest -- every clip of the batch gets the
    same known audio and its own noise; ``start_name`` with ``start_step`` starts the loop at that step from the wav,
    noised to the step's level first unless ``start_noise`` is false (then the wav is the state as given).
    ``resample_jump`` with ``resample_n`` (both or neither; they need ``known_name``) run the inpainting with RePaint's
    resampling: at every ``resample_jump``-th position the chain goes back up that many steps and down again,
    ``resample_n`` times in all (``sampling.repaint_program``).

    Warm start (not in the reference; mel-conditional runs, ``mel_name`` and ``mel_names``): ``start_griffinlim`` = N
    (0 .. 4096) with ``start_step`` starts the loop from the Griffin-Lim estimate of the conditioning mel itself
    (``TacotronSTFT.mel_to_audio`` at the dataset's STFT keys, N iterations, ``griffinlim_momentum`` in [0, 1), default
    0) instead of a wav; the mel's last frame is repeated once so that the estimate has frames x hop samples, and with
    ``mel_names`` every clip is inverted at its own length.  Everything behind it is the partial start above
    (``start_noise`` included).  Refused on unconditional runs, together with ``start_name``, without ``start_step``, with
    ``mel_path`` (the STFT keys of stored mels are unknown) and with ``model.subbands``.

    Restoration (not in the reference; ``sampler`` ddpm or ddim, no editing): ``guide_name`` (a wav stem under
    ``dataset.data_path``, the degraded recording, at ``dataset.sampling_rate``) with ``guide_op`` = ``declip`` (the
    recording is clipped at ``guide_clip``, default its largest magnitude) or ``lowpass`` (the recording is band-limited:
    its measurement is the wav low-passed and decimated by ``guide_factor``, default 2) and ``guide_scale`` (the
    guidance step, required: there is no default that fits every model and operator) runs Diffusion Posterior Sampling,
    ``sampling.sampling_guided`` -- a forward and a data-only backward of the network per step, every clip of the batch
    guided by the same recording.  ``guide_op=mel`` guides towards a mel spectrogram through ``sampling.mel_operator``
    (the engine's log-mel and its HIP adjoint; ``guide_clip`` / ``guide_factor`` are refused): with ``guide_name`` the
    measurement is the engine's mel of that wav -- 80 bands at ``dataset.sampling_rate``, ``filter_length`` /
    ``hop_length`` / ``win_length`` / ``mel_fmin`` / ``mel_fmax`` from ``dataset`` where present, else 1024 / 256 / 1024,
    0 and min(8000, sampling_rate / 2); without ``guide_name``, on a mel-conditional run (``mel_name``) only, it is the
    conditioning mel itself, which keeps a vocoder on its mel.  ``report_mel=true`` (mel-conditional runs, any sampler)
    prints per batch the mean absolute difference between the engine's log-mel of the generated clips and the
    conditioning mel (over the frames of the condition), and appends it to ``mel_errors`` where that is a list.

    Objective metrics (not in the reference; ``mel_name`` / ``mel_names`` runs whose mel is computed from
    ``<dataset.data_path>/<stem>.wav``, any sampler): ``report_metrics=true`` compares every written clip with its source
    wav through ``metrics.spectral_metrics`` (the pair trimmed to the recording's length; the log-mel terms at
    ``dataset``'s transform), prints per batch the means of ``mr_stft / ls_mae / lsd / mcd`` and appends one dict per clip
    (``name``, ``clip`` and every metric) to ``metric_rows`` where that is a list.  With ``mel_path`` tensors (there is no
    source wav) and on unconditional runs it is a ValueError.  ``report_pitch=true`` (the same runs, the same
    ValueErrors; alone or with ``report_metrics``) does the same through ``metrics.pitch_metrics`` at ``dataset``'s
    sampling rate and hop: it prints per batch the nan-means of ``f0_rmse / f0_cents / gpe / vuv_error / vuv_f1 /
    periodicity_rmse`` over the clips (a clip with no frame voiced in both signals has no F0 numbers) and adds the six
    keys to the clip's dict in ``metric_rows`` -- the dict of ``report_metrics`` where both are on.  A clip or source wav
    shorter than the tracker admits (734 samples at 22050 Hz and hop 256) is a ValueError before anything is sampled.
    ``report_stoi=true`` (the same runs, the same ValueErrors; alone or with either) does the same through
    ``metrics.stoi`` at ``dataset``'s sampling rate: the nan-means of ``stoi / estoi`` per batch (a clip that keeps fewer
    than 30 frames at 10 kHz has neither) and the two keys in ``metric_rows``; a sampling rate the resampler does not
    bring to 10 kHz, or a clip shorter than one 256-sample frame there, is a ValueError before anything is sampled.

    Class-conditional models (``model.n_classes = K``; not in the reference): ``label`` is a class index in 0..K (K = the
    null class), a list of them cycled over the samples, or ``all`` (= 0..K-1 in turn); the wav names get ``_c{label}``.
    ``cfg_scale`` adds classifier-free guidance (``sampling``'s ``cfg_scale``: twice the network batch per step); it needs
    ``label`` and does not combine with the editing or restoration keys.  No trained class-conditional weights exist
    here: what the samples sound like has not been measured.

    ``ema`` (not in the reference; CLI ``+generate.ema=true|false``): which weights of the checkpoint are sampled, see
    ``weights_key``.  The default takes ``ema_state_dict`` when the checkpoint has one (runs trained with
    ``train.ema_decay``) and ``model_state_dict`` otherwise.

    Reproducible clips (not in the reference; with every ``sampler`` and the editing, resampling, label / CFG and guide
    keys): ``clip_seeds=true`` (needs ``seed``) seeds every clip on its own -- global clip ``k = n_samples rank + i``, the
    number in its wav name, draws from ``sampling.clip_seeds(seed, k, 1)`` and, with ``label``, has the class
    ``labels[k % len(labels)]`` -- so ``{iter}k_{k}.wav`` is the same file for any ``batch_size`` dividing ``n_samples``
    and any number of ranks (``num_ranks``: the processes of the run, one per GPU) that produces clip k.

    Ragged batches (not in the reference; mel-conditional WaveNet or SaShiMi, the latter with ``hop_length`` a multiple
    of the product of ``model.pool``): ``mel_names`` is a LIST of utterances (wav stems, as
    ``mel_name`` names one; the two exclude each other), each vocoded once.  ``ragged_plan`` sorts them longest first and
    cuts batches of at most ``batch_size`` (default: all in one); ranks take the batches round-robin.  A batch runs at
    the length of its longest utterance with the per-clip ``lengths`` of ``sampling`` -- every utterance comes out as it
    would alone, none sees another's or its own padding -- and each wav is written trimmed to ``frames x hop_length``
    samples as ``{iter//1000}k_{stem}.wav``.  With ``clip_seeds=true`` the seed of utterance k (its place in the list) is
    ``sampling.clip_seeds(seed, k, 1)``, so the same file comes out at any ``batch_size`` up to the arithmetic of the
    kernel path (the padded length L_max of its batch selects kernels and sets the edge indicators of the Winograd
    correction rows; not bit for bit).  Per batch ``L_max``, the lengths and the padded share are printed: a padded
    position still costs its full time.  Does not combine with the editing, restoration, label and ``clips`` keys.
    Returns the list of the trimmed clips [1, len_k] in the order of ``mel_names`` (None for another rank's).  ``clips``
    (a list of global clip numbers; needs ``clip_seeds``) generates only these, under their usual names: rank r of N takes
    ``clips[r::N]`` in batches of up to ``batch_size`` (``clip_plan``).  Returns the audio of the clips this rank made.

    Adaptive prior (not in the reference; PriorGrad, Lee et al., ICLR 2022; mel-conditional models, every ``sampler``,
    ``mel_name`` and ``mel_names``, with the clip-seed, editing, resampling and guide keys): ``prior=energy`` with
    ``prior_energy_max`` (required) and ``prior_energy_min`` (0) / ``prior_std_min`` (0.1) runs from
    N(0, diag(sigma^2)), sigma = ``mel.prior_std_from_mel`` of the conditioning mel, the ``prior_std`` of the samplers.
    Without these keys a checkpoint's ``prior`` entry (written by ``train.prior=energy``) is used and printed;
    ``prior=none`` forces N(0, I); value keys that contradict the entry and ``cfg_scale`` with a prior raise ValueError.
    A model must have been trained with the prior it is sampled with.  What the samples sound like has not been
    measured.

    Spectral prior (not in the reference; SpecGrad, Koizumi et al., Interspeech 2022; mel-conditional models, the
    unguided samplers, ``mel_name`` and ``mel_names``, with the clip-seed keys): ``prior=spectral`` with ``prior_ref``
    (required) and ``prior_floor`` (0.01) / ``prior_lifter`` (24) runs from N(0, Sigma) with Sigma shaped per frame and
    bin by ``TacotronSTFT.spectral_filter`` of the conditioning mel at the dataset's STFT keys (the ``prior_filter`` of
    the samplers).  The checkpoint's entry (written by ``train.prior=spectral``), ``prior=none`` and contradicting keys
    behave as above; the editing, partial-start, resampling and guide keys raise ValueError (their noise is not shaped).
    What the samples sound like has not been measured.

    Multi-band runs (not in the reference; ``pqmf.py``): with ``model.subbands = K`` (``model_cfg``; optional
    ``pqmf_taps`` / ``pqmf_cutoff`` / ``pqmf_beta``), or from a checkpoint with a ``pqmf`` entry (written by such a
    training run; used and printed, and the network is then built with its K), the network has K channels, every
    sampler runs on ``[B, K, length / K]`` and ``PQMF.synthesis`` turns the result into the waveform that is written,
    returned and compared by ``report_mel`` / ``report_metrics`` / ``report_pitch``.  With ``mel_names`` the engine's
    per-clip lengths are ``frames x hop_length / K``; the padding of the sub-bands is exactly zero, so an utterance's
    waveform is the synthesis of its own sub-bands (with ``clip_seeds`` an utterance shorter than its batch is another
    draw than alone: the noise of a K-channel state is numbered over the padded length).  Labels, ``cfg_scale``, every ``sampler`` and ``clip_seeds`` work as
    before; the editing, start, resampling and guide keys and ``prior`` are ValueErrors (they act on the full-band
    signal), as are keys that contradict the checkpoint's entry, ``model.subbands`` on a checkpoint without one, and a
    ``ckpt_smooth`` over differing entries.  What the samples sound like has not been measured."""
    from .models import construct_model
    from .models.utils import check_n_classes
    from .sampling import (calc_diffusion_hyperparams, ddim_steps, declip_operator, logsnr_steps, lowpass_operator,
                           mel_operator, program_evaluations, repaint_program, sampling, sampling_aligned, sampling_ddim,
                           sampling_dpmpp, sampling_guided, spans_to_mask)
    from .sampling import clip_seeds as seeds_of_clips
    from scipy.io.wavfile import write as wavwrite

    if ckpt_smooth is not None or ckpt_iter == "init":     # checked here, before a model is built
        weights_key(None, ema, ckpt_smooth)
    from .pqmf import PQMF, model_options

    def check_subbands(cfg):      # a multi-band run (model.subbands, or the checkpoint's pqmf entry), before a model is built
        from .pqmf import check_run
        check_run(cfg, dataset_cfg, where="generate")
        given = [k for k, v in (("known_name", known_name), ("keep", keep), ("start_name", start_name),
                                ("start_griffinlim", start_griffinlim), ("start_step", start_step), ("resample_jump", resample_jump), ("resample_n", resample_n),
                                ("guide_name", guide_name), ("guide_op", guide_op), ("guide_clip", guide_clip),
                                ("guide_factor", guide_factor), ("guide_scale", guide_scale),
                                ("prior", None if prior == "none" else prior)) if v is not None]
        if given:
            raise ValueError(f"generate.{given[0]} does not combine with model.subbands (editing, guidance and the "
                             "adaptive prior act on the full-band signal; their sub-band forms are not built)")
    if model_options(model_cfg) is not None:
        check_subbands(model_cfg)
    prior_cfg = prior_settings(prior, prior_energy_max, prior_energy_min, prior_std_min, model_cfg.get("unconditional"),
                               ref=prior_ref, floor=prior_floor, lifter=prior_lifter,
                               n_fft=dataset_cfg.get("filter_length", 1024))
    prior_given = [k for k, v in zip(PRIOR_KEYS + SPECTRAL_PRIOR_KEYS, (prior_energy_max, prior_energy_min, prior_std_min,
                                                                      prior_ref, prior_floor, prior_lifter)) if v is not None]
    if isinstance(prior_cfg, dict) and cfg_scale is not None:
        raise ValueError(f"generate.cfg_scale does not combine with generate.prior={prior} (classifier-free guidance with an "
                         "adaptive prior is not built)")
    if isinstance(prior_cfg, dict):
        prior_hop(model_cfg, dataset_cfg)
    if isinstance(prior_cfg, dict) and mel_name is None and mel_names is None:
        raise ValueError(f"generate.prior={prior} needs generate.mel_name or generate.mel_names (the conditioning mel)")
    if mel_names is not None:
        mel_names = _check_mel_names(mel_names, mel_name, clip_seeds, seed, known_name=known_name, start_name=start_name,
                                     resample_jump=resample_jump, guide_name=guide_name, guide_op=guide_op, label=label,
                                     cfg_scale=cfg_scale, clips=clips, report_mel=report_mel)
        if model_cfg.get("unconditional"):
            raise ValueError("generate.mel_names needs a mel-conditional model (model.unconditional=false)")
        _check_ragged_hop(model_cfg, dataset_cfg)
        plan = None
    else:
        plan = clip_plan(n_samples, n_samples if batch_size is None else batch_size, rank, num_ranks, clip_seeds, clips, seed)
    # guide_op=mel on a mel-conditional run needs no recording: the measurement is the conditioning mel itself
    guided = guide_name is not None or (guide_op == "mel" and mel_name is not None)
    guide_key = "generate.guide_name" if guide_name is not None else "generate.guide_op=mel"
    if not guided:
        given = [k for k, v in (("guide_op", guide_op), ("guide_clip", guide_clip), ("guide_factor", guide_factor),
                                ("guide_scale", guide_scale)) if v is not None]
        if given:
            raise ValueError(f"generate.{given[0]} needs generate.guide_name (the degraded recording)")
    else:
        if guide_op not in ("declip", "lowpass", "mel"):
            raise ValueError(f"generate.guide_op={guide_op!r}: expected declip, lowpass or mel")
        if guide_scale is None:
            raise ValueError(f"{guide_key} needs generate.guide_scale (the guidance step; no default is chosen: it "
                             "depends on the model and the operator)")
        if float(guide_scale) == 0.0:
            raise ValueError(f"generate.guide_scale=0 is the unguided run: drop {guide_key}")
        if guide_op != "lowpass" and guide_factor is not None:
            raise ValueError("generate.guide_factor belongs to generate.guide_op=lowpass")
        if guide_op != "declip" and guide_clip is not None:
            raise ValueError("generate.guide_clip belongs to generate.guide_op=declip")
        if (sampler or "ddpm") not in ("ddpm", "ddim"):
            raise ValueError(f"{guide_key} with generate.sampler={sampler}: guided runs are built for ddpm and ddim")
        if known_name is not None or start_name is not None or resample_jump is not None or start_griffinlim is not None:
            raise ValueError(f"{guide_key} does not combine with the editing keys (known_name, start_name, "
                             "start_griffinlim, resample_jump)")
    if report_mel is not None:
        if not isinstance(report_mel, bool):
            raise ValueError(f"generate.report_mel={report_mel!r}: expected true or false")
        if report_mel and mel_name is None:
            raise ValueError("generate.report_mel needs a mel-conditional run (generate.mel_name: the error is measured "
                             "against the conditioning mel)")

    if report_metrics is not None:
        if not isinstance(report_metrics, bool):
            raise ValueError(f"generate.report_metrics={report_metrics!r}: expected true or false")
        if report_metrics and (model_cfg.get("unconditional") or (mel_name is None and mel_names is None)):
            raise ValueError("generate.report_metrics needs a mel-conditional run (generate.mel_name or generate.mel_names: "
                             "the clips are compared with the wavs their mels were computed from)")
        if report_metrics and mel_path is not None:
            raise ValueError("generate.report_metrics does not combine with generate.mel_path (pre-computed mel tensors "
                             "have no source wav to compare with)")

    if report_pitch is not None:        # (the preconditions of report_metrics)
        if not isinstance(report_pitch, bool):
            raise ValueError(f"generate.report_pitch={report_pitch!r}: expected true or false")
        if report_pitch and (model_cfg.get("unconditional") or (mel_name is None and mel_names is None)):
            raise ValueError("generate.report_pitch needs a mel-conditional run (generate.mel_name or generate.mel_names: "
                             "the clips are compared with the wavs their mels were computed from)")
        if report_pitch and mel_path is not None:
            raise ValueError("generate.report_pitch does not combine with generate.mel_path (pre-computed mel tensors "
                             "have no source wav to compare with)")

    if report_stoi is not None:         # (the preconditions of report_metrics)
        if not isinstance(report_stoi, bool):
            raise ValueError(f"generate.report_stoi={report_stoi!r}: expected true or false")
        if report_stoi and (model_cfg.get("unconditional") or (mel_name is None and mel_names is None)):
            raise ValueError("generate.report_stoi needs a mel-conditional run (generate.mel_name or generate.mel_names: "
                             "the clips are compared with the wavs their mels were computed from)")
        if report_stoi and mel_path is not None:
            raise ValueError("generate.report_stoi does not combine with generate.mel_path (pre-computed mel tensors "
                             "have no source wav to compare with)")

    source_wavs = {}        # report_metrics / report_pitch / report_stoi: the source wavs read so far
    n_classes = check_n_classes(model_cfg.get("n_classes"))
    labels_of = None        # the class of every sample, cycled
    if label is not None:
        if not n_classes:
            raise ValueError("generate.label needs a class-conditional model (model.n_classes)")
        if isinstance(label, str):
            if label != "all":
                raise ValueError(f"generate.label={label!r}: expected a class index, a list of them, or all")
            labels_of = list(range(n_classes))
        else:
            labels_of = list(label) if isinstance(label, (list, tuple)) else [label]
            if not labels_of or any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= n_classes
                                    for v in labels_of):
                raise ValueError(f"generate.label={label!r}: class indices are integers in 0..{n_classes} "
                                 f"({n_classes} = the null class)")
    if cfg_scale is not None:
        if labels_of is None:
            raise ValueError("generate.cfg_scale needs generate.label (classifier-free guidance steers towards a class)")
        if isinstance(cfg_scale, (bool, str)) or not np.isfinite(float(cfg_scale)):
            raise ValueError(f"generate.cfg_scale={cfg_scale!r}: expected a finite number")
        if guided:
            raise ValueError(f"generate.cfg_scale does not combine with {guide_key} (guided runs take "
                             "generate.label alone)")
        if known_name is not None or start_name is not None or resample_jump is not None or start_griffinlim is not None:
            raise ValueError("generate.cfg_scale does not combine with the editing keys (known_name, start_name, "
                             "start_griffinlim, resample_jump)")
    if known_name is not None and not keep:
        raise ValueError("generate.known_name needs generate.keep: at least one [start, end) span of kept samples")
    if keep and known_name is None:
        raise ValueError("generate.keep needs generate.known_name (the wav whose samples are kept)")
    if start_name is not None and start_step is None:
        raise ValueError("generate.start_name needs generate.start_step (the step the loop starts at)")
    if start_step is not None and start_name is None and start_griffinlim is None:
        raise ValueError("generate.start_step needs generate.start_name (the wav the loop starts from)")
    if start_griffinlim is None and griffinlim_momentum is not None:
        raise ValueError("generate.griffinlim_momentum belongs to generate.start_griffinlim")
    if start_griffinlim is not None:        # the warm start from the conditioning mel itself, before a model is built
        from .mel import check_griffin_lim
        if model_cfg.get("unconditional") or (mel_name is None and mel_names is None):
            raise ValueError("generate.start_griffinlim needs a mel-conditional run (generate.mel_name or "
                             "generate.mel_names: the start is the Griffin-Lim estimate of the conditioning mel)")
        if start_name is not None:
            raise ValueError("generate.start_griffinlim and generate.start_name exclude each other (two starts)")
        if start_step is None:
            raise ValueError("generate.start_griffinlim needs generate.start_step (the step the loop starts at)")
        if mel_path is not None:
            raise ValueError("generate.start_griffinlim does not combine with generate.mel_path (the STFT keys of "
                             "pre-computed mel tensors are unknown)")
        start_griffinlim, griffinlim_momentum = check_griffin_lim(
            start_griffinlim, 0.0 if griffinlim_momentum is None else griffinlim_momentum, "generate.start_griffinlim")
    if (resample_jump is None) != (resample_n is None):
        raise ValueError("generate.resample_jump and generate.resample_n come together (got "
                         f"{'resample_jump' if resample_n is None else 'resample_n'} only)")
    if resample_jump is not None and known_name is None:
        raise ValueError("generate.resample_jump / generate.resample_n need generate.known_name (resampling harmonises "
                         "an inpainting run)")
    sampler = sampler or "ddpm"
    if sampler not in ("ddpm", "aligned", "ddim", "dpmpp2m"):
        raise ValueError(f"generate.sampler={sampler!r}: expected ddpm, aligned, ddim or dpmpp2m")
    if sampler == "aligned" and diffusion_cfg.get("beta") is None:
        raise ValueError("generate.sampler=aligned needs diffusion.beta (the short inference schedule, e.g. "
                         "diffusion.beta=[0.0001,0.001,0.01,0.05,0.2,0.5])")
    if sampler == "ddim" and steps is None:
        raise ValueError("generate.sampler=ddim needs generate.steps (the number of DDIM steps, or a list of them)")
    if sampler == "dpmpp2m":
        if steps is None:
            raise ValueError("generate.sampler=dpmpp2m needs generate.steps (the number of steps, or a list of them)")
        if float(eta or 0.0) != 0.0:
            raise ValueError(f"generate.eta={eta!r} with generate.sampler=dpmpp2m: the solver is deterministic (eta is "
                             "DDIM's)")
        spacing = spacing or "logsnr"
        if spacing not in ("logsnr", "uniform"):
            raise ValueError(f"generate.spacing={spacing!r}: expected logsnr or uniform")
    elif spacing is not None:
        raise ValueError("generate.spacing belongs to generate.sampler=dpmpp2m")
    if rank is not None and torch.cuda.is_available():
        torch.cuda.set_device(rank % torch.cuda.device_count())
    rank = rank or 0
    local_path, output_directory = local_directory(name, model_cfg, diffusion_cfg, dataset_cfg, "waveforms", exp_root)
    dh = calc_diffusion_hyperparams(**diffusion_cfg, fast=True)
    if sampler in ("ddim", "dpmpp2m"):   # these run on the training schedule (the T-step linspace), never on diffusion.beta
        dh_train = calc_diffusion_hyperparams(diffusion_cfg["T"], diffusion_cfg["beta_0"], diffusion_cfg["beta_T"])
        if sampler == "dpmpp2m" and spacing == "logsnr":
            n_evals = len(logsnr_steps(dh_train["Alpha_bar"], steps))
        else:
            n_evals = len(ddim_steps(dh_train["T"], steps))
    else:
        n_evals = dh["T"]
    if resample_jump is not None:       # checked here, before a model is built
        repaint_program(n_evals, resample_jump, resample_n, start_step)
        n_evals = program_evaluations(n_evals, resample_jump, resample_n, start_step)
    model_kwargs = {k: v for k, v in model_cfg.items()}
    net = construct_model(model_kwargs).cuda().eval()
    if precision not in (None, "f32"):
        net.set_option("precision", precision)     # NotImplementedError where the engine has no such kernels for this model

    ckpt_path = os.path.join(exp_root, local_path, "checkpoint")
    prior_entry = None      # what the checkpoint was trained with
    pqmf_cfg = model_options(model_cfg)     # the filter bank of a multi-band run (below: against the checkpoint's entry)

    def bank_of(entries):
        """``pqmf.resolve`` of the run's keys against the checkpoints' ``pqmf`` entries (None: none); a checkpoint
        trained on sub-bands and sampled without ``model.subbands`` has its network rebuilt with the entry's K."""
        from .pqmf import resolve, same_options
        odd = [it for it, e in entries if not same_options(e, entries[0][1])]
        if odd:
            raise ValueError(f"generate.ckpt_smooth: the checkpoints were trained with different filter banks (iteration "
                             f"{entries[0][0]}: {entries[0][1]!r}, iteration {odd[0]}: {dict(entries)[odd[0]]!r})")
        cfg = resolve(model_cfg, entries[0][1])
        if cfg is None or pqmf_cfg is not None:
            return cfg, net
        full = dict(model_kwargs, subbands=cfg["subbands"], pqmf_taps=cfg["taps"], pqmf_cutoff=cfg["cutoff"],
                    pqmf_beta=cfg["beta"])
        check_subbands(full)
        rebuilt = construct_model(full).cuda().eval()
        if precision not in (None, "f32"):
            rebuilt.set_option("precision", precision)
        return cfg, rebuilt
    if ckpt_iter == "init":
        ckpt_iter = 0
    else:
        if ckpt_iter == "max":
            ckpt_iter = find_max_epoch(ckpt_path)
        ckpt_iter = int(ckpt_iter)
        if ckpt_smooth is None:
            model_file = os.path.join(ckpt_path, f"{ckpt_iter}.pkl")
            try:
                checkpoint = torch.load(model_file, map_location="cpu")
            except Exception as e:  # the reference raises a bare 'No valid model found' (`generate.py:110-112`)
                raise Exception(f"No valid model found ({model_file}: {e})")
            key = weights_key(checkpoint, ema)
            pqmf_cfg, net = bank_of([(ckpt_iter, checkpoint.get("pqmf"))])
            try:
                net.load_state_dict(checkpoint[key])
            except Exception as e:
                raise Exception(f"No valid model found ({model_file}: {e})")
            if key == "ema_state_dict":
                print(f"sampling from the EMA weights of iteration {ckpt_iter} (generate.ema=false: the raw weights)")
            prior_entry = checkpoint.get("prior")
        else:                       # `generate.py:113-115`: average of the checkpoints in (ckpt_smooth, ckpt_iter]
            entries, banks = [], []
            state_dict = smooth_ckpt(ckpt_path, int(ckpt_smooth), ckpt_iter, priors=entries, banks=banks)
            if state_dict is None:
                raise Exception(f"No checkpoints in ({ckpt_smooth}, {ckpt_iter}] under {ckpt_path}")
            odd = [it for it, e in entries if not same_prior(e, entries[0][1])]
            if odd:     # weights trained towards different priors have no common one to be sampled from
                raise ValueError(f"generate.ckpt_smooth: the checkpoints in ({ckpt_smooth}, {ckpt_iter}] were trained with "
                                 f"different priors (iteration {entries[0][0]}: {entries[0][1]!r}, iteration {odd[0]}: "
                                 f"{dict(entries)[odd[0]]!r})")
            prior_entry = entries[0][1]
            pqmf_cfg, net = bank_of(banks)
            net.load_state_dict(state_dict)
    bank, K = None, 1       # multi-band runs: the samplers return K sub-bands at a K-th of the length
    if pqmf_cfg is not None:
        bank, K = PQMF(**pqmf_cfg), pqmf_cfg["subbands"]
        print("multi-band run{}: subbands={subbands} taps={taps} cutoff={cutoff:g} beta={beta:g}".format(
            " (the checkpoint's pqmf entry)" if model_cfg.get("subbands") is None else "", **pqmf_cfg))
        if prior_entry is not None:
            raise ValueError("the checkpoint holds a prior entry and a pqmf entry: the adaptive prior in sub-bands is not "
                             "built")
    prior_cfg = resolve_prior(prior_cfg, prior_entry, prior_given)
    if prior_cfg is not None:
        if cfg_scale is not None:
            raise ValueError("generate.cfg_scale does not combine with the adaptive prior of the checkpoint "
                             "(generate.prior=none samples from N(0, I))")
        hop_of_prior = prior_hop(model_cfg, dataset_cfg)
        if prior_cfg["kind"] == "spectral":
            given = [k for k, v in (("known_name", known_name), ("start_name", start_name),
                                    ("start_griffinlim", start_griffinlim), ("resample_jump", resample_jump)) if v is not None]
            if guided:
                given.append(guide_key[len("generate."):])
            if given:
                raise ValueError(f"generate.{given[0]} does not combine with the spectral prior (editing, partial starts, "
                                 "resampling and guidance draw noise the prior does not shape; generate.prior=none "
                                 "samples from N(0, I))")
            from .mel import TacotronSTFT
            keys = ("filter_length", "hop_length", "win_length", "sampling_rate", "mel_fmin", "mel_fmax")
            prior_stft = TacotronSTFT(**{k: dataset_cfg[k] for k in keys if k in dataset_cfg})
            print("spectral prior{}: ref={ref:g} floor={floor:g} lifter={lifter}".format(
                " (the checkpoint's prior entry)" if prior is None else "", **prior_cfg))
        else:
            print("adaptive prior{}: energy_max={energy_max:g} energy_min={energy_min:g} std_min={std_min:g}".format(
                " (the checkpoint's prior entry)" if prior is None else "", **prior_cfg))

    def sigma_of(mel, L, frame_counts=None):
        """The prior's sampler arguments of a conditioning mel [B, bands, frames], or nothing: the standard deviation
        [B, 1, L] (energy), or the filter [B, K, L // hop + 1] and its STFT (spectral; clip b's last own frame, of its
        ``frame_counts[b]``, is repeated once: a run of frames x hop samples has one frame more than its mel)."""
        if prior_cfg is None or mel is None:
            return {}
        if prior_cfg["kind"] == "spectral":
            filt = prior_stft.spectral_filter(mel.to(device="cuda", dtype=torch.float32), L,
                                              **{k: prior_cfg[k] for k in SPECTRAL_PRIOR_KEYS})
            for b, f in enumerate(frame_counts or ()):
                filt[b, :, f] = filt[b, :, f - 1]
            return {"prior_filter": filt, "prior_stft": prior_stft}
        from .mel import prior_std_from_mel
        return {"prior_std": prior_std_from_mel(mel.to(device="cuda", dtype=torch.float32), hop_of_prior, L,
                                                **{k: prior_cfg[k] for k in PRIOR_KEYS})}

    def griffinlim_start(mel, frame_counts, lens=None):
        """The partial-start arguments of generate.start_griffinlim: ``x_start`` [B, 1, frames x hop] is ``mel_to_audio``
        of the conditioning mel [B, bands, F] at the run's STFT keys.  A run of frames x hop samples has one frame more
        than its mel: every clip's last frame (of its own ``frame_counts[b]``) is repeated once."""
        from .mel import Mel2Samp
        keys = ("filter_length", "hop_length", "win_length", "sampling_rate", "mel_fmin", "mel_fmax")
        stft = Mel2Samp(**{k: dataset_cfg[k] for k in keys if k in dataset_cfg}).stft
        mel = mel.detach().to(device="cuda", dtype=torch.float32)
        ext = torch.cat([mel, mel[..., -1:]], dim=-1)
        for b, f in enumerate(frame_counts):
            ext[b, :, f] = mel[b, :, f - 1]
        x0 = stft.mel_to_audio(ext, n_iters=start_griffinlim, momentum=griffinlim_momentum, lengths=lens)
        print(f"start: Griffin-Lim estimate of the conditioning mel ({start_griffinlim} iterations, momentum "
              f"{griffinlim_momentum:g}), the loop starts at step {start_step}")
        return dict(x_start=x0[:, None, :], start_step=start_step, start_noise=None if start_noise else False)

    output_directory = os.path.join(output_directory, str(ckpt_iter))
    os.makedirs(output_directory, mode=0o775, exist_ok=True)

    if mel_names is not None:
        # ---- ragged batches: every utterance once, batches of the plan at their own L_max with per-clip lengths
        hop = dataset_cfg["hop_length"]
        mels = []
        for stem in mel_names:
            if mel_path is not None:
                try:
                    mels.append(torch.load(os.path.join(mel_path, f"{stem}.wav.pt")).to(torch.float32).cuda())
                except Exception:
                    raise Exception(f"No ground truth mel spectrogram found ({stem})")
            else:
                from .mel import Mel2Samp, load_wav_to_torch
                keys = ("filter_length", "hop_length", "win_length", "sampling_rate", "mel_fmin", "mel_fmax")
                _mel = Mel2Samp(**{k: dataset_cfg[k] for k in keys if k in dataset_cfg})
                audio, sr = load_wav_to_torch(os.path.join(str(dataset_cfg["data_path"]), f"{stem}.wav"))
                mels.append(_mel.get_mel(audio).to(torch.float32).cuda())
                if report_pitch:        # refused here, before the first batch is sampled
                    _check_pitch_source(stem, min(int(audio.shape[0]), int(mels[-1].shape[-1]) * hop), dataset_cfg)
                if report_stoi:
                    _check_stoi_source(stem, min(int(audio.shape[0]), int(mels[-1].shape[-1]) * hop), dataset_cfg)
        frames = [int(m.shape[-1]) for m in mels]
        batches = ragged_plan(frames, len(mel_names) if batch_size is None else batch_size)
        clips_out = [None] * len(mel_names)
        t0 = time.perf_counter()
        for i, batch in list(enumerate(batches))[rank % max(int(num_ranks or 1), 1)::max(int(num_ranks or 1), 1)]:
            lens = [frames[k] * hop for k in batch]
            Tmax, Lmax = frames[batch[0]], lens[0]
            mel = torch.zeros(len(batch), mels[0].shape[0], Tmax, device="cuda", dtype=torch.float32)
            for b, k in enumerate(batch):
                mel[b, :, :frames[k]] = mels[k]
            size = (len(batch), K, Lmax // K)
            s = [seeds_of_clips(seed, k, 1)[0] for k in batch] if clip_seeds else (None if seed is None else seed + i)
            print(f"batch {i}: L_max = {Lmax}, lengths = {lens}, padded share = "
                  f"{1.0 - sum(lens) / float(len(batch) * Lmax):.3f}")
            pr = sigma_of(mel, Lmax, [frames[k] for k in batch])     # (each frame on its own: a clip's sigma is what it is alone; its padding is unused)
            run_lens = lens if bank is None else [n // K for n in lens]      # what the engine runs: sub-band positions
            if start_griffinlim is not None:
                pr = dict(pr, **griffinlim_start(mel, [frames[k] for k in batch], lens))
            if sampler == "aligned":
                x = sampling_aligned(net, size, diffusion_cfg, condition=mel, seed=s, lengths=run_lens, **pr)
            elif sampler == "ddim":
                x = sampling_ddim(net, size, dh_train, steps, eta=float(eta or 0.0), condition=mel, seed=s, lengths=run_lens,
                                  **pr)
            elif sampler == "dpmpp2m":
                x = sampling_dpmpp(net, size, dh_train, steps, condition=mel, spacing=spacing, seed=s, lengths=run_lens, **pr)
            else:
                x = sampling(net, size, dh, condition=mel, seed=s, lengths=run_lens, **pr)
            if bank is not None:        # the sub-band padding is exactly zero: a clip's synthesis is what it is alone
                x = bank.synthesis(x)
            for b, k in enumerate(batch):
                clips_out[k] = x[b, :, :lens[b]].clone()
            if report_metrics:
                _report_metrics(i, x, [mel_names[k] for k in batch], batch, lens, dataset_cfg, metric_rows, source_wavs)
            if report_pitch:
                _report_pitch(i, x, [mel_names[k] for k in batch], batch, lens, dataset_cfg, metric_rows,
                              bool(report_metrics), source_wavs)
            if report_stoi:
                _report_stoi(i, x, [mel_names[k] for k in batch], batch, lens, dataset_cfg, metric_rows,
                             bool(report_metrics or report_pitch), source_wavs)
        torch.cuda.synchronize()
        made = [k for k, c in enumerate(clips_out) if c is not None]
        print(f"generated {len(made)} utterances of {len(mel_names)} at iteration {ckpt_iter} in "
              f"{time.perf_counter() - t0:.1f} seconds ({n_evals} network evaluations per batch)")
        for k in made:
            outfile = os.path.join(output_directory, "{}k_{}.wav".format(ckpt_iter // 1000, mel_names[k]))
            wavwrite(outfile, dataset_cfg["sampling_rate"], clips_out[k].squeeze(0).cpu().numpy().astype(np.float32))
            if written is not None:
                written.append(outfile)
        return clips_out

    if batch_size is None:
        batch_size = n_samples
    assert plan is not None or n_samples % batch_size == 0
    if mel_name is not None:
        if mel_path is not None:      # pre-generated spectrogram (`generate.py:135-141`)
            try:
                mel = torch.load(os.path.join(mel_path, f"{mel_name}.wav.pt")).unsqueeze(0).cuda()
            except Exception:
                raise Exception("No ground truth mel spectrogram found")
        else:                         # from the waveform (`generate.py:142-153`)
            from .mel import Mel2Samp, load_wav_to_torch
            keys = ("filter_length", "hop_length", "win_length", "sampling_rate", "mel_fmin", "mel_fmax")
            _mel = Mel2Samp(**{k: dataset_cfg[k] for k in keys if k in dataset_cfg})
            audio, sr = load_wav_to_torch(os.path.join(str(dataset_cfg["data_path"]), f"{mel_name}.wav"))
            mel = _mel.get_mel(audio).unsqueeze(0)
            if report_pitch:          # refused here, before anything is sampled
                _check_pitch_source(mel_name, min(int(audio.shape[0]), int(mel.shape[-1]) * dataset_cfg["hop_length"]),
                                    dataset_cfg)
            if report_stoi:
                _check_stoi_source(mel_name, min(int(audio.shape[0]), int(mel.shape[-1]) * dataset_cfg["hop_length"]),
                                   dataset_cfg)
        audio_length = mel.shape[-1] * dataset_cfg["hop_length"]
    else:
        audio_length, mel = dataset_cfg["segment_length"], None
    edit = {}
    if known_name is not None:
        edit["known"] = _load_clip(dataset_cfg, known_name, audio_length, mel is not None)
        edit["mask"] = spans_to_mask((batch_size, 1, audio_length), keep)
    if start_name is not None:
        edit["x_start"] = _load_clip(dataset_cfg, start_name, audio_length, mel is not None)
        edit["start_step"] = start_step
        edit["start_noise"] = None if start_noise else False
    if start_griffinlim is not None:
        edit.update(griffinlim_start(mel, [int(mel.shape[-1])]))
    if resample_jump is not None:
        edit["resample"] = (resample_jump, resample_n)
    mel_of = None       # log-mel of a [B, 1, L] batch on the engine, cut to the frames of the conditioning mel
    if guide_op == "mel" or report_mel:
        sr = dataset_cfg["sampling_rate"]
        stft_kw = dict(filter_length=1024, hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=min(8000.0, sr / 2.0))
        stft_kw.update({k: dataset_cfg[k] for k in stft_kw if k in dataset_cfg})
        mel_A = mel_operator(sampling_rate=sr, n_mel_channels=80, **stft_kw)
        # a run of mel frames x hop samples has one frame more than its conditioning mel: the last one is not compared
        mel_of = mel_A if mel is None else (lambda x: mel_A(x)[..., :mel.shape[-1]])
    guide = None
    if guide_name is None and guided:
        guide = dict(measurement=mel.detach().to(torch.float32).expand(batch_size, -1, -1), operator=mel_of,
                     scale=float(guide_scale))
    elif guided:
        rec = _load_clip(dataset_cfg, guide_name, audio_length, mel is not None).expand(batch_size, 1, audio_length)
        if guide_op == "mel":
            guide = dict(measurement=mel_of(rec[:1].cuda()).expand(batch_size, -1, -1), operator=mel_of,
                         scale=float(guide_scale))
        elif guide_op == "declip":
            op = declip_operator(float(rec.abs().max()) if guide_clip is None else guide_clip)
            guide = dict(measurement=rec, operator=op, scale=float(guide_scale))
        else:
            op = lowpass_operator(2 if guide_factor is None else guide_factor)
            guide = dict(measurement=op(rec), operator=op, scale=float(guide_scale))

    prior_one = sigma_of(mel, audio_length)     # [1, 1, L]: every clip of a batch shares the mel
    t0 = time.perf_counter()
    out = []
    # the global clip numbers of every batch: the plan of generate.clip_seeds, or this rank's n_samples in order
    batches = plan if plan is not None else [[n_samples * rank + i * batch_size + b for b in range(batch_size)]
                                             for i in range(n_samples // batch_size)]
    numbers = [k for batch in batches for k in batch]
    for i, batch in enumerate(batches):
        size = (len(batch), K, audio_length // K)
        if plan is not None:    # a seed and a class per clip, both functions of the global clip number alone
            s = [seeds_of_clips(seed, k, 1)[0] for k in batch]
            class_of = [k % len(labels_of) for k in batch] if labels_of is not None else None
        else:
            s = None if seed is None else seed + 1000 * rank + i
            class_of = [(i * batch_size + b) % len(labels_of) for b in range(batch_size)] if labels_of is not None else None
        if labels_of is not None:
            edit["labels"] = [labels_of[c] for c in class_of]
            if cfg_scale is not None:
                edit["cfg_scale"] = float(cfg_scale)
        if "prior_std" in prior_one:
            edit["prior_std"] = prior_one["prior_std"].expand(len(batch), 1, audio_length)
        elif prior_one:
            edit.update(prior_one, prior_filter=prior_one["prior_filter"].expand(len(batch), -1, -1))
        if guide is not None:
            ddim = sampler == "ddim"
            guide_b = dict(guide, measurement=guide["measurement"][:len(batch)])
            out.append(sampling_guided(net, size, dh_train if ddim else dh, sampler=sampler, steps=steps if ddim else None,
                                       eta=float(eta or 0.0) if ddim else 0.0, condition=mel, seed=s,
                                       labels=edit.get("labels"), prior_std=edit.get("prior_std"), **guide_b))
        elif sampler == "aligned":
            out.append(sampling_aligned(net, size, diffusion_cfg, condition=mel, seed=s, **edit))
        elif sampler == "ddim":
            out.append(sampling_ddim(net, size, dh_train, steps, eta=float(eta or 0.0), condition=mel, seed=s, **edit))
        elif sampler == "dpmpp2m":
            out.append(sampling_dpmpp(net, size, dh_train, steps, condition=mel, spacing=spacing, seed=s, **edit))
        else:
            out.append(sampling(net, size, dh, condition=mel, seed=s, **edit))
        if bank is not None:        # the samplers return the K sub-bands: one synthesis bank at the end of the run
            out[-1] = bank.synthesis(out[-1])
        if report_mel:
            err = float((mel_of(out[-1]) - mel).abs().mean())
            print(f"batch {i} mel error: mean |log-mel(generated) - condition| = {err:.4f}")
            if mel_errors is not None:
                mel_errors.append(err)
        if report_metrics:
            _report_metrics(i, out[-1], [mel_name] * len(batch), batch, [audio_length] * len(batch), dataset_cfg,
                            metric_rows, source_wavs)
        if report_pitch:
            _report_pitch(i, out[-1], [mel_name] * len(batch), batch, [audio_length] * len(batch), dataset_cfg,
                          metric_rows, bool(report_metrics), source_wavs)
        if report_stoi:
            _report_stoi(i, out[-1], [mel_name] * len(batch), batch, [audio_length] * len(batch), dataset_cfg,
                         metric_rows, bool(report_metrics or report_pitch), source_wavs)
    generated_audio = torch.cat(out, dim=0) if out else torch.empty(0, 1, audio_length, device="cuda")
    torch.cuda.synchronize()
    print(f"generated {len(numbers)} samples shape {tuple(generated_audio.shape)} at iteration {ckpt_iter} in "
          f"{time.perf_counter() - t0:.1f} seconds")
    if guide is not None:
        print(f"guided sampler {sampler} ({guide_op}, scale {float(guide_scale):g}): {n_evals} network evaluations "
              f"(each a forward and a data-only backward) per batch")
    elif sampler != "ddpm" or resample_jump is not None:
        note = f" (eta={float(eta or 0.0)})" if sampler == "ddim" else f" ({spacing} spacing)" if sampler == "dpmpp2m" else ""
        print(f"sampler {sampler}{note}: {n_evals} network evaluations per batch")
    for i, k in enumerate(numbers):
        outfile = "{}k_{}.wav".format(ckpt_iter // 1000, k)   # `generate.py:189`: k = n_samples * rank + i
        if labels_of is not None:
            outfile = outfile[:-4] + f"_c{labels_of[(k if plan is not None else i) % len(labels_of)]}.wav"
        wavwrite(os.path.join(output_directory, outfile), dataset_cfg["sampling_rate"],
                 generated_audio[i].squeeze().cpu().numpy().astype(np.float32))
        if written is not None:
            written.append(os.path.join(output_directory, outfile))
    return generated_audio


def _worker(rank, cfg, exp_root):
    gen = dict(cfg.get("generate", {}))
    gen.setdefault("precision", (cfg.get("engine") or {}).get("precision"))
    gen.setdefault("num_ranks", max(torch.cuda.device_count(), 1))     # main() starts one process per GPU
    generate(rank, dict(cfg["diffusion"]), dict(cfg["model"]), dict(cfg["dataset"]), exp_root=exp_root, **gen)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config-dir", required=True, help="Hydra-style config tree (the reference's configs/)")
    ap.add_argument("--exp-root", default="exp")
    ap.add_argument("overrides", nargs="*", help="key=value overrides, e.g. experiment=sc09 model=wavenet")
    args = ap.parse_args(argv)
    cfg = load_config(args.config_dir, args.overrides)
    num_gpus = torch.cuda.device_count()
    if num_gpus <= 1:
        _worker(0, cfg, args.exp_root)
    else:  # one process per GPU, no communication (`generate.py:217-227`)
        import torch.multiprocessing as mp
        mp.spawn(_worker, args=(cfg, args.exp_root), nprocs=num_gpus, join=True)


if __name__ == "__main__":
    main(sys.argv[1:])

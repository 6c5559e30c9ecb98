"""``train.py``-compatible driver on the HIP engine.

Same call surface and on-disk conventions as the reference (``train.py:27-196,224-252``): Hydra-style
config tree + ``key=value`` overrides, ``exp/<run>/checkpoint/<iter>.pkl`` holding
``{'model_state_dict', 'optimizer_state_dict'}``, resume from ``train.ckpt_iter`` (``max`` = newest),
Adam at ``train.learning_rate``, one process per GPU with ``apply_gradient_allreduce`` (RCCL), rank-0
checkpoints followed by an in-loop ``generate`` call.  wandb is replaced by a JSON-lines log
(``exp/<run>/train_log.jsonl``, same keys: ``train/loss``, ``train/log_loss``, ``train/loss_epoch``).  With
``+generate.report_metrics=true`` the in-loop ``generate`` compares its clips with their source wavs and the log gets
``val/mr_stft``, ``val/ls_mae``, ``val/lsd`` and ``val/mcd`` at that iteration (``metrics.py``); with
``+generate.report_pitch=true`` it gets ``val/f0_rmse``, ``val/f0_cents``, ``val/gpe``, ``val/vuv_error``, ``val/vuv_f1``
and ``val/periodicity_rmse`` (``metrics.pitch_metrics``; means over the clips on which a key is defined, a key that is
defined on none is left out); with ``+generate.report_stoi=true`` ``val/stoi`` and ``val/estoi`` (``metrics.stoi``, the
same rule).

    python -m diffwave_sashimi_amd.train --config-dir /path/to/configs experiment=sc09 model=sashimi \
        dataset.data_path=/data/sc09 train.batch_size_per_gpu=32

Datasets: ``sc09`` (a directory tree of 1 s / 16 kHz ``*_nohash_*.wav`` files, ``dataloaders/sc.py:25-64``),
``ljspeech`` (``dataloaders/mel2samp.py:59-113``: random ``segment_length`` crops of the wavs under ``data_path``;
the log-mel of each batch is computed on the GPU by ``dws_mel_spectrogram`` right before the step instead of per
item on the loader's CPU workers) and ``synthetic`` (uniform noise clips, for smoke runs).
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

from .generate import (PRIOR_KEYS, SPECTRAL_PRIOR_KEYS, find_max_epoch, generate, load_config, local_directory, prior_hop, prior_settings,
                       same_prior)

HASH_DIVIDER, EXCEPT_FOLDER = "_nohash_", "_background_noise_"   # `dataloaders/sc.py:15-16`


def fix_length(t, length):
    """``dataloaders/sc.py:25-32``: crop or zero-pad a [1, n] waveform to ``length``."""
    assert t.dim() == 2 and t.shape[0] == 1
    if t.shape[1] > length:
        return t[:, :length]
    if t.shape[1] < length:
        return torch.cat([t, torch.zeros(1, length - t.shape[1])], dim=1)
    return t


class SpeechCommands(torch.utils.data.Dataset):
    """``dataloaders/sc.py:46-64``: items are ``(waveform[1,16000] in [-1,1), sample_rate, label)``.

    ``classes``: the sorted names of the sub-folders that hold clips (SC09: ``eight .. zero``).  With
    ``label_index=True`` (class-conditional training) the label of an item is its index in ``classes`` instead of
    the folder name."""

    def __init__(self, path, length=16000, label_index=False):
        self._path, self._length, self._label_index = path, length, label_index
        walker = sorted(str(p) for p in Path(path).glob("**/*.wav"))
        self._walker = [w for w in walker if HASH_DIVIDER in w and EXCEPT_FOLDER not in w]
        self.classes = sorted({os.path.split(os.path.relpath(w, path))[0] for w in self._walker})

    def __getitem__(self, n):
        from scipy.io import wavfile
        f = self._walker[n]
        label = os.path.split(os.path.relpath(f, self._path))[0]
        sr, x = wavfile.read(f)
        if x.dtype == np.int16:            # torchaudio.load(normalize=True) semantics
            x = x.astype(np.float32) / 32768.0
        elif x.dtype == np.int32:
            x = x.astype(np.float32) / 2147483648.0
        else:
            x = x.astype(np.float32)
        if x.ndim == 2:
            x = x[:, 0]
        if self._label_index:
            label = self.classes.index(label)
        return fix_length(torch.from_numpy(x).unsqueeze(0), self._length), sr, label

    def __len__(self):
        return len(self._walker)


class LJSegments(torch.utils.data.Dataset):
    """The audio half of ``Mel2Samp`` (``dataloaders/mel2samp.py:59-113``): wavs found under ``data_path``
    (`files_to_list`, shuffled with ``random.seed(1234)``), sampling-rate check, a random ``segment_length`` crop
    (zero-padded when shorter); items are the raw-scale float waveform ``[segment_length]``."""

    def __init__(self, data_path, segment_length, sampling_rate, valid=False, **_ignored):
        import random
        self.audio_files = sorted(str(p) for p in Path(data_path).glob("**/*.wav"))
        random.seed(1234)
        random.shuffle(self.audio_files)
        self.segment_length, self.sampling_rate, self.valid = segment_length, sampling_rate, valid

    def __getitem__(self, index):
        import random
        from .mel import load_wav_to_torch
        audio, sr = load_wav_to_torch(self.audio_files[index])
        if sr != self.sampling_rate:
            raise ValueError("{} SR doesn't match target {} SR".format(sr, self.sampling_rate))
        if not self.valid:
            if audio.size(0) >= self.segment_length:
                start = random.randint(0, audio.size(0) - self.segment_length)
                audio = audio[start:start + self.segment_length]
            else:
                audio = torch.nn.functional.pad(audio, (0, self.segment_length - audio.size(0)), "constant").data
        return audio

    def __len__(self):
        return len(self.audio_files)


class SyntheticClips(torch.utils.data.Dataset):
    """U(-0.3, 0.3) clips (SURVEY.md 8d's synthetic workload) with the sc09 item layout.  ``n_classes = K``
    (class-conditional smoke runs): item n carries the label ``n % K``."""

    def __init__(self, n_items, length, sampling_rate=16000, seed=0, n_classes=0):
        self.n, self.length, self.sr, self.seed, self.n_classes = n_items, length, sampling_rate, seed, n_classes

    def __getitem__(self, n):
        g = torch.Generator().manual_seed(self.seed * 1000003 + n)
        label = n % self.n_classes if self.n_classes else "synthetic"
        return (torch.rand(1, self.length, generator=g) * 2 - 1) * 0.3, self.sr, label

    def __len__(self):
        return self.n


def dataloader(dataset_cfg, batch_size, num_gpus, unconditional=True, rank=0, num_workers=4, n_classes=0):
    """``dataloaders/__init__.py:6-33``.  ``n_classes`` (a class-conditional model's ``model.n_classes``): items carry
    the class index; sc09's folder count must match, ``ljspeech`` has no classes."""
    name = dataset_cfg.get("_name_", "sc09")
    n_classes = int(n_classes or 0)
    if name == "sc09":
        assert unconditional
        dataset = SpeechCommands(dataset_cfg["data_path"], dataset_cfg.get("segment_length", 16000),
                                 label_index=n_classes > 0)
        if n_classes and len(dataset.classes) != n_classes:
            raise ValueError(f"model.n_classes = {n_classes}, but {dataset_cfg['data_path']} holds {len(dataset.classes)} "
                             f"class folders ({', '.join(dataset.classes)})")
    elif name == "synthetic":
        dataset = SyntheticClips(dataset_cfg.get("n_items", 64), dataset_cfg.get("segment_length", 16000),
                                 dataset_cfg.get("sampling_rate", 16000), n_classes=n_classes)
    elif name == "ljspeech":
        if n_classes:
            raise ValueError("model.n_classes with dataset ljspeech: the dataset has no class labels")
        assert not unconditional
        dataset = LJSegments(**{k: v for k, v in dataset_cfg.items() if k != "_name_"})
    else:
        raise NotImplementedError(f"dataset '{name}' is not built (sc09, ljspeech, synthetic are)")
    sampler = None
    if num_gpus > 1:
        from torch.utils.data.distributed import DistributedSampler
        sampler = DistributedSampler(dataset, num_replicas=num_gpus, rank=rank)
    return torch.utils.data.DataLoader(dataset, batch_size=batch_size, sampler=sampler, shuffle=False,
                                       num_workers=num_workers, pin_memory=False, drop_last=True)


def optim_param_groups(net, honour_hints=False):
    """What the optimizer is built from.  Default: `net.parameters()`, i.e. ONE group -- the reference's `train.py:91` (and its
    checkpoints' `optimizer_state_dict`, `:104-107,159`).  `honour_hints=True` (`+train.honour_optim_hints=true`): the S4 kernel
    parameters carry `_optim = {"weight_decay": 0.0[, "lr": ...]}` (`models/s4.py:508-518`), and every distinct hint becomes its
    own parameter group after the plain one, the way the S4 authors' own training harness consumes them.  Under the reference's
    Adam (no weight decay) and SaShiMi's lr=None construction the update is the same; the group layout differs, so such a run's
    optimizer state does not load into a one-group run and vice versa."""
    params = list(net.parameters())
    if not honour_hints:
        return params
    plain = [p for p in params if not getattr(p, "_optim", None)]
    groups = [{"params": plain}]
    keys = []
    for p in params:
        h = getattr(p, "_optim", None)
        if not h:
            continue
        k = tuple(sorted(h.items()))
        if k not in keys:
            keys.append(k)
            groups.append({"params": [], **dict(k)})
        groups[1 + keys.index(k)]["params"].append(p)
    return groups


def optimizer_options(optimizer=None, ema_decay=None, clip_grad_norm=None):
    """The optimizer keys of the ``train`` group, checked (before any model is built): ``train.optimizer`` = ``torch``
    (default: ``torch.optim.Adam``, the reference's) or ``engine`` (``optim.EngineAdam``, the fused HIP step);
    ``train.ema_decay`` = D with 0 < D < 1 and ``train.clip_grad_norm`` = C > 0 both need ``optimizer=engine``.
    Returns ``(kind, ema_decay or None, clip_grad_norm or None)``."""
    kind = "torch" if optimizer is None else optimizer
    if kind not in ("torch", "engine"):
        raise ValueError(f"train.optimizer={optimizer!r}: expected engine or torch")

    def number(key, v):
        if isinstance(v, (bool, str)) or not isinstance(v, (int, float)) or not np.isfinite(float(v)):
            raise ValueError(f"train.{key}={v!r}: expected a number")
        return float(v)
    if ema_decay is not None:
        ema_decay = number("ema_decay", ema_decay)
        if not 0.0 < ema_decay < 1.0:
            raise ValueError(f"train.ema_decay={ema_decay!r} (needs 0 < D < 1)")
        if kind != "engine":
            raise ValueError("train.ema_decay needs train.optimizer=engine (the EMA is part of the fused step)")
    if clip_grad_norm is not None:
        clip_grad_norm = number("clip_grad_norm", clip_grad_norm)
        if not clip_grad_norm > 0.0:
            raise ValueError(f"train.clip_grad_norm={clip_grad_norm!r} (needs C > 0)")
        if kind != "engine":
            raise ValueError("train.clip_grad_norm needs train.optimizer=engine (the clipping is part of the fused step)")
    return kind, ema_decay, clip_grad_norm


class PriorMismatch(ValueError):
    """A resume whose ``train.prior`` keys differ from the checkpoint's ``prior`` entry."""


class PqmfMismatch(ValueError):
    """A resume whose ``model.subbands`` / ``model.pqmf_*`` keys differ from the checkpoint's ``pqmf`` entry."""


def train(rank, num_gpus, diffusion_cfg, model_cfg, dataset_cfg, generate_cfg, ckpt_iter, n_iters, iters_per_ckpt,
          iters_per_logging, learning_rate, batch_size_per_gpu, name=None, exp_root="exp", num_workers=4, precision=None,
          honour_optim_hints=False, label_dropout=None, optimizer=None, ema_decay=None, clip_grad_norm=None, prior=None,
          prior_energy_max=None, prior_energy_min=None, prior_std_min=None, stft_weight=None, stft_max_step=None,
          stft_resolutions=None, prior_ref=None, prior_floor=None, prior_lifter=None):
    """``train.py:49-196``.  With ``model.n_classes`` (class-conditional; not in the reference) every batch's class
    indices go to the network and ``label_dropout`` (``train.label_dropout``, default 0.1) of them are replaced by the
    null class, which is what classifier-free guidance needs at sampling time; the in-loop ``generate`` cycles the
    classes.

    ``optimizer`` / ``ema_decay`` / ``clip_grad_norm`` (``+train.optimizer=engine +train.ema_decay=0.9999
    +train.clip_grad_norm=1.0``; not in the reference): see ``optimizer_options``.  With an EMA the checkpoints also hold
    ``ema_state_dict`` (the averaged weights in the layout of ``model_state_dict``), which ``generate`` then samples
    from; a resume restores it, or starts it from the loaded weights when the checkpoint has none.

    ``prior`` (``+train.prior=energy +train.prior_energy_max=E [+train.prior_energy_min=0 +train.prior_std_min=0.1]``; not
    in the reference; mel-conditional models): the adaptive prior of PriorGrad (Lee et al., ICLR 2022).  Every batch is
    noised towards N(0, diag(sigma^2)) with sigma = ``mel.prior_std_from_mel`` of its own mel segment and trained on the
    Sigma^-1-weighted loss (``training_loss(prior_std=)``); the checkpoints get a ``prior`` entry with the four values,
    which ``generate`` -- the in-loop one too -- picks up.  A resume must name the prior the checkpoint was trained with
    (none for a checkpoint without an entry): anything else raises ``PriorMismatch`` (a ValueError).  What such a model
    sounds like has not been measured.

    ``prior=spectral`` (``+train.prior=spectral +train.prior_ref=R [+train.prior_floor=0.01 +train.prior_lifter=24]``; not
    in the reference; mel-conditional models, one audio channel): the time-varying spectral prior of SpecGrad (Koizumi et
    al., Interspeech 2022).  Every batch is noised with ``eps = T_F(z)``, F = ``TacotronSTFT.spectral_filter`` of its own
    mel segment at the dataset's STFT keys, and trained on ``mean(T_{1/F}(eps_theta - eps)^2)``
    (``training_loss(prior_filter=)``; ``dws_tv_filter``).  The checkpoints' ``prior`` entry is then
    ``{"kind": "spectral", "ref", "floor", "lifter"}``; ``generate`` and a resume treat it as above (an energy entry and
    a spectral entry never match).  What such a model sounds like has not been measured.

    ``stft_weight`` (``+train.stft_weight=W [+train.stft_max_step=K] [+train.stft_resolutions=[[n_fft,hop,win],...]]``;
    not in the reference; one audio channel): adds W times Parallel WaveGAN's multi-resolution STFT loss of the denoised
    estimate x0_hat against the clean audio, on the clips whose step is below K (``training_loss(stft_weight=)``).
    ``train/eps_loss`` and ``train/stft_loss`` join ``train/loss`` in the log; the checkpoints get a ``stft_loss`` entry
    with the three values, which a resume prints (it is information, not a condition: a run may change or drop the
    term).  The term is local to a rank.  What it does for audio quality has not been measured.

    Multi-band runs (``+model.subbands=K [+model.pqmf_taps=62 +model.pqmf_cutoff=C +model.pqmf_beta=9.0]``, K = 2 or 4;
    not in the reference; ``pqmf.py``): the network is built with K channels and trained on the PQMF sub-bands of every
    batch (``training_loss(pqmf=)``), a K-th of the positions per evaluation.  On a mel-conditional model
    ``prod(model.mel_upsample) x K`` must be ``dataset.hop_length``; ``dataset.segment_length`` must be a multiple of K
    (and, on SaShiMi, of K times the pooling product; ``model.L`` stays the full-band length).  The checkpoints get a
    ``pqmf`` entry with the four values, which ``generate`` picks up; a resume with other values raises ``PqmfMismatch``
    (a ValueError).  ``train.prior`` is refused; ``train.stft_weight`` compares the synthesised estimate with the
    waveform.  What such a model sounds like has not been measured."""
    opt_kind, ema_decay, clip_grad_norm = optimizer_options(optimizer, ema_decay, clip_grad_norm)
    from .training import stft_loss_options
    stft_cfg = stft_loss_options(stft_weight, stft_max_step, stft_resolutions, diffusion_cfg.get("T"), where="train")
    from .pqmf import PQMF, check_run, same_options
    pqmf_cfg = check_run(model_cfg, dataset_cfg, where="train")      # model.subbands: a multi-band run (pqmf.py)
    if stft_cfg is not None and pqmf_cfg is None and model_cfg.get("in_channels", 1) != 1:
        raise ValueError(f"train.stft_weight needs model.in_channels = 1 (got {model_cfg.get('in_channels')!r})")
    if pqmf_cfg is not None and prior not in (None, "none"):
        raise ValueError("train.prior does not combine with model.subbands (the adaptive prior is a full-band quantity; "
                         "its sub-band form is not built)")
    prior_cfg = prior_settings(prior, prior_energy_max, prior_energy_min, prior_std_min, model_cfg.get("unconditional"),
                               where="train", ref=prior_ref, floor=prior_floor, lifter=prior_lifter,
                               n_fft=dataset_cfg.get("filter_length", 1024))
    prior_cfg = prior_cfg if isinstance(prior_cfg, dict) else None
    prior_h = prior_hop(model_cfg, dataset_cfg) if prior_cfg is not None else None
    spectral = prior_cfg is not None and prior_cfg["kind"] == "spectral"
    if spectral and model_cfg.get("in_channels", 1) != 1:
        raise ValueError(f"train.prior=spectral needs model.in_channels = 1 (got {model_cfg.get('in_channels')!r})")

    def prior_of(mel, L):       # the prior's arguments of training_loss from a batch's own mel
        if spectral:
            return dict(prior_filter=stft.spectral_filter(mel, L, **{k: prior_cfg[k] for k in SPECTRAL_PRIOR_KEYS}),
                        prior_stft=stft)
        from .mel import prior_std_from_mel
        return dict(prior_std=prior_std_from_mel(mel, prior_h, L, **{k: prior_cfg[k] for k in PRIOR_KEYS}))
    from .distributed_util import apply_gradient_allreduce, reduce_tensor
    from .models import construct_model
    from .sampling import calc_diffusion_hyperparams
    from .training import training_loss
    from .models.utils import check_n_classes

    n_classes = check_n_classes(model_cfg.get("n_classes"))
    if label_dropout is not None and not n_classes:
        raise ValueError("train.label_dropout needs model.n_classes")
    label_dropout = float(0.1 if label_dropout is None else label_dropout) if n_classes else 0.0
    if not 0.0 <= label_dropout < 1.0:
        raise ValueError(f"train.label_dropout = {label_dropout!r} (needs 0 <= p < 1)")
    local_path, checkpoint_directory = local_directory(name, model_cfg, diffusion_cfg, dataset_cfg, "checkpoint", exp_root)
    log_path = os.path.join(exp_root, local_path, "train_log.jsonl")
    dh = calc_diffusion_hyperparams(**diffusion_cfg, fast=False)
    trainloader = dataloader(dataset_cfg, batch_size_per_gpu, num_gpus, unconditional=model_cfg["unconditional"],
                             rank=rank, num_workers=num_workers, n_classes=n_classes)
    if len(trainloader) == 0:
        raise RuntimeError("the dataset holds fewer clips than one batch")
    print("Data loaded")
    net = construct_model(dict(model_cfg)).cuda().train()
    if precision not in (None, "f32"):      # `+engine.precision=bf16x6`: the split GEMMs of either backbone's step on the bf16 matrix cores
        net.set_option("precision", precision)
    band = {} if pqmf_cfg is None else {"pqmf": PQMF(**pqmf_cfg)}    # (training_loss splits every batch into the sub-bands)
    if pqmf_cfg is not None:
        print("multi-band run: subbands={subbands} taps={taps} cutoff={cutoff:g} beta={beta:g}".format(**pqmf_cfg))
    print(f"{type(net).__name__} parameters: {sum(p.numel() for p in net.parameters()) / 1e6:.6f}M")   # `utils.py:76-88`
    if num_gpus > 1:
        net = apply_gradient_allreduce(net)
    learning_rate = float(learning_rate)
    groups = optim_param_groups(net, str(honour_optim_hints).lower() in ("1", "true"))
    own_lr = [isinstance(g, dict) and "lr" in g for g in groups] if isinstance(groups[0], dict) else [False]
    if opt_kind == "engine":
        from .optim import EngineAdam
        optimizer = EngineAdam(groups, lr=learning_rate, ema_decay=ema_decay, max_grad_norm=clip_grad_norm, module=net)
    else:
        optimizer = torch.optim.Adam(groups, lr=learning_rate)

    if ckpt_iter == "max":
        ckpt_iter = find_max_epoch(checkpoint_directory)
    ckpt_iter = int(ckpt_iter)
    if ckpt_iter >= 0:
        try:
            checkpoint = torch.load(os.path.join(checkpoint_directory, f"{ckpt_iter}.pkl"), map_location="cpu")
            if not same_prior(checkpoint.get("prior"), prior_cfg):
                raise PriorMismatch(f"checkpoint {ckpt_iter} was trained with the prior {checkpoint.get('prior')!r}, this run "
                                    f"asks for {prior_cfg!r}: resume with the same train.prior keys (weights trained "
                                    "towards one prior are not a start for another)")
            if not same_options(checkpoint.get("pqmf"), pqmf_cfg):
                raise PqmfMismatch(f"checkpoint {ckpt_iter} was trained with the filter bank {checkpoint.get('pqmf')!r}, this "
                                   f"run asks for {pqmf_cfg!r}: resume with the same model.subbands / model.pqmf_* keys")
            net.load_state_dict(checkpoint["model_state_dict"])
            if "stft_loss" in checkpoint or stft_cfg is not None:
                print(f"checkpoint {ckpt_iter} was trained with stft_loss = {checkpoint.get('stft_loss')!r}, this run "
                      f"trains with {stft_cfg!r}")
            if "optimizer_state_dict" in checkpoint:
                optimizer.load_state_dict(checkpoint["optimizer_state_dict"])
                for g, own in zip(optimizer.param_groups, own_lr):    # `train.py:111-112` (one group there); a hinted lr stays
                    if not own:
                        g["lr"] = learning_rate
            if ema_decay is not None:
                if "ema_state_dict" in checkpoint:
                    optimizer.load_ema_state_dict(checkpoint["ema_state_dict"])
                else:
                    optimizer.reset_ema()
                    print(f"checkpoint {ckpt_iter} holds no ema_state_dict: the EMA starts from the loaded weights")
            print(f"Successfully loaded model at iteration {ckpt_iter}")
        except (PriorMismatch, PqmfMismatch):    # (not a checkpoint that failed to load: a run that would silently change its loss)
            raise
        except Exception as e:   # the reference swallows the error the same way (`train.py:115-117`)
            print(f"Model checkpoint found at iteration {ckpt_iter}, but was not successfully loaded ({e}) - "
                  "training from scratch.")
            ckpt_iter = -1
            if ema_decay is not None:
                optimizer.reset_ema()       # (a partly loaded model: the shadows follow whatever the weights are now)
    else:
        print("No valid checkpoint model found - training from scratch.")
        ckpt_iter = -1

    def log(record, step):
        if rank == 0:
            with open(log_path, "a") as f:
                f.write(json.dumps(dict(record, step=step)) + "\n")

    stft = None
    if not model_cfg["unconditional"]:
        from .mel import MAX_WAV_VALUE, TacotronSTFT
        keys = dict(filter_length="filter_length", hop_length="hop_length", win_length="win_length",
                    sampling_rate="sampling_rate", mel_fmin="mel_fmin", mel_fmax="mel_fmax")
        stft = TacotronSTFT(**{k: dataset_cfg[v] for k, v in keys.items() if v in dataset_cfg})
    loss_fn = nn.MSELoss()
    n_iter = ckpt_iter + 1
    epoch = 0
    while n_iter < n_iters + 1:
        epoch_loss, n_batches = 0.0, 0
        if getattr(trainloader, "sampler", None) is not None and hasattr(trainloader.sampler, "set_epoch"):
            trainloader.sampler.set_epoch(epoch)
        for data in trainloader:
            if stft is None:
                audio, mel = data[0].cuda(), None
            else:   # `mel2samp.py:76-82,107-111`: mel of audio / MAX_WAV_VALUE, audio [B, 1, L] in [-1, 1]
                audio = (data.cuda() / MAX_WAV_VALUE).unsqueeze(1)
                mel = stft.mel_spectrogram(audio[:, 0])
            optimizer.zero_grad()
            if stft_cfg is not None:
                parts = {}
                more = dict(labels=data[2], label_dropout=label_dropout) if n_classes else {}
                if prior_cfg is not None:
                    more.update(prior_of(mel, audio.shape[-1]))
                loss = training_loss(net, loss_fn, audio, dh, mel_spec=mel, stft_weight=stft_cfg["weight"],
                                     stft_max_step=stft_cfg["max_step"], stft_resolutions=stft_cfg["resolutions"],
                                     parts=parts, **more, **band)
            elif prior_cfg is not None:
                more = dict(labels=data[2], label_dropout=label_dropout) if n_classes else {}
                loss = training_loss(net, loss_fn, audio, dh, mel_spec=mel, **prior_of(mel, audio.shape[-1]), **more)
            elif n_classes:    # (the labels stay on the host: the engine takes them from there, nothing waits for the GPU)
                loss = training_loss(net, loss_fn, audio, dh, mel_spec=mel, labels=data[2], label_dropout=label_dropout,
                                     **band)
            else:
                loss = training_loss(net, loss_fn, audio, dh, mel_spec=mel, **band)
            reduced_loss = reduce_tensor(loss.data, num_gpus).item() if num_gpus > 1 else loss.item()
            loss.backward()
            optimizer.step()
            epoch_loss += reduced_loss
            n_batches += 1
            if n_iter % iters_per_logging == 0:
                record = {"train/loss": reduced_loss, "train/log_loss": float(np.log(reduced_loss))}
                if clip_grad_norm is not None:      # (the norm lives on the device: read at logging iterations only)
                    record["train/grad_norm"] = float(optimizer.grad_norm)
                if stft_cfg is not None:            # (rank 0's own terms: the spectral term is local to a rank)
                    record["train/eps_loss"] = float(parts["eps"])
                    record["train/stft_loss"] = float(parts["stft"])
                log(record, n_iter)
            if n_iter % iters_per_ckpt == 0 and rank == 0:
                saved = {"model_state_dict": net.state_dict(), "optimizer_state_dict": optimizer.state_dict()}
                if ema_decay is not None:       # (the in-loop generate below samples from it)
                    saved["ema_state_dict"] = optimizer.ema_state_dict(net)
                if prior_cfg is not None:       # (generate samples from the prior the weights were trained with)
                    saved["prior"] = dict(prior_cfg)
                if stft_cfg is not None:        # (informational: what the loss of these weights held)
                    saved["stft_loss"] = dict(stft_cfg)
                if pqmf_cfg is not None:        # (generate synthesises with the bank the weights were trained on)
                    saved["pqmf"] = dict(pqmf_cfg)
                torch.save(saved, os.path.join(checkpoint_directory, f"{n_iter}.pkl"))
                print(f"model at iteration {n_iter} is saved")
                if generate_cfg and generate_cfg.get("n_samples", 0):
                    if not model_cfg["unconditional"]:
                        assert generate_cfg.get("mel_name") is not None     # `train.py:170`
                    gen = dict(generate_cfg, ckpt_iter=n_iter)
                    if n_classes:
                        gen.setdefault("label", "all")      # the classes in turn over the batch
                    net.eval()
                    wavs = []
                    # generate.report_metrics / generate.report_pitch: metrics.py
                    rows = [] if gen.get("report_metrics") or gen.get("report_pitch") or gen.get("report_stoi") else None
                    if rows is not None:
                        gen["metric_rows"] = rows
                    generate(rank, diffusion_cfg, model_cfg, dataset_cfg, name=name, exp_root=exp_root,
                             written=wavs, **gen)
                    net.train()
                    log({"val/audio": wavs}, n_iter)     # the reference logs the clips to wandb (`train.py:180-183`)
                    if rows and gen.get("report_metrics"):     # the means over the clips just written, against their source wavs
                        log({"val/" + k: float(np.mean([r[k] for r in rows]))
                             for k in ("mr_stft", "ls_mae", "lsd", "mcd")}, n_iter)
                    if rows and gen.get("report_pitch"):       # nan-means: a clip without a voiced frame has no F0 numbers
                        from .metrics import PITCH_METRICS, nanmean
                        means = {k: nanmean(r[k] for r in rows) for k in PITCH_METRICS if k in rows[0]}
                        log({"val/" + k: v for k, v in means.items() if np.isfinite(v)}, n_iter)
                    if rows and gen.get("report_stoi"):        # nan-means: a clip that keeps under 30 frames has neither
                        from .metrics import STOI_METRICS, nanmean
                        means = {k: nanmean(r[k] for r in rows) for k in STOI_METRICS if k in rows[0]}
                        log({"val/" + k: v for k, v in means.items() if np.isfinite(v)}, n_iter)
            n_iter += 1
            if n_iter >= n_iters + 1:
                break
        epoch += 1
        if n_batches:
            log({"train/loss_epoch": epoch_loss / n_batches, "train/log_loss_epoch": float(np.log(epoch_loss / n_batches))},
                n_iter)
    return net


def distributed_train(rank, num_gpus, group_name, cfg, exp_root="exp"):
    """``train.py:27-47``."""
    from .distributed_util import init_distributed
    dist_cfg = dict(cfg.get("distributed") or {})
    if num_gpus > 1:
        torch.cuda.set_device(rank % torch.cuda.device_count())
        init_distributed(rank, num_gpus, group_name, dist_cfg.get("dist_backend", "nccl"),
                         dist_cfg.get("dist_url", "tcp://127.0.0.1:54321"))
    tr = dict(cfg["train"])
    tr.setdefault("precision", (cfg.get("engine") or {}).get("precision"))
    train(rank, num_gpus, dict(cfg["diffusion"]), dict(cfg["model"]), dict(cfg["dataset"]), dict(cfg.get("generate") or {}),
          exp_root=exp_root, **tr)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config-dir", required=True, help="Hydra-style config tree (the reference's configs/)")
    ap.add_argument("--exp-root", default="exp")
    ap.add_argument("overrides", nargs="*", help="key=value overrides, e.g. experiment=sc09 model=sashimi")
    args = ap.parse_args(argv)
    cfg = load_config(args.config_dir, args.overrides)
    cfg.pop("wandb", None)
    os.makedirs(args.exp_root, mode=0o775, exist_ok=True)
    group = time.strftime("%Y%m%d-%H%M%S")
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1:      # launched by torch.distributed.run
        distributed_train(int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), group, cfg, args.exp_root)
        return
    num_gpus = torch.cuda.device_count()
    if num_gpus <= 1:
        distributed_train(0, 1, group, cfg, args.exp_root)
    else:  # one process per GPU (`train.py:236-249`)
        import torch.multiprocessing as mp
        mp.spawn(distributed_train, args=(num_gpus, group, cfg, args.exp_root), nprocs=num_gpus, join=True)


if __name__ == "__main__":
    main(sys.argv[1:])

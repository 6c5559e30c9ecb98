"""Objective metrics of a directory of generated wavs against a directory of recordings (not in the reference).

    python -m diffwave_sashimi_amd.evaluate --generated exp/<run>/waveforms/<iter> --reference /data/LJSpeech/wavs \
        --config-dir /path/to/configs experiment=ljspeech --json metrics.json

Files are paired by wav stem; a generated stem with ``generate``'s ``{n}k_`` prefix (``0k_LJ001-0001``) matches
``LJ001-0001`` when the plain stem has no partner.  Every pair is trimmed to its shorter member (a vocoded clip is
``frames x hop_length`` samples long, up to one hop more than its recording) and goes through
``metrics.spectral_metrics`` in ragged batches, longest first.  One table row per metric is printed -- mean, standard
deviation, 95 % interval of the mean, n -- and ``--json`` receives the per-file values.

The STFT keys (``--sampling-rate``, ``--filter-length``, ``--hop-length``, ``--win-length``, ``--mel-fmin``,
``--mel-fmax``) set the transform of ``ls_mae`` / ``lsd`` / ``mcd``; with ``--config-dir`` they are read from the
composed config's ``dataset`` (``key=value`` overrides as for ``generate``), and a key spelled out wins.

``--pitch`` adds the pitch family of ``metrics.pitch_metrics`` (YIN tracks of both files at ``--sampling-rate`` and
``--hop-length``; ``--pitch-win``, ``--pitch-fmin``, ``--pitch-fmax``, ``--pitch-threshold``): six more rows, printed after
the others.  ``f0_rmse`` / ``f0_cents`` / ``gpe`` of a pair with no frame voiced in both files, and ``vuv_f1`` of a pair
without a voiced frame, are NaN: such a pair is left out of that metric's mean, and the ``n`` column counts the rest.  ``--json`` holds ``null``
for such a value (strict JSON has no NaN) and the parameters under ``"pitch"``.

``--stoi`` adds ``stoi`` and ``estoi`` (``metrics.stoi``: both files converted to 10 kHz on the GPU, Taal's constants):
two more rows, printed last.  A pair that keeps fewer than 30 frames has neither; it is treated like an undefined pitch
value (left out of the mean, ``null`` in ``--json``, the parameters under ``"stoi"``).

``--griffin-lim N`` (``--griffin-lim-momentum``, default 0) adds the baseline that needs no weights: the engine's log-mel of
every recording at the run's STFT keys is inverted with N Griffin-Lim iterations (``TacotronSTFT.mel_to_audio``, in the same
ragged batches) and scored against the recording -- cut to its whole hops, ``samples // hop_length`` of them -- with the
same metric calls as the generated file, ``--pitch`` and ``--stoi`` included.  A second block of rows headed ``griffin-lim
baseline (N iterations)`` is printed; ``--json`` receives ``baseline_<metric>`` per file and the parameters and the
block's summary under ``"griffin_lim"``.

``--resample``: a wav whose rate is not ``--sampling-rate`` is converted on the GPU after loading (``audio.resample``)
instead of being refused; the one-hop pairing check and the trim see the converted clips, and the number of converted
files is printed.
"""
import argparse
import json
import math
import os
import re
import sys

import numpy as np
import torch

from . import metrics as _metrics

STFT_KEYS = ("sampling_rate", "filter_length", "hop_length", "win_length", "mel_fmin", "mel_fmax")
STFT_DEFAULTS = dict(sampling_rate=22050, filter_length=1024, hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0)
_PREFIX = re.compile(r"^\d+k_(.+)$")


def _stems(directory):
    if not os.path.isdir(directory):
        raise ValueError(f"evaluate: {directory} is not a directory")
    return sorted(f[:-4] for f in os.listdir(directory) if f.endswith(".wav"))


def pair_files(generated_dir, reference_dir):
    """``(pairs, unpaired_generated, unpaired_reference)``: ``pairs`` is a sorted list of ``(generated stem, reference
    stem)``.  A generated stem pairs with the reference of the same name; one without such a partner and of the form
    ``{n}k_{stem}`` pairs with ``{stem}``.  A reference that two generated files claim is an error (ValueError)."""
    gen, ref = _stems(generated_dir), set(_stems(reference_dir))
    pairs, lone, taken = [], [], {}
    for g in gen:
        m = _PREFIX.match(g)
        r = g if g in ref else (m.group(1) if m and m.group(1) in ref else None)
        if r is None:
            lone.append(g)
            continue
        if r in taken:
            raise ValueError(f"evaluate: {taken[r]}.wav and {g}.wav both pair with the reference {r}.wav")
        taken[r] = g
        pairs.append((g, r))
    return pairs, lone, sorted(ref - set(taken))


def read_wav(path):
    """``(x, sampling rate)``: a wav as float32 [T] -- int16 scaled by 1/32768, float as it is, the first channel -- at
    whatever rate it has; ValueError on another sample type."""
    from scipy.io import wavfile
    sr, x = wavfile.read(path)
    return _samples(path, x), int(sr)


def load_wav(path, sampling_rate):
    """A wav as float32 [T]: int16 scaled by 1/32768, float as it is, the first channel; ValueError on another rate or
    sample type."""
    from scipy.io import wavfile
    sr, x = wavfile.read(path)
    if sr != sampling_rate:
        raise ValueError(f"evaluate: {path} has sampling rate {sr}, expected {sampling_rate}")
    return _samples(path, x)


def _samples(path, x):
    if x.dtype == np.int16:
        x = x.astype(np.float32) / 32768.0
    elif x.dtype.kind == "f":
        x = x.astype(np.float32)
    else:
        raise ValueError(f"evaluate: {path} holds {x.dtype} samples (int16 and float wavs are read)")
    if x.ndim == 2:
        x = x[:, 0]
    return torch.from_numpy(np.ascontiguousarray(x))


def _load_converted(path, sampling_rate, converted):
    """``--resample``: the wav at ``path``, converted to ``sampling_rate`` on the GPU (``audio.resample``) where it has
    another rate; such a path is appended to ``converted``."""
    from . import audio
    x, sr = read_wav(path)
    if sr == sampling_rate:
        return x
    audio.check_ratio(sr, sampling_rate, what=f"evaluate --resample ({path})")
    converted.append(path)
    return audio.resample(x[None].to("cuda" if torch.cuda.is_available() else "cpu"), sr, sampling_rate)[0][0].cpu()


def load_pairs(generated_dir, reference_dir, pairs, sampling_rate, hop_length, converted=None):
    """The wavs of ``pairs`` as a list of ``(x, y)`` float32 [len] tensors, each trimmed to its shorter member; a pair
    whose lengths differ by more than ``hop_length`` is not the same utterance (ValueError).  ``converted``: None -- a wav
    at another rate than ``sampling_rate`` is a ValueError -- or a list: such a wav is converted on the GPU first (the
    length check and the trim see the converted clips) and its path appended."""
    out = []
    for g, r in pairs:
        if converted is None:
            x = load_wav(os.path.join(generated_dir, g + ".wav"), sampling_rate)
            y = load_wav(os.path.join(reference_dir, r + ".wav"), sampling_rate)
        else:
            x = _load_converted(os.path.join(generated_dir, g + ".wav"), sampling_rate, converted)
            y = _load_converted(os.path.join(reference_dir, r + ".wav"), sampling_rate, converted)
        if abs(x.shape[0] - y.shape[0]) > hop_length:
            raise ValueError(f"evaluate: {g}.wav has {x.shape[0]} samples and {r}.wav {y.shape[0]}: more than one hop "
                             f"({hop_length}) apart")
        n = min(x.shape[0], y.shape[0])
        out.append((x[:n], y[:n]))
    return out


def evaluate_pairs(clips, stft, batch_size=16, device=None, resolutions=_metrics.MR_STFT_RESOLUTIONS, n_cep=13, pitch=None,
                   stoi=None):
    """``spectral_metrics`` of a list of ``(x, y)`` clips of different lengths: sorted longest first and cut into
    batches of ``batch_size`` (``generate.ragged_plan``), each batch at its longest length with ``lengths=``.  Returns a
    list of dicts of floats in the order of ``clips``.  Without a GPU the metric call raises (there is no CPU path).
    ``pitch``: None, or the keyword arguments of ``metrics.pitch_metrics`` (a dict, possibly empty), whose
    ``PITCH_METRICS`` are then added to every row (NaN where a clip has none).  ``stoi``: None, or the clips' sampling
    rate: ``metrics.stoi``'s ``STOI_METRICS`` are added (NaN for a clip that keeps fewer than 30 frames)."""
    from .generate import ragged_plan
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    rows = [None] * len(clips)
    lens = [int(x.shape[0]) for x, _ in clips]
    for batch in ragged_plan(lens, batch_size) if clips else []:
        T = lens[batch[0]]
        x, y = torch.zeros(len(batch), T), torch.zeros(len(batch), T)
        for b, k in enumerate(batch):
            x[b, :lens[k]], y[b, :lens[k]] = clips[k]
        x, y = x.to(device), y.to(device)
        m = _metrics.spectral_metrics(x, y, [lens[k] for k in batch], stft=stft, resolutions=resolutions, n_cep=n_cep)
        if pitch is not None:
            pm = _metrics.pitch_metrics(x, y, [lens[k] for k in batch], **pitch)
            m = dict(m, **{key: pm[key] for key in _metrics.PITCH_METRICS})
        if stoi is not None:
            sm = _metrics.stoi(x, y, [lens[k] for k in batch], sampling_rate=stoi)
            m = dict(m, **{key: sm[key] for key in _metrics.STOI_METRICS})
        for b, k in enumerate(batch):
            rows[k] = {key: float(v[b]) for key, v in m.items()}
    return rows


def griffin_lim_clips(clips, stft, n_iters, momentum=0.0, batch_size=16, device=None):
    """The Griffin-Lim baseline of a list of ``(x, y)`` clips: ``(g, y')`` per clip, ``y'`` the recording cut to its whole
    hops and ``g = stft.mel_to_audio(stft.mel_spectrogram(y'))`` with ``n_iters`` iterations, of the same length.  The mels
    are taken clip by clip (a clip's own reflection), the inversions run in the ragged batches of ``evaluate_pairs``; a
    clip's estimate does not depend on its batch."""
    from .generate import ragged_plan
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    hop = stft.hop_length
    lens = [int(y.shape[0]) // hop * hop for _, y in clips]
    out = [None] * len(clips)
    for batch in ragged_plan(lens, batch_size) if clips else []:
        mels = [stft.mel_spectrogram(clips[k][1][None, :lens[k]].to(device)) for k in batch]
        mel = torch.zeros(len(batch), mels[0].shape[1], mels[0].shape[2], device=device)
        for b, m in enumerate(mels):
            mel[b, :, :m.shape[2]] = m[0]
        g = stft.mel_to_audio(mel, n_iters=n_iters, momentum=momentum, lengths=[lens[k] for k in batch]).cpu()
        for b, k in enumerate(batch):
            out[k] = (g[b, :lens[k]].clone(), clips[k][1][:lens[k]])
    return out


def summarise(rows):
    """Per metric ``(mean, standard deviation, half width of the 95 % interval of the mean, n)``: the sample standard
    deviation (n - 1) and the normal interval 1.96 s / sqrt(n); both 0 for a single file."""
    out = {}
    for key in (rows[0] if rows else {}):
        v = np.array([r[key] for r in rows], dtype=np.float64)
        sd = float(v.std(ddof=1)) if len(v) > 1 else 0.0
        out[key] = (float(v.mean()), sd, 1.96 * sd / math.sqrt(len(v)), len(v))
    return out


def summarise_finite(rows, keys):
    """``summarise`` of ``keys`` over the rows whose value is finite (a NaN marks a clip on which the metric is
    undefined): n counts those rows; the mean is NaN and the rest 0 where there is none."""
    out = {}
    for key in keys:
        v = np.array([r[key] for r in rows], dtype=np.float64)
        v = v[np.isfinite(v)]
        sd = float(v.std(ddof=1)) if len(v) > 1 else 0.0
        out[key] = (float(v.mean()), sd, 1.96 * sd / math.sqrt(len(v)), len(v)) if len(v) else (float("nan"), 0.0, 0.0, 0)
    return out


def pitch_arguments(args, keys):
    """The ``metrics.pitch_metrics`` keywords of the parsed ``--pitch*`` flags at the STFT ``keys``' rate and hop, or
    None without ``--pitch`` (a ``--pitch-*`` value without it is a ValueError)."""
    given = {k: getattr(args, "pitch_" + k) for k in ("win", "fmin", "fmax", "threshold")}
    if not args.pitch:
        extra = [k for k, v in given.items() if v is not None]
        if extra:
            raise ValueError(f"evaluate: --pitch-{extra[0]} needs --pitch")
        return None
    pitch = dict(_metrics.PITCH_DEFAULTS, sampling_rate=keys["sampling_rate"], hop=keys["hop_length"])
    pitch.update({k: v for k, v in given.items() if v is not None})
    return pitch


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--generated", required=True, help="directory of generated wavs")
    ap.add_argument("--reference", required=True, help="directory of the recordings")
    ap.add_argument("--config-dir", help="Hydra-style config tree: the STFT keys are read from its dataset")
    for k in STFT_KEYS:
        ap.add_argument("--" + k.replace("_", "-"), type=int if k.endswith("length") or k == "sampling_rate" else float)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--json", help="write the per-file values here")
    ap.add_argument("--strict", action="store_true", help="an unpaired file is an error")
    ap.add_argument("--pitch", action="store_true", help="add the pitch metrics (metrics.pitch_metrics)")
    ap.add_argument("--pitch-win", type=int, help="integration window of the pitch tracker in samples (default 1024)")
    ap.add_argument("--pitch-fmin", type=float, help="lowest F0 searched, Hz (default 50)")
    ap.add_argument("--pitch-fmax", type=float, help="highest F0 searched, Hz (default 550)")
    ap.add_argument("--pitch-threshold", type=float, help="YIN threshold (default 0.15)")
    ap.add_argument("--stoi", action="store_true", help="add STOI and ESTOI (metrics.stoi; both files go to 10 kHz)")
    ap.add_argument("--griffin-lim", type=int, metavar="N",
                    help="add the baseline rows: every recording's mel inverted with N Griffin-Lim iterations")
    ap.add_argument("--griffin-lim-momentum", type=float, help="Fast Griffin-Lim's momentum in [0, 1) (default 0)")
    ap.add_argument("--resample", action="store_true",
                    help="convert a wav at another rate to --sampling-rate on the GPU instead of refusing it")
    ap.add_argument("overrides", nargs="*", help="key=value overrides of --config-dir, e.g. experiment=ljspeech")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.overrides and not args.config_dir:
        raise ValueError("evaluate: key=value overrides need --config-dir")
    keys = dict(STFT_DEFAULTS)
    if args.config_dir:
        from .generate import load_config
        ds = load_config(args.config_dir, args.overrides).get("dataset") or {}
        keys.update({k: ds[k] for k in STFT_KEYS if k in ds})
    keys.update({k: getattr(args, k) for k in STFT_KEYS if getattr(args, k) is not None})
    if args.batch_size < 1:
        raise ValueError(f"evaluate: --batch-size {args.batch_size}: expected an integer >= 1")
    pitch = pitch_arguments(args, keys)
    if pitch is not None:       # the parameters are checked before a file is read (the clips: once they are loaded)
        _metrics.check_pitch([], what="evaluate --pitch", **pitch)

    baseline = None             # --griffin-lim: (N, momentum), checked before a file is read
    if args.griffin_lim is None and args.griffin_lim_momentum is not None:
        raise ValueError("evaluate: --griffin-lim-momentum needs --griffin-lim")
    if args.griffin_lim is not None:
        from .mel import check_griffin_lim
        baseline = check_griffin_lim(args.griffin_lim, args.griffin_lim_momentum or 0.0, "evaluate --griffin-lim")

    pairs, lone_gen, lone_ref = pair_files(args.generated, args.reference)
    for name, lone in (("generated", lone_gen), ("reference", lone_ref)):
        if lone:
            print(f"unpaired {name} files ({len(lone)}): " + " ".join(s + ".wav" for s in lone))
    if args.strict and (lone_gen or lone_ref):
        raise ValueError(f"evaluate: --strict: {len(lone_gen)} generated and {len(lone_ref)} reference files have no partner")
    if not pairs:
        raise ValueError(f"evaluate: no generated wav under {args.generated} pairs with a wav under {args.reference}")
    if args.stoi:               # the rate is checked before a file is read
        _metrics.stoi_lengths([], keys["sampling_rate"], "evaluate --stoi")
    converted = [] if args.resample else None
    clips = load_pairs(args.generated, args.reference, pairs, keys["sampling_rate"], keys["hop_length"], converted)
    if converted is not None:
        print(f"converted to {keys['sampling_rate']} Hz: {len(converted)} files")
    from .mel import TacotronSTFT
    stft = TacotronSTFT(filter_length=keys["filter_length"], hop_length=keys["hop_length"], win_length=keys["win_length"],
                        sampling_rate=keys["sampling_rate"], mel_fmin=keys["mel_fmin"], mel_fmax=keys["mel_fmax"])
    nan_keys = (_metrics.PITCH_METRICS if pitch is not None else ()) + (_metrics.STOI_METRICS if args.stoi else ())

    def score(clips):
        if not nan_keys:
            rows = evaluate_pairs(clips, stft, args.batch_size)
            summary = summarise(rows)
        else:
            rows = evaluate_pairs(clips, stft, args.batch_size, pitch=pitch, stoi=keys["sampling_rate"] if args.stoi else None)
            summary = summarise([{k: v for k, v in row.items() if k not in nan_keys} for row in rows])
            summary.update(summarise_finite(rows, nan_keys))
        print(f"{'metric':<20}{'mean':>12}{'std':>12}{'95% +-':>12}{'n':>6}")
        for key, (mean, sd, ci, n) in summary.items():
            print(f"{key:<20}{mean:>12.6f}{sd:>12.6f}{ci:>12.6f}{n:>6d}")
        return rows, summary

    rows, summary = score(clips)
    if baseline is not None:
        print(f"griffin-lim baseline ({baseline[0]} iterations)")
        base_rows, base_summary = score(griffin_lim_clips(clips, stft, *baseline, batch_size=args.batch_size))
    if args.json:
        record = {"stft": keys,
                  "files": [dict(generated=g + ".wav", reference=r + ".wav", samples=int(c[0].shape[0]), **row)
                            for (g, r), c, row in zip(pairs, clips, rows)],
                  "summary": {k: dict(mean=m, std=s, ci95=c, n=n) for k, (m, s, c, n) in summary.items()},
                  "unpaired_generated": lone_gen, "unpaired_reference": lone_ref}
        if pitch is not None:
            record["pitch"] = pitch
        if args.stoi:
            record["stoi"] = dict(_metrics.STOI_DEFAULTS, sampling_rate=keys["sampling_rate"])
        if converted is not None:
            record["converted"] = [os.path.basename(p) for p in converted]
        base_keys = ()
        if baseline is not None:
            for entry, row in zip(record["files"], base_rows):
                entry.update({"baseline_" + k: v for k, v in row.items()})
            base_keys = tuple("baseline_" + k for k in nan_keys)
            record["griffin_lim"] = dict(n_iters=baseline[0], momentum=baseline[1], seed=0,
                                         summary={k: dict(mean=m, std=s, ci95=c, n=n) for k, (m, s, c, n) in base_summary.items()})
        if nan_keys:                    # an undefined value (NaN) is written as null: strict JSON has no NaN
            for entry in record["files"]:
                entry.update({k: None for k in nan_keys + base_keys if math.isnan(entry[k])})
            for k in nan_keys:
                if math.isnan(record["summary"][k]["mean"]):
                    record["summary"][k]["mean"] = None
                if baseline is not None and math.isnan(record["griffin_lim"]["summary"][k]["mean"]):
                    record["griffin_lim"]["summary"][k]["mean"] = None
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)
    return rows


if __name__ == "__main__":
    main(sys.argv[1:])

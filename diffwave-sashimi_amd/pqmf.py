"""Pseudo-QMF filter bank for multi-band runs (Multi-band MelGAN, Yang et al. 2020; not in the reference).

An analysis bank splits a waveform ``[B, 1, T]`` into K critically sampled sub-bands ``[B, K, T/K]``; the diffusion model
is trained and sampled on the sub-bands (a K-th of the positions per network evaluation) and one synthesis bank at the end
of a run puts the waveform back.  The filters are designed here in float64 (``design``); the two banks run in
``dws_pqmf_analysis`` / ``dws_pqmf_synthesis`` (``csrc/pqmf_kernels.hip``), each the other's adjoint under the
tap-reversed table, so both directions are differentiable (first order).  There is no CPU path.

    prototype   h[n]     = c sinc(c (n - taps/2)) kaiser(taps + 1, beta)[n],  n = 0 .. taps,  normalised to sum(h) = 1
    analysis    ha[k, n] = 2 h[n] cos((2k + 1) pi / (2K) (n - taps/2) + (-1)^k pi/4)
    synthesis   hs[k, n] = 2 h[n] cos((2k + 1) pi / (2K) (n - taps/2) - (-1)^k pi/4)

The bank reconstructs nearly, not perfectly: 6.2e-4 (K = 4) and 4.4e-4 (K = 2) relative error on white noise in float64.
What a model trained on sub-bands sounds like has not been measured.
"""
import math

import numpy as np
import torch

from . import _lib

TILE = 1024                 # full-band positions per workgroup: PQMF_TILE of csrc/pqmf_kernels.hip (dws_pqmf_tile())
SUBBANDS = (2, 4)           # the engine takes up to 4 channels; K = 3 has no use
TAPS_MAX = 254
# K = 4: the value of the public Multi-band MelGAN recipes.  K = 2: the minimiser of the Lin-Vaidyanathan objective
# max_{m != 0} |(h * h)[taps + 2 K m]| on a 2e-4 grid.
DEFAULT_CUTOFF = {4: 0.142, 2: 0.267}
MODEL_KEYS = ("subbands", "pqmf_taps", "pqmf_cutoff", "pqmf_beta")     # the keys of the `model` config group

_tables = {}                # (device, K, taps, cutoff, beta) -> (ha, hs, rev(ha), rev(hs)) float32 [K, taps + 1]


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_real(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(float(v))


def check_options(subbands=4, taps=62, cutoff=None, beta=9.0, where="PQMF"):
    """The four values of a bank, checked (ValueError naming the value): ``(K, taps, cutoff, beta)`` with the default
    cutoff filled in."""
    if not _is_int(subbands) or subbands not in SUBBANDS:
        raise ValueError(f"{where}: subbands = {subbands!r} (2 or 4)")
    if not _is_int(taps) or not 2 <= taps <= TAPS_MAX or taps % 2:
        raise ValueError(f"{where}: taps = {taps!r} (an even integer in 2 .. {TAPS_MAX})")
    if cutoff is None:
        cutoff = DEFAULT_CUTOFF[int(subbands)]
    if not _is_real(cutoff) or not 0.0 < float(cutoff) < 1.0:
        raise ValueError(f"{where}: cutoff = {cutoff!r} (a number inside (0, 1), in units of the Nyquist frequency)")
    if not _is_real(beta) or float(beta) < 0.0:
        raise ValueError(f"{where}: beta = {beta!r} (a number >= 0)")
    return int(subbands), int(taps), float(cutoff), float(beta)


def prototype(taps=62, cutoff=0.142, beta=9.0):
    """The Kaiser-windowed sinc low-pass ``h`` [taps + 1] in float64, ``sum(h) = 1`` (scipy's ``firwin(taps + 1, cutoff,
    window=("kaiser", beta))``)."""
    n = np.arange(taps + 1, dtype=np.float64)
    h = cutoff * np.sinc(cutoff * (n - taps / 2)) * np.kaiser(taps + 1, beta)
    return h / h.sum()


def design(subbands=4, taps=62, cutoff=None, beta=9.0):
    """``(ha, hs)``: the analysis and synthesis filters [K, taps + 1] in float64 (the formulas of the module docstring)."""
    K, taps, cutoff, beta = check_options(subbands, taps, cutoff, beta, "pqmf.design")
    h = prototype(taps, cutoff, beta)
    n = np.arange(taps + 1, dtype=np.float64) - taps / 2
    k = np.arange(K, dtype=np.float64)[:, None]
    arg = (2 * k + 1) * (np.pi / (2 * K)) * n[None, :]
    sign = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)[:, None] * (np.pi / 4)
    return 2 * h[None, :] * np.cos(arg + sign), 2 * h[None, :] * np.cos(arg - sign)


def _need_gpu(t):
    from .metrics import _need_gpu as need
    need(t, t)


def _launch(which, x, table, K, taps, gain):
    """One launch on checked arguments: ``x`` float32 contiguous on the device, [B, T] (analysis) or [B, K, Ts]."""
    lib = _lib.load()
    B = int(x.shape[0])
    with torch.cuda.device(x.device):
        if which == "analysis":
            T = int(x.shape[1])
            out = torch.empty(B, K, T // K, device=x.device, dtype=torch.float32)
            _lib.check(lib.dws_pqmf_analysis(x.data_ptr(), B, T, table.data_ptr(), K, taps, float(gain), out.data_ptr(),
                                             _lib.current_stream()))
        else:
            Ts = int(x.shape[2])
            out = torch.empty(B, K * Ts, device=x.device, dtype=torch.float32)
            _lib.check(lib.dws_pqmf_synthesis(x.data_ptr(), B, Ts, table.data_ptr(), K, taps, float(gain), out.data_ptr(),
                                              _lib.current_stream()))
    return out


class _Bank(torch.autograd.Function):
    """One bank with its table and the tap-reversed one: the backward is the OTHER entry with the reversed table and
    the same gain (include/dws.h).  First order only."""

    @staticmethod
    def forward(ctx, x, which, table, reversed_table, K, taps, gain):
        ctx.cfg = ("synthesis" if which == "analysis" else "analysis", reversed_table, K, taps, gain)
        return _launch(which, x, table, K, taps, gain)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        which, table, K, taps, gain = ctx.cfg
        return _launch(which, g.to(torch.float32).contiguous(), table, K, taps, gain), None, None, None, None, None, None


class PQMF:
    """``PQMF(subbands=4, taps=62, cutoff=None, beta=9.0)``: the bank of ``design`` on the HIP engine.  ``cutoff=None``
    is 0.142 for K = 4 and 0.267 for K = 2.  Anything but K in {2, 4} and an even ``taps`` in 2 .. 254 is a ValueError."""

    def __init__(self, subbands=4, taps=62, cutoff=None, beta=9.0):
        self.subbands, self.taps, self.cutoff, self.beta = check_options(subbands, taps, cutoff, beta)

    def options(self):
        """The four values as a dict (the ``pqmf`` entry of a checkpoint)."""
        return dict(subbands=self.subbands, taps=self.taps, cutoff=self.cutoff, beta=self.beta)

    def __repr__(self):
        return "PQMF(subbands={subbands}, taps={taps}, cutoff={cutoff!r}, beta={beta!r})".format(**self.options())

    def filters(self):
        """``design`` of this bank: ``(ha, hs)`` float64 [K, taps + 1]."""
        return design(self.subbands, self.taps, self.cutoff, self.beta)

    def _tables(self, device):
        key = (device, self.subbands, self.taps, self.cutoff, self.beta)
        if key not in _tables:
            ha, hs = self.filters()
            _tables[key] = tuple(torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(device)
                                 for f in (ha, hs, ha[:, ::-1], hs[:, ::-1]))
        return _tables[key]

    def check_analysis_input(self, x, what="PQMF.analysis"):
        """ValueError unless ``x`` is a float tensor [B, 1, T] or [B, T] with T a positive multiple of K."""
        if not isinstance(x, torch.Tensor) or not x.dtype.is_floating_point or x.dim() not in (2, 3) or \
                (x.dim() == 3 and x.shape[1] != 1):
            raise ValueError(f"{what}: x has shape {tuple(getattr(x, 'shape', ()))!r}, expected a float tensor [B, 1, T] or "
                             "[B, T]")
        if x.shape[0] < 1 or x.shape[-1] < 1 or x.shape[-1] % self.subbands:
            raise ValueError(f"{what}: x {tuple(x.shape)}: the length must be a positive multiple of subbands = "
                             f"{self.subbands}")

    def analysis(self, x):
        """``[B, 1, T]`` or ``[B, T]`` -> the K sub-bands ``[B, K, T/K]`` (float32, cuda), differentiable in ``x``:
        ``out[b, k, t] = sum_n ha[k, n] x[b, K t + n - taps/2]``, x read as zero outside the clip.  Arguments are checked
        first (ValueError), then the device (RuntimeError)."""
        self.check_analysis_input(x)
        _need_gpu(x)
        ha, _, ha_rev, _ = self._tables(x.device)
        x = (x[:, 0] if x.dim() == 3 else x).to(torch.float32).contiguous()
        return _Bank.apply(x, "analysis", ha, ha_rev, self.subbands, self.taps, 1.0)

    def synthesis(self, s):
        """The K sub-bands ``[B, K, Ts]`` -> ``[B, 1, K Ts]`` (float32, cuda), differentiable in ``s``:
        ``out[b, u] = K sum_k sum_n hs[k, n] s[b, k, q]`` over the n with ``u + n - taps/2 = K q`` -- zero-stuffing by K,
        filtering and summing the bands, in polyphase form.  A clip's result is bit for bit what it is alone, also when
        the batch pads it with zeros behind its end.  Checks as ``analysis``."""
        if not isinstance(s, torch.Tensor) or not s.dtype.is_floating_point or s.dim() != 3:
            raise ValueError(f"PQMF.synthesis: s has shape {tuple(getattr(s, 'shape', ()))!r}, expected a float tensor "
                             f"[B, {self.subbands}, Ts]")
        if s.shape[1] != self.subbands or s.shape[0] < 1 or s.shape[2] < 1:
            raise ValueError(f"PQMF.synthesis: s {tuple(s.shape)}: expected [B, {self.subbands}, Ts] (subbands = "
                             f"{self.subbands} channels, B and Ts at least 1)")
        _need_gpu(s)
        _, hs, _, hs_rev = self._tables(s.device)
        out = _Bank.apply(s.to(torch.float32).contiguous(), "synthesis", hs, hs_rev, self.subbands, self.taps,
                          float(self.subbands))
        return out.unsqueeze(1)


# ---- the `model.subbands` keys of train / generate
def model_options(model_cfg, where="model"):
    """The bank a model config asks for: None without ``model.subbands`` (the three ``pqmf_*`` keys then need it), else
    the checked ``PQMF.options()`` dict.  ``in_channels`` / ``out_channels`` that contradict K are a ValueError."""
    K = model_cfg.get("subbands")
    others = [k for k in MODEL_KEYS[1:] if model_cfg.get(k) is not None]
    if K is None:
        if others:
            raise ValueError(f"{where}.{others[0]} needs {where}.subbands")
        return None
    K, taps, cutoff, beta = check_options(K, 62 if model_cfg.get("pqmf_taps") is None else model_cfg.get("pqmf_taps"),
                                          model_cfg.get("pqmf_cutoff"),
                                          9.0 if model_cfg.get("pqmf_beta") is None else model_cfg.get("pqmf_beta"),
                                          where=f"{where}.subbands / {where}.pqmf_*")
    for key in ("in_channels", "out_channels"):
        if model_cfg.get(key) is not None and model_cfg.get(key) != K:
            raise ValueError(f"{where}.{key} = {model_cfg.get(key)!r} contradicts {where}.subbands = {K} (the network runs "
                             "on the K sub-bands)")
    return dict(subbands=K, taps=taps, cutoff=cutoff, beta=beta)


def network_config(model_cfg):
    """``model_cfg`` as the network is built from it: the ``MODEL_KEYS`` taken out, and with ``model.subbands = K``
    ``in_channels = out_channels = K`` and SaShiMi's ``L`` (the full-band clip length) divided by K.  A copy; without the
    keys an equal one."""
    cfg = {k: v for k, v in model_cfg.items() if k not in MODEL_KEYS}
    opts = model_options(model_cfg)
    if opts is not None:
        K = opts["subbands"]
        cfg["in_channels"] = cfg["out_channels"] = K
        if cfg.get("_name_", model_cfg.get("_name_")) == "sashimi" and "L" in cfg:
            if not _is_int(cfg["L"]) or cfg["L"] % K:
                raise ValueError(f"model.L = {cfg['L']!r} is not a multiple of model.subbands = {K}")
            cfg["L"] = cfg["L"] // K
    return cfg


def check_run(model_cfg, dataset_cfg, where="train"):
    """The checks of a multi-band run before a model is built (ValueError naming the key): K, the conditioner's stride
    ``prod(model.mel_upsample) K = dataset.hop_length`` on a mel-conditional model, the clip length a multiple of K and,
    on SaShiMi, ``length / K`` a multiple of the pooling product.  Returns ``model_options(model_cfg)``."""
    opts = model_options(model_cfg)
    if opts is None:
        return None
    K = opts["subbands"]
    length = dataset_cfg.get("segment_length")
    if not model_cfg.get("unconditional"):
        up = [int(v) for v in model_cfg.get("mel_upsample", [16, 16])]
        if int(np.prod(up)) * K != dataset_cfg.get("hop_length"):
            raise ValueError(f"{where}: model.mel_upsample = {up} with model.subbands = {K} upsamples a mel frame to "
                             f"{int(np.prod(up)) * K} samples, dataset.hop_length is {dataset_cfg.get('hop_length')!r} (the "
                             "conditioner runs at the sub-band rate: prod(mel_upsample) x subbands must be hop_length)")
    if length is not None and (not _is_int(length) or length < K or length % K):
        raise ValueError(f"{where}: dataset.segment_length = {length!r} is not a positive multiple of model.subbands = {K}")
    if model_cfg.get("_name_") == "sashimi":
        from .models.sashimi import pool_span
        span = pool_span(model_cfg.get("pool", [4, 4]))
        for key, n in (("dataset.segment_length", length if model_cfg.get("unconditional") else None),
                       ("model.L", model_cfg.get("L"))):
            if n is not None and (not _is_int(n) or n % K or (n // K) % span):
                raise ValueError(f"{where}: {key} = {n!r} with model.subbands = {K}: length / subbands must be a multiple of "
                                 f"{span}, the product of model.pool = {list(model_cfg.get('pool', [4, 4]))}")
        if not model_cfg.get("unconditional"):
            hop = dataset_cfg.get("hop_length")
            if _is_int(hop) and (hop // K) % span:
                raise ValueError(f"{where}: dataset.hop_length = {hop!r} with model.subbands = {K}: hop_length / subbands "
                                 f"must be a multiple of {span}, the product of model.pool (utterances of frames x hop "
                                 "samples must divide through every pooling stage)")
    return opts


def same_options(a, b):
    """Two ``pqmf`` entries (None: a full-band run) name the same bank."""
    if a is None or b is None:
        return a is None and b is None
    return all(k in a and k in b for k in ("subbands", "taps", "cutoff", "beta")) and \
        int(a["subbands"]) == int(b["subbands"]) and int(a["taps"]) == int(b["taps"]) and \
        float(a["cutoff"]) == float(b["cutoff"]) and float(a["beta"]) == float(b["beta"])


def resolve(model_cfg, entry, where="generate"):
    """The bank a run on a checkpoint uses: the ``model.subbands`` keys against the checkpoint's ``pqmf`` entry (None: it
    has none).  No keys -> the entry; keys that contradict the entry (or an entry-less checkpoint) -> ValueError.
    Returns the options dict or None."""
    if entry is not None and (not isinstance(entry, dict) or any(k not in entry for k in ("subbands", "taps", "cutoff", "beta"))):
        raise ValueError(f"the checkpoint's pqmf entry {entry!r} is not one this version writes")
    if model_cfg.get("subbands") is None:
        model_options(model_cfg)        # (pqmf_* keys without subbands)
        return None if entry is None else dict(entry)
    opts = model_options(model_cfg)
    if entry is None:
        raise ValueError(f"{where}: model.subbands = {opts['subbands']} contradicts the checkpoint, which holds no pqmf entry "
                         "(it was trained on the full band)")
    given = {"subbands": "subbands", "pqmf_taps": "taps", "pqmf_cutoff": "cutoff", "pqmf_beta": "beta"}
    for key, name in given.items():
        if model_cfg.get(key) is not None and float(opts[name]) != float(entry[name]):
            raise ValueError(f"{where}: model.{key} = {model_cfg.get(key)!r} contradicts the checkpoint, which was trained "
                             f"with {name} = {entry[name]!r}")
    return dict(entry)

"""GPU: the schedule sampler's scalar path with every group of four full.  An injected `noise` (and `known_noise`) that
is not 16-byte aligned sends the update, editing, resampling and jump kernels down their scalar path although
n = B C L is a multiple of 4 -- no other test reaches that combination (their scalar cases have n % 4 != 0).  Each run
must equal, bit for bit, the same call given an aligned copy of the same values; the aligned runs are pinned to their
per-step loops by the neighbouring test files."""
import pytest
import torch

from tests import cases
from tests.test_edit_sampling_gpu import DCFG, _edit_inputs, _mask
from tests.test_few_step_sampling_gpu import _inputs

pytestmark = pytest.mark.gpu

B, L = 2, 600
T, BETA_T = 50, 0.05


def _offset_by_one_float(t, gpu):
    """A contiguous device view of t's values that starts one float into a larger buffer (sampling.py keeps the offset)."""
    buf = torch.zeros(t.numel() + 4, device=gpu)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _runs(net):
    """(name, call(use_graph, noise, known_noise)) of every run of the issue; the noises are [rows, B, 1, L]."""
    from diffwave_sashimi_amd.sampling import (calc_diffusion_hyperparams, repaint_program, sampling_aligned,
                                               sampling_ddim, sampling_dpmpp)
    dh = calc_diffusion_hyperparams(T, 1e-4, BETA_T)
    y, _, _ = _edit_inputs(B, L, 1)
    mask = _mask(B, L)
    size = (B, 1, L)
    samplers = {"ddpm": (6, lambda **kw: sampling_aligned(net, size, DCFG, **kw)),
                "ddim": (8, lambda **kw: sampling_ddim(net, size, dh, 8, 0.5, **kw)),
                "dpmpp": (6, lambda **kw: sampling_dpmpp(net, size, dh, 6, **kw))}
    out = []
    for name, modes in (("ddpm", ("plain", "mask", "resample")), ("ddim", ("plain", "mask", "resample")),
                        ("dpmpp", ("resample",))):
        S, fn = samplers[name]
        for mode in modes:
            rows = len(repaint_program(S, 2, 2)) if mode == "resample" else S
            kw = {} if mode == "plain" else dict(known=y, mask=mask)
            if mode == "resample":
                kw["resample"] = (2, 2)
            out.append((f"{name}_{mode}", rows, mode != "plain", fn, kw))
    return out


def test_unaligned_noise_takes_the_scalar_path_and_changes_nothing(gpu):
    cfg, _, _, wseed, _, _ = cases.WAVENET_CASES["wn_tiny"]
    net = cases.build_ours(cfg, wseed).to(gpu)
    assert (B * L) % 4 == 0
    for name, rows, edited, fn, kw in _runs(net):
        x_T, noise = _inputs(B, L, rows)
        _, kz, _ = _edit_inputs(B, L, rows)
        noise, kz = noise.to(gpu), kz.to(gpu)
        assert noise.data_ptr() % 16 == 0 and kz.data_ptr() % 16 == 0
        off = dict(noise=_offset_by_one_float(noise, gpu))
        al = dict(noise=noise)
        if edited:
            off["known_noise"] = _offset_by_one_float(kz, gpu)
            al["known_noise"] = kz
        for g in (False, True):
            want = fn(x_T=x_T, use_graph=g, **al, **kw)
            got = fn(x_T=x_T, use_graph=g, **off, **kw)
            assert torch.equal(got, want), (name, g, float((got - want).abs().max()))

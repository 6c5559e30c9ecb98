"""GPU: the samplers with an adaptive prior (``prior_std=`` / ``dws_sampler_set_prior``), all bit for bit.

The anchor, which needs no new reference: a run with ``prior_std = sigma`` that draws its own noise equals the run WITHOUT
a prior that is handed ``x_T = fp32(sigma z_S)`` and ``noise[s] = fp32(sigma z_s)``, with ``z_s`` Philox stream s of the
seed (``dws_philox_normal``) in the numbering of sampling.py / sampler.hip: s for the update noise of step s, S for a
drawn x_T, S + 1 + s for the known-region noise, 2S + 1 for the q-sample start; v, V, V + 1 + v, 2V + 1 in a program run.

Cases: wn_tiny at L = 300 (float4 groups) and B = 3, L = 301 (the element-wise instances; with a seed list clips that are
no multiple of four long), wn_cond_tiny / ss_cond_tiny with sigma from the mel; S = 6 steps."""
import numpy as np
import pytest
import torch

from tests import cases
from tests.test_cfg_sampling_gpu import KINDS, S, _graphs, _sample, _schedule
from tests.test_clip_seeds_gpu import _plain

pytestmark = pytest.mark.gpu

SEED = 1234
SHAPES = [(2, 300), (3, 301)]


def _z(size, seed, stream, gpu):
    """Philox stream `stream` of a scalar seed over the whole batch, as the samplers draw it"""
    from diffwave_sashimi_amd import _lib
    z = torch.empty(size, device=gpu)
    _lib.check(_lib.load().dws_philox_normal(z.data_ptr(), z.numel(), seed, stream, _lib.current_stream()))
    return z


def _sigma(size, gpu, seed=3):
    B, C, L = size
    return (torch.rand(B, 1, L, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.1).to(gpu)


def _streams(size, gpu, rows, first=0, seed=SEED):
    """[rows, B, C, L]: Philox streams first .. first + rows - 1"""
    return torch.stack([_z(size, seed, first + r, gpu) for r in range(rows)])


# ------------------------------------------------------------------------------------------------------ 1. the anchor
@pytest.mark.parametrize("B,L", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_prior_run_is_the_plain_run_with_prescaled_noise(gpu, kind, B, L):
    net, _ = _plain("wn_tiny", gpu)
    steps, _, dh = _schedule(kind)
    n = len(steps)          # (the log-SNR spacing of the multistep kind may give fewer than S steps)
    size = (B, 1, L)
    sg = _sigma(size, gpu)
    more = dict(net_steps=np.arange(S, dtype=np.float32)) if kind == "ddpm" else {}     # the schedule entry on both sides
    got = _sample(net, kind, size, dh, seed=SEED, prior_std=sg, **more)
    x_T = sg * _z(size, SEED, n, gpu)
    z = None if kind == "dpmpp2m" else _streams(size, gpu, n)
    want = _sample(net, kind, size, dh, x_T=x_T, **({} if z is None else {"noise": sg * z}), **more)
    assert torch.equal(got, want) and torch.isfinite(got).all()
    assert not torch.equal(got, _sample(net, kind, size, dh, seed=SEED, **more))
    assert torch.equal(_sample(net, kind, size, dh, seed=SEED, prior_std=sg, use_graph=False, **more), got)
    if z is not None:       # injected noise is scaled too; an injected x_T is a state and is taken as it is
        assert torch.equal(_sample(net, kind, size, dh, x_T=x_T, noise=z, prior_std=sg, **more), got)
        assert torch.equal(_sample(net, kind, size, dh, x_T=x_T, noise=z, prior_std=sg, use_graph=False, **more), got)
    # sigma = 1 is the run without the argument ([B, C, L] is accepted as [B, 1, L] is)
    assert torch.equal(_sample(net, kind, size, dh, seed=SEED, prior_std=torch.ones(B, 1, L), **more),
                       _sample(net, kind, size, dh, seed=SEED, **more))


@pytest.mark.parametrize("name", ["wn_cond_tiny", "ss_cond_tiny"])
def test_sigma_from_the_mel_on_the_conditional_models(gpu, name):
    from diffwave_sashimi_amd import sampling as smp
    from diffwave_sashimi_amd.mel import prior_std_from_mel
    if name == "wn_cond_tiny":
        cfg, B, L, Tmel, wseed, iseed, _ = cases.WAVENET_COND_CASES[name]
    else:
        cfg, B, Tmel, wseed, iseed, _ = cases.SASHIMI_COND_CASES[name]
        L = cfg["L"]
    net = cases.build_ours(cfg, wseed).to(gpu)
    mel = cases.mel_inputs(B, Tmel, iseed).to(gpu)
    mel[0, :, 0] = float(np.log(1e-5))          # a silent frame: sigma = std_min over its hop
    size = (B, 1, L)
    sg = prior_std_from_mel(mel, 256, L, energy_max=7.0)
    assert float(sg.min()) == np.float32(0.1) and float(sg.max()) > 0.5
    dh = smp.calc_diffusion_hyperparams(50, 1e-4, 0.05)
    run = lambda **kw: smp.sampling_ddim(net, size, dh, S, eta=0.5, condition=mel, **kw)
    got = run(seed=SEED, prior_std=sg)
    want = run(x_T=sg * _z(size, SEED, S, gpu), noise=sg * _streams(size, gpu, S))
    assert torch.equal(got, want) and torch.isfinite(got).all()


# ---------------------------------------------------------------------------------------------------- 2. edited runs
@pytest.mark.parametrize("B,L", SHAPES)
@pytest.mark.parametrize("what", ["replace", "resample", "qsample"])
def test_every_noise_site_of_an_edited_run_is_scaled(gpu, what, B, L):
    """DDIM at eta 0.5.  replace: the known-region noise (stream S + 1 + s).  resample = (2, 2): a program of V visits,
    noise rows and streams numbered by the visit, the jump visits' noise scaled as well.  qsample: the start noise
    (stream 2S + 1) of a partial start at step 3."""
    from diffwave_sashimi_amd import sampling as smp
    net, _ = _plain("wn_tiny", gpu)
    _, _, dh = _schedule("ddim")
    size = (B, 1, L)
    sg = _sigma(size, gpu, seed=5)
    g = torch.Generator().manual_seed(9)
    known = torch.randn(B, 1, L, generator=g) * 0.3
    mask = smp.spans_to_mask(size, [(0, 90), (201, 250), (297, L)])
    run = lambda **kw: smp.sampling_ddim(net, size, dh, S, eta=0.5, **kw)
    if what == "qsample":
        edit = dict(x_start=known, start_step=3)
        got = run(seed=SEED, prior_std=sg, **edit)
        want = run(noise=sg * _streams(size, gpu, S), start_noise=sg * _z(size, SEED, 2 * S + 1, gpu), **edit)
        injected = run(noise=_streams(size, gpu, S), start_noise=_z(size, SEED, 2 * S + 1, gpu), prior_std=sg, **edit)
    else:
        edit = dict(known=known, mask=mask)
        if what == "resample":
            edit["resample"] = (2, 2)
            R = len(smp.repaint_program(S, 2, 2))
            assert R > S
        else:
            R = S
        z, zk, z_T = _streams(size, gpu, R), _streams(size, gpu, R, first=R + 1), _z(size, SEED, R, gpu)
        got = run(seed=SEED, prior_std=sg, **edit)
        want = run(x_T=sg * z_T, noise=sg * z, known_noise=sg * zk, **edit)
        injected = run(x_T=sg * z_T, noise=z, known_noise=zk, prior_std=sg, **edit)
        m = mask.expand(size)
        assert torch.equal(got.cpu()[m], known[m])
    assert torch.equal(got, want) and torch.isfinite(got).all()
    assert torch.equal(injected, got)
    assert not torch.equal(got, run(seed=SEED, **edit))
    assert torch.equal(run(seed=SEED, prior_std=sg, use_graph=False, **edit), got)


def test_the_multistep_kind_scales_its_known_region_noise(gpu):
    """DPM-Solver++(2M) draws no update noise, but its edited step draws the known-region noise."""
    from diffwave_sashimi_amd import sampling as smp
    net, L = _plain("wn_tiny", gpu)
    _, _, dh = _schedule("dpmpp2m")
    size = (2, 1, L)
    sg = _sigma(size, gpu, seed=6)
    known = torch.randn(2, 1, L, generator=torch.Generator().manual_seed(10)) * 0.3
    mask = smp.spans_to_mask(size, [(10, 150)])
    run = lambda **kw: smp.sampling_dpmpp(net, size, dh, S, known=known, mask=mask, **kw)
    n = len(smp.logsnr_steps(dh["Alpha_bar"], S))
    got = run(seed=SEED, prior_std=sg)
    want = run(x_T=sg * _z(size, SEED, n, gpu), known_noise=sg * _streams(size, gpu, n, first=n + 1))
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------- 3. per-clip seeds
@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_a_clip_with_its_seed_and_its_sigma_is_its_b1_run(gpu, kind):
    net, _ = _plain("wn_tiny", gpu)
    _, _, dh = _schedule(kind)
    B, L = 3, 301
    seeds = [11, 11, 2 ** 63 + 5]
    sg = _sigma((B, 1, L), gpu, seed=7)
    out = _sample(net, kind, (B, 1, L), dh, seed=seeds, prior_std=sg)
    for b, k in enumerate(seeds):
        assert torch.equal(out[b:b + 1], _sample(net, kind, (1, 1, L), dh, seed=k, prior_std=sg[b:b + 1])), b
    assert not torch.equal(out[0], out[1])          # one seed, two sigmas
    assert torch.equal(_sample(net, kind, (B, 1, L), dh, seed=seeds, prior_std=sg, use_graph=False), out)
    # the float4 instances of the per-clip form
    out4 = _sample(net, kind, (B, 1, 300), dh, seed=seeds, prior_std=sg[..., :300].contiguous())
    assert torch.equal(out4[2:3], _sample(net, kind, (1, 1, 300), dh, seed=seeds[2], prior_std=sg[2:3, :, :300].contiguous()))


# --------------------------------------------------------------------------------------------------------- 4. lengths
def test_ragged_batch_with_a_prior(gpu):
    """wn_cond_tiny, lengths [512, 300]: over [0, len_b) the run is the per-step loop (module calls with the same lengths,
    the numpy float32 DDIM update, noise pre-scaled by sigma); the padding comes back as exact zeros, and NaN in the
    padding of sigma reaches no valid position."""
    from diffwave_sashimi_amd import sampling as smp
    from diffwave_sashimi_amd.mel import prior_std_from_mel
    cfg, B, L, Tmel, wseed, iseed, _ = cases.WAVENET_COND_CASES["wn_cond_tiny"]
    net = cases.build_ours(cfg, wseed).to(gpu)
    lens = [L, 300]
    mel = cases.mel_inputs(B, Tmel, iseed).to(gpu)
    sg = prior_std_from_mel(mel, 256, L, energy_max=7.0)
    dirty = sg.clone()
    dirty[1, :, 300:] = float("nan")
    dh = smp.calc_diffusion_hyperparams(50, 1e-4, 0.05)
    tau = smp.ddim_steps(50, S)
    k = smp.ddim_coefficients(dh["Alpha_bar"], tau, 0.5)
    g = torch.Generator().manual_seed(77)
    x_T, noise = torch.randn(B, 1, L, generator=g), torch.randn(S, B, 1, L, generator=g)
    sg_h = sg.cpu().numpy()
    x = x_T.numpy().copy()
    for s in range(S - 1, -1, -1):
        with torch.no_grad():
            eps = net((torch.from_numpy(x).to(gpu), torch.full((B, 1), float(tau[s]), device=gpu)), mel_spec=mel,
                      lengths=lens).cpu().numpy()
        k1, k2, k3, k4, k5 = (np.float32(v) for v in k[:, s])
        u = (x - k1 * eps) / k2
        x = k3 * u + k4 * eps
        if s > 0 and k5 > 0:
            n = sg_h * noise[s].numpy()
            x = x + k5 * n
    assert x.dtype == np.float32
    want = torch.from_numpy(x).to(gpu)
    for use_graph in (True, False):
        got = smp.sampling_ddim(net, (B, 1, L), dh, S, eta=0.5, condition=mel, x_T=x_T, noise=noise, lengths=lens,
                                prior_std=dirty, use_graph=use_graph)
        for b, n in enumerate(lens):
            assert torch.equal(got[b, :, :n], want[b, :, :n]), (use_graph, b)
            assert torch.count_nonzero(got[b, :, n:]) == 0
        assert torch.isfinite(got).all()
    with pytest.raises(ValueError, match="finite and > 0"):       # NaN at a valid position is refused
        smp.sampling_ddim(net, (B, 1, L), dh, S, eta=0.5, condition=mel, lengths=[L, 301], prior_std=dirty)
    # a drawn run with per-clip seeds: the short clip is its own run at its own length
    seeds = [5, 6]
    both = smp.sampling_ddim(net, (B, 1, L), dh, S, eta=0.5, condition=mel, seed=seeds, lengths=lens, prior_std=dirty)
    assert torch.isfinite(both).all() and torch.count_nonzero(both[1, :, 300:]) == 0 and torch.count_nonzero(both[1, :, :300]) > 0


# ------------------------------------------------------------------------------------- 5. graphs, state and refusals
def test_prior_tables_replay_and_the_plain_path_is_untouched(gpu):
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd import sampling as smp
    net, L = _plain("wn_tiny", gpu)
    _, _, dh = _schedule("ddim")
    size = (3, 1, L)
    run = lambda **kw: smp.sampling_ddim(net, size, dh, S, eta=0.5, seed=7, **kw)
    s1, s2 = _sigma(size, gpu, 1), _sigma(size, gpu, 2)
    plain = run()
    a = run(prior_std=s1)
    base = _graphs(net)
    b = run(prior_std=s2)
    assert _graphs(net) == base                                     # another table of the same shape: a replay
    assert not torch.equal(a, b) and not torch.equal(a, plain)
    assert torch.equal(run(), plain) and _graphs(net) == base       # the prior was dropped: the plain bits, the plain graph
    assert torch.equal(run(prior_std=s1), a) and torch.equal(run(), plain) and torch.equal(run(prior_std=s2), b)
    assert _graphs(net) == base                                     # on / off / on: each form was captured once
    # with per-clip seeds: a form of its own, once
    c = smp.sampling_ddim(net, size, dh, S, eta=0.5, seed=[1, 2, 3], prior_std=s1)
    g2 = _graphs(net)
    assert g2 <= base + 1
    assert torch.equal(smp.sampling_ddim(net, size, dh, S, eta=0.5, seed=[1, 2, 3], prior_std=s1), c) and _graphs(net) == g2

    # the engine's own refusals, on the raw entry points
    lib, h, st = _lib.load(), net._handle, _lib.current_stream()
    dhs = smp.calc_diffusion_hyperparams(S, 1e-4, 0.05)
    tabs = [smp._host_table(dhs[k]) for k in ("Alpha", "Alpha_bar", "Sigma")]
    x0 = torch.randn(3, 1, L)
    x = x0.to(gpu).clone()
    table = s1.expand(size).contiguous()
    try:
        with pytest.raises(RuntimeError, match="dws_sampler_set_prior"):
            _lib.check(lib.dws_sampler_set_prior(h, table.data_ptr(), 2, L, st))        # the model is prepared for 3 clips
        with pytest.raises(RuntimeError, match="dws_sampler_set_prior"):
            _lib.check(lib.dws_sampler_set_prior(h, table.data_ptr(), 3, L - 1, st))
        _lib.check(lib.dws_sampler_set_prior(h, table.data_ptr(), 3, L, st))
        with pytest.raises(NotImplementedError, match="adaptive prior"):
            _lib.check(lib.dws_sampler_run(h, x.data_ptr(), tabs[0][1], tabs[1][1], tabs[2][1], S, 0, 1, 0, 1, st))
        with pytest.raises(NotImplementedError, match="adaptive prior"):
            _lib.check(lib.dws_sampler_steps(h, x.data_ptr(), tabs[0][1], tabs[1][1], tabs[2][1], S, S - 1, 1, 1, 1, st))
        with pytest.raises(NotImplementedError, match="adaptive prior"):
            _lib.check(lib.dws_sampler_set_cfg(h, 1, 1.5))                               # guidance onto a prior
        _lib.check(lib.dws_sampler_set_prior(h, None, 0, 0, st))
        _lib.check(lib.dws_sampler_set_cfg(h, 1, 1.5))
        with pytest.raises(NotImplementedError, match="classifier-free"):
            _lib.check(lib.dws_sampler_set_prior(h, table.data_ptr(), 3, L, st))        # a prior onto guidance
        _lib.check(lib.dws_sampler_set_cfg(h, 0, 0.0))
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), x0)                                                  # nothing ran
        _lib.check(lib.dws_sampler_set_prior(h, table.data_ptr(), 3, L, st))
        net._prepare(2, L)                                                               # another shape drops the table
        net._prepare(3, L)
        _lib.check(lib.dws_sampler_steps(h, x.data_ptr(), tabs[0][1], tabs[1][1], tabs[2][1], S, S - 1, 1, 1, 1, st))
        torch.cuda.synchronize()
        assert not torch.equal(x.cpu(), x0)
    finally:
        _lib.check(lib.dws_sampler_set_cfg(h, 0, 0.0))
        _lib.check(lib.dws_sampler_set_prior(h, None, 0, 0, st))
    with pytest.raises(ValueError, match="classifier-free"):
        smp.sampling_ddim(net, size, dh, S, eta=0.5, seed=7, prior_std=s1, labels=[0, 0, 0], cfg_scale=1.0)
    assert torch.equal(run(), plain) and torch.equal(run(prior_std=s1), a)              # the engine is usable as before
    assert torch.equal(smp.sampling(net, size, dhs, seed=7), smp.sampling(net, size, dhs, seed=7, prior_std=torch.ones(size)))

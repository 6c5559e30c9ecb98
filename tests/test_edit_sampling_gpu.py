"""GPU: the editing modes of `dws_sampler_run_edit` -- inpainting / continuation by known-region replacement and the
partial start -- against per-step loops written out with module calls and a numpy float32 update (bit for bit), against
the float64 oracle, and the graph cache behind them.  The loops follow the formulas of include/dws.h, not the kernel.
These pin the arithmetic, not the audio (no trained weights exist offline)."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.conftest import REL_TOL, rel_err
from tests.test_few_step_sampling_gpu import SIX, _eps, _graphs, _inputs, _net

pytestmark = pytest.mark.gpu

DCFG = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=SIX)


def _aligned():
    """(dh, steps, q) of the aligned six-step DDPM run."""
    from diffwave_sashimi_amd.sampling import align_steps, calc_diffusion_hyperparams, edit_coefficients
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05, beta=SIX, fast=True)
    return dh, align_steps(50, 1e-4, 0.05, SIX), edit_coefficients(dh["Alpha_bar"])


def _ddim(eta, S=8):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, ddim_coefficients, ddim_steps, edit_coefficients
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    tau = ddim_steps(50, S)
    return dh, tau, ddim_coefficients(dh["Alpha_bar"], tau, eta), edit_coefficients(dh["Alpha_bar"][tau])


def _mask(B, L, seed=0):
    """Two spans and one isolated sample per clip, different per clip, boundaries that are no multiples of 4."""
    m = torch.zeros(B, 1, L, dtype=torch.bool)
    for b in range(B):
        o = 7 * b + seed
        m[b, 0, 5 + o:41 + o] = True
        m[b, 0, L // 2 + 3 + o:L // 2 + 90 + o] = True
        m[b, 0, L - 10 - o] = True
    assert 0 < int(m.sum()) < m.numel() // 2
    return m


def _edit_inputs(B, L, S, seed=91):
    """known audio y [B,1,L], known-region noise [S,B,1,L], start noise [B,1,L]"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, L, generator=g) * 2 - 1, torch.randn(S, B, 1, L, generator=g),
            torch.randn(B, 1, L, generator=g))


def _loop(net, gpu, steps, x, noise, dh=None, k=None, mel=None, q=None, y=None, mask=None, kz=None, s0=None):
    """Steps s0..0 in numpy float32, every operation rounded once: the DDPM update of `dh` or the DDIM update of `k`
    with the network at steps[s]; then, where mask, x = (q1[s] y) + (q2[s] zk[s]) for s > 0 and x = y at s = 0."""
    x = x.numpy().copy()
    S = len(steps)
    for s in range(S - 1 if s0 is None else s0, -1, -1):
        eps = _eps(net, x, float(steps[s]), gpu, mel)
        if k is None:
            a_t, ab_t = np.float32(dh["Alpha"][s]), np.float32(dh["Alpha_bar"][s])
            c1 = (np.float32(1) - a_t) / np.sqrt(np.float32(1) - ab_t)
            x = (x - c1 * eps) / np.sqrt(a_t)
            if s > 0:
                x = x + np.float32(dh["Sigma"][s]) * noise[s].numpy()
        else:
            k1, k2, k3, k4, k5 = (np.float32(v) for v in k[:, s])
            u = (x - k1 * eps) / k2
            x = k3 * u + k4 * eps
            if s > 0 and k5 > 0:
                x = x + k5 * noise[s].numpy()
        if mask is not None:
            rep = (q[0, s] * y.numpy()) + (q[1, s] * kz[s].numpy()) if s > 0 else y.numpy()
            x = np.where(mask.numpy(), rep, x)
        assert x.dtype == np.float32
    return torch.from_numpy(x).to(gpu)


def _qsample(q, s0, x, z0):
    return torch.from_numpy((q[2, s0] * x.numpy()) + (q[3, s0] * z0.numpy()))


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_off_means_off(gpu, kind):
    """All-zero mask, start_step = S-1, state as given: the unedited run, bit for bit."""
    from diffwave_sashimi_amd.sampling import sampling, sampling_ddim
    net, B, L, _ = _net(kind, gpu)
    dh, steps, _ = _aligned()
    dht, tau, _, _ = _ddim(0.5)
    y, _, _ = _edit_inputs(B, L, 8)
    zero = torch.zeros(B, 1, L, dtype=torch.bool)
    for g in (True, False):
        x_T, noise = _inputs(B, L, 6)
        a = sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise, net_steps=steps, use_graph=g)
        b = sampling(net, (B, 1, L), dh, noise=noise, net_steps=steps, use_graph=g, known=y, mask=zero, x_start=x_T,
                     start_step=5, start_noise=False)
        assert torch.equal(a, b), (g, float((a - b).abs().max()))
        a = sampling(net, (B, 1, L), dh, seed=5, net_steps=steps, use_graph=g)
        b = sampling(net, (B, 1, L), dh, seed=5, net_steps=steps, use_graph=g, known=y, mask=zero)
        assert torch.equal(a, b), g
        x_T, noise = _inputs(B, L, 8)
        a = sampling_ddim(net, (B, 1, L), dht, 8, 0.5, x_T=x_T, noise=noise, use_graph=g)
        b = sampling_ddim(net, (B, 1, L), dht, 8, 0.5, noise=noise, use_graph=g, known=y, mask=zero, x_start=x_T,
                          start_step=7, start_noise=False)
        assert torch.equal(a, b), g
        a = sampling_ddim(net, (B, 1, L), dht, 8, 0.5, seed=6, use_graph=g)
        b = sampling_ddim(net, (B, 1, L), dht, 8, 0.5, seed=6, use_graph=g, known=y, mask=zero)
        assert torch.equal(a, b), g


@pytest.mark.parametrize("kind", ["wavenet", "sashimi", "sashimi_cond"])
def test_inpainting_equals_its_per_step_loop_ddpm(gpu, kind):
    from diffwave_sashimi_amd.sampling import sampling_aligned
    net, B, L, mel = _net(kind, gpu)
    dh, steps, q = _aligned()
    x_T, noise = _inputs(B, L, 6)
    y, kz, _ = _edit_inputs(B, L, 6)
    mask = _mask(B, L)
    want = _loop(net, gpu, steps, x_T, noise, dh=dh, mel=mel, q=q, y=y, mask=mask, kz=kz)
    for g in (True, False):
        got = sampling_aligned(net, (B, 1, L), DCFG, mel, x_T=x_T, noise=noise, use_graph=g, known=y, mask=mask,
                               known_noise=kz)
        assert torch.equal(got, want), (g, float((got - want).abs().max()))
        assert torch.equal(got[mask.to(gpu)], y.to(gpu)[mask.to(gpu)])           # known samples survive exactly
    plain = sampling_aligned(net, (B, 1, L), DCFG, mel, x_T=x_T, noise=noise)
    assert not torch.equal(plain, want)


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_inpainting_equals_its_per_step_loop_ddim(gpu, kind, eta):
    from diffwave_sashimi_amd.sampling import sampling_ddim
    net, B, L, _ = _net(kind, gpu)
    dh, tau, k, q = _ddim(eta)
    x_T, noise = _inputs(B, L, 8)
    y, kz, _ = _edit_inputs(B, L, 8)
    mask = _mask(B, L, seed=2)
    want = _loop(net, gpu, tau, x_T, noise, k=k, q=q, y=y, mask=mask, kz=kz)
    for g in (True, False):
        got = sampling_ddim(net, (B, 1, L), dh, 8, eta, x_T=x_T, noise=noise, use_graph=g, known=y, mask=mask,
                            known_noise=kz)
        assert torch.equal(got, want), (g, float((got - want).abs().max()))
        assert torch.equal(got[mask.to(gpu)], y.to(gpu)[mask.to(gpu)])


def test_inpainting_scalar_path_and_all_ones_mask(gpu):
    """B C L = 3 x 601 is no multiple of 4: the scalar path.  With an all-ones mask the output is `known` whatever the
    weights."""
    from diffwave_sashimi_amd.sampling import sampling_aligned, sampling_ddim
    cfg, _, _, wseed, _, _ = cases.WAVENET_CASES["wn_c64"]
    net = cases.build_ours(cfg, wseed).to(gpu)
    B, L = 3, 601
    assert (B * L) % 4 != 0
    dh, steps, q = _aligned()
    x_T, noise = _inputs(B, L, 6)
    y, kz, _ = _edit_inputs(B, L, 6)
    mask = _mask(B, L)
    want = _loop(net, gpu, steps, x_T, noise, dh=dh, q=q, y=y, mask=mask, kz=kz)
    for g in (True, False):
        got = sampling_aligned(net, (B, 1, L), DCFG, x_T=x_T, noise=noise, use_graph=g, known=y, mask=mask,
                               known_noise=kz)
        assert torch.equal(got, want), (g, float((got - want).abs().max()))
    dht, tau, k, qd = _ddim(0.5)
    x_T8, noise8 = _inputs(B, L, 8)
    _, kz8, _ = _edit_inputs(B, L, 8)
    want = _loop(net, gpu, tau, x_T8, noise8, k=k, q=qd, y=y, mask=mask, kz=kz8)
    got = sampling_ddim(net, (B, 1, L), dht, 8, 0.5, x_T=x_T8, noise=noise8, known=y, mask=mask, known_noise=kz8)
    assert torch.equal(got, want), float((got - want).abs().max())
    ones = torch.ones(1, 1, L)                                   # 0/1 numbers, broadcast over the batch
    for g in (True, False):
        assert torch.equal(sampling_aligned(net, (B, 1, L), DCFG, seed=3, use_graph=g, known=y, mask=ones), y.to(gpu))
        assert torch.equal(sampling_ddim(net, (B, 1, L), dht, 8, 0.5, seed=3, use_graph=g, known=y, mask=ones), y.to(gpu))


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_partial_start_equals_its_loop(gpu, kind):
    from diffwave_sashimi_amd.sampling import sampling_aligned, sampling_ddim
    net, B, L, _ = _net(kind, gpu)
    dh, steps, q = _aligned()
    x, noise = _inputs(B, L, 6)
    _, _, z0 = _edit_inputs(B, L, 6)
    full = sampling_aligned(net, (B, 1, L), DCFG, x_T=x, noise=noise)
    for s0 in (0, 2, 5):
        want = _loop(net, gpu, steps, x, noise, dh=dh, s0=s0)
        wantq = _loop(net, gpu, steps, _qsample(q, s0, x, z0), noise, dh=dh, s0=s0)
        for g in (True, False):
            got = sampling_aligned(net, (B, 1, L), DCFG, noise=noise, use_graph=g, x_start=x, start_step=s0,
                                   start_noise=False)
            assert torch.equal(got, want), (s0, g, float((got - want).abs().max()))
            got = sampling_aligned(net, (B, 1, L), DCFG, noise=noise, use_graph=g, x_start=x, start_step=s0,
                                   start_noise=z0)
            assert torch.equal(got, wantq), (s0, g, float((got - wantq).abs().max()))
        assert torch.equal(want, full) == (s0 == 5)              # s0 = S-1 as given is x_T=
    dht, tau, k, qd = _ddim(0.5)
    x8, noise8 = _inputs(B, L, 8)
    wantq = _loop(net, gpu, tau, _qsample(qd, 2, x8, z0), noise8, k=k, s0=2)
    got = sampling_ddim(net, (B, 1, L), dht, 8, 0.5, noise=noise8, x_start=x8, start_step=2, start_noise=z0)
    assert torch.equal(got, wantq), float((got - wantq).abs().max())


def test_combined_inpainting_partial_start_and_mel(gpu):
    from diffwave_sashimi_amd.sampling import sampling_aligned
    net, B, L, mel = _net("sashimi_cond", gpu)
    dh, steps, q = _aligned()
    x, noise = _inputs(B, L, 6)
    y, kz, z0 = _edit_inputs(B, L, 6)
    mask = _mask(B, L, seed=1)
    want = _loop(net, gpu, steps, _qsample(q, 3, x, z0), noise, dh=dh, mel=mel, q=q, y=y, mask=mask, kz=kz, s0=3)
    for g in (True, False):
        got = sampling_aligned(net, (B, 1, L), DCFG, mel, noise=noise, use_graph=g, known=y, mask=mask, known_noise=kz,
                               x_start=x, start_step=3, start_noise=z0)
        assert torch.equal(got, want), (g, float((got - want).abs().max()))


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_seeded_runs(gpu, kind):
    from diffwave_sashimi_amd.sampling import sampling_aligned, sampling_ddim
    net, B, L, _ = _net(kind, gpu)
    dht = _ddim(0.5)[0]
    y, _, _ = _edit_inputs(B, L, 6)
    mask = _mask(B, L)
    md = mask.to(gpu)
    runs = (lambda seed, g, **kw: sampling_aligned(net, (B, 1, L), DCFG, seed=seed, use_graph=g, **kw),
            lambda seed, g, **kw: sampling_ddim(net, (B, 1, L), dht, 8, 0.5, seed=seed, use_graph=g, **kw))
    for run in runs:
        a = run(11, True, known=y, mask=mask)
        assert torch.equal(a, run(11, False, known=y, mask=mask)) and torch.equal(a, run(11, True, known=y, mask=mask))
        b = run(12, True, known=y, mask=mask)
        assert torch.isfinite(a).all() and not torch.equal(a[~md], b[~md])
        assert torch.equal(a[md], y.to(gpu)[md]) and torch.equal(b[md], y.to(gpu)[md])
        c = run(11, True, x_start=y, start_step=3)                       # seeded q-sample start
        assert torch.equal(c, run(11, False, x_start=y, start_step=3)) and torch.isfinite(c).all()
        assert not torch.equal(c, run(11, True, x_start=y, start_step=3, start_noise=False))
        assert not torch.equal(c, run(12, True, x_start=y, start_step=3))
        d = run(11, True, known=y, mask=mask, x_start=y, start_step=3)
        assert torch.equal(d, run(11, False, known=y, mask=mask, x_start=y, start_step=3))


def test_float64_oracle(gpu):
    """wn_tiny, aligned six steps, half-clip continuation plus a q-sample start at step 3, against the same loop in
    float64.  rel_err over the free samples only (the kept ones are exact and would only dilute the measure); the mask
    keeps half of every clip, so half of every clip is compared."""
    from diffwave_sashimi_amd.sampling import sampling, spans_to_mask
    from oracle import wavenet as own
    cfg, B, L, wseed, _, _ = cases.WAVENET_CASES["wn_tiny"]
    net = cases.build_ours(cfg, wseed).to(gpu)
    sd64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu())
            for k, v in net.state_dict().items()}
    dh, steps, q = _aligned()
    x, noise = _inputs(B, L, 6)
    y, kz, z0 = _edit_inputs(B, L, 6)
    mask = spans_to_mask((B, 1, L), [[0, L // 2]])
    assert int(mask.sum()) * 2 <= L
    got = sampling(net, (B, 1, L), dh, noise=noise, net_steps=steps, known=y, mask=mask, known_noise=kz, x_start=x,
                   start_step=3, start_noise=z0)
    al, ab, sg = (dh[k].double() for k in ("Alpha", "Alpha_bar", "Sigma"))
    lv = dh["Alpha_bar"].double()
    xd = torch.sqrt(lv[3]) * x.double() + torch.sqrt(1 - lv[3]) * z0.double()
    with torch.no_grad():
        for s in range(3, -1, -1):
            eps = own.wavenet_forward(sd64, cfg, xd, torch.full((B, 1), float(steps[s]), dtype=torch.float64))
            xd = (xd - (1 - al[s]) / torch.sqrt(1 - ab[s]) * eps) / torch.sqrt(al[s])
            if s > 0:
                xd = xd + sg[s] * noise[s].double()
                rep = torch.sqrt(lv[s - 1]) * y.double() + torch.sqrt(1 - lv[s - 1]) * kz[s].double()
            else:
                rep = y.double()
            xd = torch.where(mask, rep, xd)
    free = ~mask.expand(B, 1, L)
    err = rel_err(got.cpu()[free], xd[free])
    print(f"edited trajectory vs float64 oracle, free samples: rel_err {err:.3e}")
    assert err < REL_TOL, err
    assert torch.equal(got.cpu()[~free], y[~free])


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_graph_cache(gpu, kind):
    """A new seed, output tensor, known clip, mask or start step replays the edited graph; edited and unedited calls
    alternate on one model without a capture and stay correct."""
    from diffwave_sashimi_amd.sampling import sampling_aligned
    net, B, L, _ = _net(kind, gpu)
    run = lambda g, **kw: sampling_aligned(net, (B, 1, L), DCFG, use_graph=g, **kw)
    y1, _, _ = _edit_inputs(B, L, 6, seed=1)
    y2, _, _ = _edit_inputs(B, L, 6, seed=2)
    m1, m2 = _mask(B, L, seed=0), _mask(B, L, seed=3)
    calls = [dict(seed=11, known=y1, mask=m1), dict(seed=12, known=y2, mask=m2),
             dict(seed=13, known=y2, mask=m1, x_start=y1, start_step=3),
             dict(seed=14, known=y1, mask=m2, x_start=y2, start_step=1, start_noise=False)]
    plain = run(True, seed=21)                                   # the unedited graph exists from here on
    n0 = _graphs(net)
    outs = [run(True, **calls[0])]
    n1 = _graphs(net)
    assert n1 == n0 + 1
    outs += [run(True, **kw) for kw in calls[1:]]
    assert _graphs(net) == n1
    assert len({o.data_ptr() for o in outs}) == len(outs) and not torch.equal(outs[0], outs[1])
    for o, kw in zip(outs, calls):
        assert torch.equal(o, run(False, **kw))
    n2 = _graphs(net)
    for _ in range(2):                                           # alternating: both graphs stay current
        assert torch.equal(run(True, seed=21), plain)
        assert torch.equal(run(True, **calls[2]), outs[2])
    assert _graphs(net) == n2 and torch.equal(plain, run(False, seed=21))


@pytest.mark.parametrize("precision", ["f32", "bf16x6"])
def test_continuation_at_the_vocoder_size(gpu, precision):
    """BASELINE config 4's network and shape (B = 32, L = 16000, mel [1, 80, 63]), aligned S = 6, continuation of the first
    8000 samples.  f32: bit-equal to the loop.  bf16x6: finite, kept samples exact, free samples within
    test_aligned_at_the_vocoder_size's bound for this network (1e-5, measured there on unedited runs: the unedited error
    of this run is computed and printed beside the edited one)."""
    from diffwave_sashimi_amd.sampling import sampling_aligned, spans_to_mask
    cfg, _, Tmel, wseed, iseed = cases.SASHIMI_C4
    B, L = 32, 16000
    net = cases.build_ours(cfg, wseed).to(gpu)
    mel = cases.mel_inputs(1, Tmel, iseed).to(gpu)
    x_T, noise = _inputs(B, L, 6)
    y, kz, _ = _edit_inputs(B, L, 6)
    mask = spans_to_mask((B, 1, L), [[0, 8000]])
    kw = dict(x_T=x_T, noise=noise)
    ekw = dict(kw, known=y, mask=mask, known_noise=kz)
    f32 = sampling_aligned(net, (B, 1, L), DCFG, mel, **ekw)
    free = ~mask.expand(B, 1, L).to(gpu)
    assert torch.equal(f32[~free], y.to(gpu)[~free])
    if precision == "f32":
        dh, steps, q = _aligned()
        want = _loop(net, gpu, steps, x_T, noise, dh=dh, mel=mel, q=q, y=y, mask=mask.expand(B, 1, L), kz=kz)
        assert torch.equal(f32, want), float((f32 - want).abs().max())
    else:
        plain32 = sampling_aligned(net, (B, 1, L), DCFG, mel, **kw)
        net.set_option("precision", "bf16x6")
        got = sampling_aligned(net, (B, 1, L), DCFG, mel, **ekw)
        plain = sampling_aligned(net, (B, 1, L), DCFG, mel, **kw)
        assert torch.isfinite(got).all() and torch.equal(got[~free], y.to(gpu)[~free])
        err, err_plain = rel_err(got[free], f32[free]), rel_err(plain, plain32)
        print(f"bf16x6 vs f32 at the vocoder size: edited (free samples) {err:.3e}, unedited {err_plain:.3e}")
        assert err < 1e-5, (err, err_plain)


@pytest.mark.parametrize("mode", ["inpaint", "start"])
def test_generate_cli_editing(tmp_path, gpu, mode):
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import _worker, load_config, local_path_name
    from tests.test_generate_cli import _tree
    d = _tree(tmp_path / "conf")
    data = tmp_path / "data"
    os.makedirs(data)
    g = torch.Generator().manual_seed(8)
    clip = (torch.rand(1600, generator=g) * 2 - 1).numpy().astype(np.float32)
    wavfile.write(str(data / "clip.wav"), 16000, clip)
    ov = ["model=wavenet", "model.res_channels=64", "model.skip_channels=64", "model.num_res_layers=4",
          "model.dilation_cycle=4", "dataset.segment_length=1600", f"dataset.data_path={data}", "generate.n_samples=2",
          "generate.ckpt_iter=init", "generate.seed=4", "generate.sampler=aligned",
          "diffusion.beta=[0.0001,0.001,0.01,0.05,0.2,0.5]"]
    if mode == "inpaint":
        ov += ["generate.known_name=clip", "generate.keep=[[0,801],[1203,1210]]"]
    else:
        ov += ["generate.start_name=clip", "generate.start_step=2"]
    cfg = load_config(d, ov)
    root = str(tmp_path / "exp")
    _worker(0, cfg, root)
    outdir = os.path.join(root, local_path_name(None, cfg["model"], cfg["diffusion"], cfg["dataset"]), "waveforms", "0")
    assert sorted(os.listdir(outdir)) == ["0k_0.wav", "0k_1.wav"]
    ws = []
    for f in ("0k_0.wav", "0k_1.wav"):
        sr, w = wavfile.read(os.path.join(outdir, f))
        assert sr == 16000 and w.dtype == np.float32 and w.shape == (1600,) and np.isfinite(w).all()
        ws.append(w)
    if mode == "inpaint":
        for w in ws:
            assert np.array_equal(w[:801], clip[:801]) and np.array_equal(w[1203:1210], clip[1203:1210])
        assert not np.array_equal(ws[0][801:1203], ws[1][801:1203])     # its own noise per clip
    else:
        assert not np.array_equal(ws[0], ws[1]) and not np.array_equal(ws[0], clip)

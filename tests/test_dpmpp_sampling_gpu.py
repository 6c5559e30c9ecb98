"""GPU: the DPM-Solver++(2M) sampler (`DWS_SAMPLER_DPMPP2M` on `dws_sampler_run_schedule` / `_edit` / `_program`) against
per-step loops written out with module calls and a numpy float32 update (bit for bit): plain, partial-start, inpainting
and resampling runs, the history buffer and its valid word across runs, the graph cache, the float64 oracle and the CLI.
The loops follow the formulas of include/dws.h, not the kernels.  These pin the arithmetic, not the audio (no trained
weights exist offline)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.conftest import REL_TOL, rel_err
from tests.test_edit_sampling_gpu import _edit_inputs, _mask, _qsample
from tests.test_few_step_sampling_gpu import _eps, _graphs, _inputs, _net
from tests.test_resample_sampling_gpu import _kept, _philox

pytestmark = pytest.mark.gpu

T, BETA_T, S = 50, 0.05, 6


def _tables(spacing="logsnr", steps=S):
    """(dh, tau, m [5][S], q [4][S]) of `steps` steps of T = 50, beta in [1e-4, 0.05]."""
    from diffwave_sashimi_amd.sampling import (calc_diffusion_hyperparams, ddim_steps, dpmpp_coefficients,
                                               edit_coefficients, logsnr_steps)
    dh = calc_diffusion_hyperparams(T, 1e-4, BETA_T)
    tau = logsnr_steps(dh["Alpha_bar"], steps) if spacing == "logsnr" else ddim_steps(T, steps)
    return dh, tau, dpmpp_coefficients(dh["Alpha_bar"], tau), edit_coefficients(dh["Alpha_bar"][tau])


def _loop(net, gpu, tau, m, x, mel=None, s0=None, q=None, y=None, mask=None, kz=None, prog=None, jc=None, noise=None):
    """The visits of a run in order (`prog`, or the countdown s0 .. 0), numpy float32, every operation rounded once.
    Entry i is visit v = V-1-i (v = s in a countdown).  Reverse visit at step s:
      p = m1 eps; d = x - p; x0 = d / m2; D = x0; with history and m5 != 0: g = x0 - hist; e = m5 g; D = x0 + e
      a = m3 x; b = m4 D; x = a + b; hist = x0
    then, where mask, x = (q1[s] y) + (q2[s] kz[v]) for s > 0 and x = y at s = 0.  Jump visit:
    x = (ja[v] x) + (jb[v] noise[v]) and the history is dropped.  The first visit has no history.
    Returns (x, the x0 of the last reverse visit)."""
    x = x.numpy().copy()
    visits = [int(a) for a in prog] if prog is not None else list(range(len(tau) - 1 if s0 is None else s0, -1, -1))
    V, hist, x0 = len(visits), None, None
    for i, a in enumerate(visits):
        v = V - 1 - i
        if a < 0:
            x = (jc[0, v] * x) + (jc[1, v] * noise[v].numpy())
            hist = None
            assert x.dtype == np.float32
            continue
        s = a
        eps = _eps(net, x, float(tau[s]), gpu, mel)
        m1, m2, m3, m4, m5 = (np.float32(c) for c in m[:, s])
        p = m1 * eps
        d = x - p
        x0 = d / m2
        D = x0
        if hist is not None and m5 != 0:
            g = x0 - hist
            e = m5 * g
            D = x0 + e
        a_, b_ = m3 * x, m4 * D
        x = a_ + b_
        hist = x0
        if mask is not None:
            rep = (q[0, s] * y.numpy()) + (q[1, s] * kz[v].numpy()) if s > 0 else y.numpy()
            x = np.where(mask.numpy(), rep, x)
        assert x.dtype == np.float32 and x0.dtype == np.float32
    return torch.from_numpy(x).to(gpu), torch.from_numpy(x0).to(gpu)


def _run(net, B, L, dh, steps=S, cond=None, **kw):
    from diffwave_sashimi_amd.sampling import sampling_dpmpp
    return sampling_dpmpp(net, (B, 1, L), dh, steps, cond, **kw)


@pytest.mark.parametrize("kind", ["wavenet", "sashimi", "sashimi_cond"])
def test_dpmpp_equals_its_per_step_loop(gpu, kind):
    net, B, L, mel = _net(kind, gpu)
    dh, tau, m, _ = _tables()
    assert tau == [0, 1, 3, 9, 23, 49] and np.all(m[4, 1:5] > 0)
    x_T, _ = _inputs(B, L, 1)
    want, x0_last = _loop(net, gpu, tau, m, x_T, mel)
    for g in (True, False):
        got = _run(net, B, L, dh, cond=mel, x_T=x_T, use_graph=g)
        assert torch.equal(got, want), (g, float((got - want).abs().max()))
        assert torch.equal(got, x0_last)                       # m3[0] = 0, m4[0] = 1, m5[0] = 0: the last step returns x0
    # the second-order terms are in: the same tables with the m5 row zeroed (first order throughout) differ
    first, _ = _loop(net, gpu, tau, np.concatenate([m[:4], np.zeros_like(m[4:])]), x_T, mel)
    assert not torch.equal(first, want)
    # uniform spacing is another run, and equals its loop
    dh, tau_u, m_u, _ = _tables("uniform")
    assert tau_u != tau
    want_u, _ = _loop(net, gpu, tau_u, m_u, x_T, mel)
    got = _run(net, B, L, dh, cond=mel, x_T=x_T, spacing="uniform")
    assert torch.equal(got, want_u), float((got - want_u).abs().max())


def test_scalar_path(gpu):
    """B C L = 3 x 601 is no multiple of 4: the scalar path of the plain, the edited and the resampling kernel."""
    from diffwave_sashimi_amd.sampling import jump_coefficients, repaint_program
    cfg, _, _, wseed, _, _ = cases.WAVENET_CASES["wn_c64"]
    net = cases.build_ours(cfg, wseed).to(gpu)
    B, L = 3, 601
    assert (B * L) % 4 != 0
    dh, tau, m, q = _tables()
    prog = repaint_program(S, 2, 2)
    jc = jump_coefficients(dh["Alpha_bar"][tau], prog)
    x_T, noise = _inputs(B, L, len(prog))
    y, kz, _ = _edit_inputs(B, L, len(prog))
    mask = _mask(B, L)
    plain, _ = _loop(net, gpu, tau, m, x_T)
    edited, _ = _loop(net, gpu, tau, m, x_T, q=q, y=y, mask=mask, kz=kz)
    resampled, _ = _loop(net, gpu, tau, m, x_T, q=q, y=y, mask=mask, kz=kz, prog=prog, jc=jc, noise=noise)
    for g in (True, False):
        got = _run(net, B, L, dh, x_T=x_T, use_graph=g)
        assert torch.equal(got, plain), (g, float((got - plain).abs().max()))
        got = _run(net, B, L, dh, x_T=x_T, use_graph=g, known=y, mask=mask, known_noise=kz[:S])
        assert torch.equal(got, edited), (g, float((got - edited).abs().max()))
        got = _run(net, B, L, dh, x_T=x_T, use_graph=g, known=y, mask=mask, known_noise=kz, resample=(2, 2), noise=noise)
        assert torch.equal(got, resampled), (g, float((got - resampled).abs().max()))
        ones = torch.ones(1, 1, L)                               # all known: the output is `known` whatever the weights
        assert torch.equal(_run(net, B, L, dh, seed=3, use_graph=g, known=y, mask=ones), y.to(gpu))


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_partial_start_begins_first_order(gpu, kind):
    """start_step = 3 of S = 6: m5[3] != 0, but the first executed step has no history -- the device decides, the tables
    are those of the whole run."""
    net, B, L, _ = _net(kind, gpu)
    dh, tau, m, q = _tables()
    assert m[4, 3] != 0
    x, _ = _inputs(B, L, 1)
    _, _, z0 = _edit_inputs(B, L, 1)
    want, _ = _loop(net, gpu, tau, m, x, s0=3)
    wantq, _ = _loop(net, gpu, tau, m, _qsample(q, 3, x, z0), s0=3)
    full = _run(net, B, L, dh, x_T=x)                            # leaves history and a set valid word behind
    for g in (True, False):
        got = _run(net, B, L, dh, use_graph=g, x_start=x, start_step=3, start_noise=False)
        assert torch.equal(got, want), (g, float((got - want).abs().max()))
        got = _run(net, B, L, dh, use_graph=g, x_start=x, start_step=3, start_noise=z0)
        assert torch.equal(got, wantq), (g, float((got - wantq).abs().max()))
    assert not torch.equal(full, want)
    for s0 in (0, 5):
        want, _ = _loop(net, gpu, tau, m, x, s0=s0)
        got = _run(net, B, L, dh, x_start=x, start_step=s0, start_noise=False)
        assert torch.equal(got, want), s0
        assert torch.equal(want, full) == (s0 == 5)              # s0 = S-1 as given is x_T=


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_no_history_crosses_runs(gpu, kind):
    """Run A then run B (another x_T) on one model: B equals B on a fresh model, graph and eager -- a stale history or a
    stale valid word would show.  Alternating with DDIM on the same model leaves DDIM's result bitwise what it was."""
    from diffwave_sashimi_amd.sampling import sampling_ddim
    net, B, L, _ = _net(kind, gpu)
    fresh, _, _, _ = _net(kind, gpu)
    dh, tau, m, _ = _tables()
    xa, _ = _inputs(B, L, 1, seed=1)
    xb, noise = _inputs(B, L, 8, seed=2)
    ddim = lambda n: sampling_ddim(n, (B, 1, L), dh, 8, 0.5, x_T=xb, noise=noise)
    want_ddim = ddim(net)                                        # before this model has run the multistep kind
    want_b = _run(fresh, B, L, dh, x_T=xb)
    assert torch.equal(want_b, _loop(fresh, gpu, tau, m, xb)[0])
    for g in (True, False):
        a = _run(net, B, L, dh, x_T=xa, use_graph=g)
        b = _run(net, B, L, dh, x_T=xb, use_graph=g)
        assert torch.equal(b, want_b) and not torch.equal(a, b), g
        assert torch.equal(ddim(net), want_ddim), g
        assert torch.equal(_run(net, B, L, dh, x_T=xb, use_graph=g), want_b), g
        # a partial start right behind a whole run, and a whole run right behind it
        p = _run(net, B, L, dh, x_start=xa, start_step=2, start_noise=False, use_graph=g)
        assert torch.equal(p, _loop(net, gpu, tau, m, xa, s0=2)[0]), g
        assert torch.equal(_run(net, B, L, dh, x_T=xb, use_graph=g), want_b), g
    assert torch.equal(ddim(net), want_ddim)


@pytest.mark.parametrize("kind", ["wavenet", "sashimi", "sashimi_cond"])
def test_inpainting_equals_its_per_step_loop(gpu, kind):
    """The replacement comes after the update; the history holds the network's prediction, not the replaced state."""
    net, B, L, mel = _net(kind, gpu)
    dh, tau, m, q = _tables()
    x_T, _ = _inputs(B, L, 1)
    y, kz, z0 = _edit_inputs(B, L, S)
    mask = _mask(B, L)
    md = mask.to(gpu)
    want, _ = _loop(net, gpu, tau, m, x_T, mel, q=q, y=y, mask=mask, kz=kz)
    for g in (True, False):
        got = _run(net, B, L, dh, cond=mel, x_T=x_T, use_graph=g, known=y, mask=mask, known_noise=kz)
        assert torch.equal(got, want), (g, float((got - want).abs().max()))
        assert torch.equal(got[md], y.to(gpu)[md])               # known samples survive exactly
    assert not torch.equal(_run(net, B, L, dh, cond=mel, x_T=x_T), want)
    # with a q-sample partial start on top
    want, _ = _loop(net, gpu, tau, m, _qsample(q, 3, x_T, z0), mel, s0=3, q=q, y=y, mask=mask, kz=kz)
    got = _run(net, B, L, dh, cond=mel, known=y, mask=mask, known_noise=kz, x_start=x_T, start_step=3, start_noise=z0)
    assert torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize("kind", ["wavenet", "sashimi", "sashimi_cond"])
def test_resampling_equals_its_per_visit_loop(gpu, kind):
    """repaint_program(6, 2, 2) = [5, 4, 3, 2, -2, 3, 2, 1, 0, -2, 1, 0]: a jump clears the history, so the visits at
    steps 3 and 1 behind the jumps are first order although m5 != 0 there."""
    from diffwave_sashimi_amd.sampling import jump_coefficients, program_streams, repaint_program
    net, B, L, mel = _net(kind, gpu)
    dh, tau, m, q = _tables()
    prog = repaint_program(S, 2, 2)
    assert prog.tolist() == [5, 4, 3, 2, -2, 3, 2, 1, 0, -2, 1, 0] and m[4, 3] != 0 and m[4, 1] != 0
    jc = jump_coefficients(dh["Alpha_bar"][tau], prog)
    V = len(prog)
    x_T, noise = _inputs(B, L, V)
    y, kz, _ = _edit_inputs(B, L, V)
    mask = _mask(B, L, seed=2)
    kw = dict(known=y, mask=mask, resample=(2, 2))
    want, _ = _loop(net, gpu, tau, m, x_T, mel, q=q, y=y, mask=mask, kz=kz, prog=prog, jc=jc, noise=noise)
    for g in (True, False):
        got = _run(net, B, L, dh, cond=mel, x_T=x_T, use_graph=g, known_noise=kz, noise=noise, **kw)
        assert torch.equal(got, want), (g, float((got - want).abs().max()))
        assert _kept(got, y, mask, gpu)
    # only the rows of jump visits are read: other rows of `noise` do not matter
    other = noise.clone()
    other[[v for v in range(V) if prog[V - 1 - v] >= 0]] = 7.0
    assert torch.equal(_run(net, B, L, dh, cond=mel, x_T=x_T, known_noise=kz, noise=other, **kw), want)
    # seeded: graph == eager, and the documented streams (visit v -> v, known region -> V + 1 + v, x_T -> V)
    a = _run(net, B, L, dh, cond=mel, seed=31, use_graph=True, **kw)
    assert torch.isfinite(a).all() and _kept(a, y, mask, gpu)
    assert torch.equal(a, _run(net, B, L, dh, cond=mel, seed=31, use_graph=False, **kw))
    st = program_streams(prog)
    n = B * L
    pn = torch.stack([_philox(n, 31, int(st["visit"][v]), gpu) for v in range(V)]).view(V, B, 1, L)
    pk = torch.stack([_philox(n, 31, V + 1 + v, gpu) for v in range(V)]).view(V, B, 1, L)
    b = _run(net, B, L, dh, cond=mel, x_T=_philox(n, 31, st["x_T"], gpu).view(B, 1, L), noise=pn, known_noise=pk, **kw)
    assert torch.equal(a, b), float((a - b).abs().max())
    free = ~mask.expand(B, 1, L).to(gpu)
    assert not torch.equal(a[free], _run(net, B, L, dh, cond=mel, seed=32, **kw)[free])
    # resamples = 1 is the edited run
    one = dict(known=y, mask=mask, known_noise=kz[:S], x_T=x_T)
    assert torch.equal(_run(net, B, L, dh, cond=mel, resample=(2, 1), **one), _run(net, B, L, dh, cond=mel, **one))


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_graph_cache(gpu, kind):
    """One capture per kind of step (plain, edited, resampling) on first use; a new seed, x, known clip, mask, start step
    or program of the same V replays, and the three alternate without a capture."""
    from diffwave_sashimi_amd.sampling import repaint_program
    net, B, L, _ = _net(kind, gpu)
    dh = _tables()[0]
    run = lambda g, **kw: _run(net, B, L, dh, use_graph=g, **kw)
    y1, _, _ = _edit_inputs(B, L, 1, seed=1)
    y2, _, _ = _edit_inputs(B, L, 1, seed=2)
    m1, m2 = _mask(B, L, seed=0), _mask(B, L, seed=3)
    x1, _ = _inputs(B, L, 1, seed=4)
    n0 = _graphs(net)
    plain = [dict(seed=21), dict(seed=22), dict(x_T=x1), dict(seed=23, x_start=y1, start_step=3),
             dict(x_start=y2, start_step=1, start_noise=False)]
    outs = [run(True, **plain[0])]
    n1 = _graphs(net)
    assert n1 == n0 + 1
    outs += [run(True, **kw) for kw in plain[1:]]
    assert _graphs(net) == n1                                    # seed, x and start step replay the plain graph
    edited = [dict(seed=11, known=y1, mask=m1), dict(seed=12, known=y2, mask=m2),
              dict(seed=13, known=y2, mask=m1, x_start=y1, start_step=3),
              dict(seed=14, known=y1, mask=m2, x_start=y2, start_step=1, start_noise=False)]
    outs.append(run(True, **edited[0]))
    n2 = _graphs(net)
    assert n2 == n1 + 1
    outs += [run(True, **kw) for kw in edited[1:]]
    assert _graphs(net) == n2
    # four programs of V = 10 visits: (1, 2) and (2, 3) from K = 4, (4, 2) from K = 5, (3, 2) over the whole run
    same_V = [dict(resample=(1, 2), x_start=y1, start_step=3), dict(resample=(2, 3), x_start=y2, start_step=3),
              dict(resample=(4, 2), x_start=y1, start_step=4, start_noise=False), dict(resample=(3, 2))]
    progs = [repaint_program(S, *kw["resample"], kw.get("start_step")).tolist() for kw in same_V]
    assert [len(p) for p in progs] == [10] * 4 and len({tuple(p) for p in progs}) == 4
    first = dict(seed=11, known=y1, mask=m1, **same_V[0])
    resampled = [first, dict(first, seed=12), dict(first, known=y2), dict(first, mask=m2)]
    resampled += [dict(seed=13, known=y2, mask=m2, **kw) for kw in same_V[1:]]
    outs.append(run(True, **resampled[0]))
    n3 = _graphs(net)
    assert n3 == n2 + 1
    outs += [run(True, **kw) for kw in resampled[1:]]
    assert _graphs(net) == n3
    calls = plain + edited + resampled
    assert len({o.data_ptr() for o in outs}) == len(outs)
    for o, kw in zip(outs, calls):
        assert torch.equal(o, run(False, **kw)), kw.keys()
    n4 = _graphs(net)
    for _ in range(2):                                           # alternating: all three graphs stay current
        for i in (0, len(plain), len(plain) + len(edited) + 4, 3, len(plain) + 2):
            assert torch.equal(run(True, **calls[i]), outs[i]), i
    assert _graphs(net) == n4
    other = run(True, seed=11, known=y1, mask=m1, resample=(2, 2))                      # V = 12: a new capture
    assert _graphs(net) == n4 + 1 and torch.equal(other, run(False, seed=11, known=y1, mask=m1, resample=(2, 2)))


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_determinism(gpu, kind):
    """With x_T given nothing is drawn: two seeds give one result.  Seed-driven: the seed draws x_T only."""
    net, B, L, _ = _net(kind, gpu)
    dh = _tables()[0]
    x_T, _ = _inputs(B, L, 1)
    for g in (True, False):
        a = _run(net, B, L, dh, x_T=x_T, seed=1, use_graph=g)
        assert torch.equal(a, _run(net, B, L, dh, x_T=x_T, seed=2, use_graph=g)), g
    a, b = _run(net, B, L, dh, seed=3, use_graph=True), _run(net, B, L, dh, seed=3, use_graph=False)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert not torch.equal(a, _run(net, B, L, dh, seed=4))
    assert torch.equal(a, _run(net, B, L, dh, x_T=_philox(B * L, 3, S, gpu).view(B, 1, L)))   # a drawn x_T is stream S


def test_abi_bad_input_is_invalid_before_anything_is_enqueued(gpu):
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.sampling import _prepare_run
    net, B, L, _ = _net("wavenet", gpu)
    dh, tau, m, _ = _tables()
    good = _run(net, B, L, dh, seed=5)
    n0 = _graphs(net)
    lib = _lib.load()
    fp = ctypes.POINTER(ctypes.c_float)
    steps = np.asarray(tau, dtype=np.float32)
    noise = torch.zeros(S, B, 1, L, device=gpu)

    def call(coef, nz=None):
        coef = np.ascontiguousarray(coef, dtype=np.float32)
        with torch.no_grad():
            x, init, _, seed = _prepare_run(net, (B, 1, L), S, None, None, None, 5)
        rc = lib.dws_sampler_run_schedule(net._handle, x.data_ptr(), _lib.DWS_SAMPLER_DPMPP2M, S, steps.ctypes.data_as(fp),
                                          coef.ctypes.data_as(fp), _lib.ptr(nz), seed, init, 1, _lib.current_stream())
        torch.cuda.synchronize()
        return rc, x

    rc, x = call(m)
    assert rc == _lib.DWS_OK and torch.equal(x, good)
    for r, s, v in ((0, 2, np.nan), (3, 1, np.inf), (1, 4, 0.0), (1, 0, -0.5), (4, 2, -0.25), (4, 0, -np.inf)):
        bad = m.copy()
        bad[r, s] = v
        rc, _ = call(bad)
        assert rc == _lib.DWS_ERR_INVALID, (r, s, v, rc)
        with pytest.raises(RuntimeError):
            _lib.check(rc)
    rc, _ = call(m, noise)                                       # noise outside a program run
    assert rc == _lib.DWS_ERR_INVALID
    assert _graphs(net) == n0                                    # refused before anything was captured
    rc, x = call(m)
    assert rc == _lib.DWS_OK and torch.equal(x, good)


def test_float64_oracle(gpu):
    """wn_tiny, the six log-SNR steps of T = 50, against the same loop in float64 (module in float64, the float32 tables
    as doubles).  DDIM (eta = 0) over the same steps against its float64 loop is printed beside it."""
    from diffwave_sashimi_amd.sampling import ddim_coefficients, sampling_ddim
    from oracle import wavenet as own
    cfg, B, L, wseed, _, _ = cases.WAVENET_CASES["wn_tiny"]
    net = cases.build_ours(cfg, wseed).to(gpu)
    sd64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu())
            for k, v in net.state_dict().items()}
    dh, tau, m, _ = _tables()
    k = ddim_coefficients(dh["Alpha_bar"], tau, 0.0)
    x_T, _ = _inputs(B, L, 1)
    got = _run(net, B, L, dh, x_T=x_T)
    got_ddim = sampling_ddim(net, (B, 1, L), dh, tau, 0.0, x_T=x_T)
    md, kd = torch.from_numpy(m).double(), torch.from_numpy(k).double()
    x, xd, hist = x_T.double(), x_T.double(), None
    with torch.no_grad():
        for s in range(S - 1, -1, -1):
            step = torch.full((B, 1), float(tau[s]), dtype=torch.float64)
            x0 = (x - md[0, s] * own.wavenet_forward(sd64, cfg, x, step)) / md[1, s]
            D = x0 + md[4, s] * (x0 - hist) if hist is not None and md[4, s] != 0 else x0
            x = md[2, s] * x + md[3, s] * D
            hist = x0
            eps = own.wavenet_forward(sd64, cfg, xd, step)
            xd = kd[2, s] * ((xd - kd[0, s] * eps) / kd[1, s]) + kd[3, s] * eps
    err, err_ddim = rel_err(got, x), rel_err(got_ddim, xd)
    print(f"six-step trajectory vs float64 oracle: DPM-Solver++(2M) rel_err {err:.3e}, DDIM rel_err {err_ddim:.3e}")
    assert err < REL_TOL, (err, err_ddim)


def test_generate_cli(tmp_path, gpu, capsys):
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import _worker, load_config, local_path_name
    from tests.test_generate_cli import _tree
    d = _tree(tmp_path / "conf")
    data = tmp_path / "data"
    os.makedirs(data)
    g = torch.Generator().manual_seed(8)
    clip = (torch.rand(1600, generator=g) * 2 - 1).numpy().astype(np.float32)
    wavfile.write(str(data / "clip.wav"), 16000, clip)
    base = ["model=wavenet", "model.res_channels=64", "model.skip_channels=64", "model.num_res_layers=4",
            "model.dilation_cycle=4", "dataset.segment_length=1600", f"dataset.data_path={data}", "generate.n_samples=2",
            "generate.ckpt_iter=init", "generate.seed=4", "generate.sampler=dpmpp2m"]
    runs = [(["generate.steps=6"], "6 network evaluations per batch", "plain"),
            # 21 log-SNR targets of the tree's T = 200 schedule collide once: 20 evaluations
            (["generate.steps=21"], "20 network evaluations per batch", "dedup"),
            (["generate.steps=6", "generate.spacing=uniform", "generate.known_name=clip",
              "generate.keep=[[0,801],[1203,1210]]", "generate.resample_jump=2", "generate.resample_n=2"],
             "10 network evaluations per batch", "resample")]
    for i, (ov, line, mode) in enumerate(runs):
        cfg = load_config(d, base + ov)
        root = str(tmp_path / f"exp{i}")
        _worker(0, cfg, root)
        out = capsys.readouterr().out
        assert "sampler dpmpp2m" in out and line in out, out
        outdir = os.path.join(root, local_path_name(None, cfg["model"], cfg["diffusion"], cfg["dataset"]), "waveforms", "0")
        assert sorted(os.listdir(outdir)) == ["0k_0.wav", "0k_1.wav"]
        ws = []
        for f in ("0k_0.wav", "0k_1.wav"):
            sr, w = wavfile.read(os.path.join(outdir, f))
            assert sr == 16000 and w.dtype == np.float32 and w.shape == (1600,) and np.isfinite(w).all()
            ws.append(w)
        if mode == "resample":
            for w in ws:
                assert np.array_equal(w[:801], clip[:801]) and np.array_equal(w[1203:1210], clip[1203:1210])
            assert not np.array_equal(ws[0][801:1203], ws[1][801:1203])
        else:
            assert not np.array_equal(ws[0], ws[1])              # its own x_T per clip

"""GPU: RePaint's resampling (`dws_sampler_run_program`) -- programs of reverse and jump visits on top of the inpainting
run -- against per-visit loops written out with module calls and a numpy float32 update (bit for bit), the trivial
program against today's edited run, the Philox stream assignment against `dws_philox_normal`, the float64 oracle, and the
graph cache.  The loops follow the formulas of include/dws.h, not the kernels.  These pin the arithmetic, not the audio
(no trained weights exist offline)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.conftest import REL_TOL, rel_err
from tests.test_edit_sampling_gpu import DCFG, _aligned, _ddim, _edit_inputs, _mask, _qsample
from tests.test_few_step_sampling_gpu import _eps, _graphs, _inputs, _net

pytestmark = pytest.mark.gpu

PROGRAMS = [(1, 2), (2, 2), (2, 3)]


def _program(S, jr, levels, start_step=None):
    """(visit_step [V], jump_coef [2][V]) of resample=jr over a run with `levels`."""
    from diffwave_sashimi_amd.sampling import jump_coefficients, repaint_program
    prog = repaint_program(S, jr[0], jr[1], start_step)
    return prog, jump_coefficients(levels, prog, start_step)


def _loop(net, gpu, steps, prog, jc, x, noise, kz, q, y, mask, dh=None, k=None, mel=None):
    """The visits of `prog` in order, numpy float32, every operation rounded once.  Entry i is visit v = V-1-i.  Reverse
    visit at step s: the network at steps[s], the DDPM update of `dh` or the DDIM update of `k` with noise[v], then where
    mask x = (q1[s] y) + (q2[s] kz[v]) for s > 0 and x = y at s = 0.  Jump visit: x = (ja[v] x) + (jb[v] noise[v])."""
    x = x.numpy().copy()
    V = len(prog)
    yn, mn = y.numpy(), mask.numpy()
    for i, a in enumerate(int(a) for a in prog):
        v = V - 1 - i
        if a < 0:
            x = (jc[0, v] * x) + (jc[1, v] * noise[v].numpy())
            assert x.dtype == np.float32
            continue
        s = a
        eps = _eps(net, x, float(steps[s]), gpu, mel)
        if k is None:
            a_t, ab_t = np.float32(dh["Alpha"][s]), np.float32(dh["Alpha_bar"][s])
            c1 = (np.float32(1) - a_t) / np.sqrt(np.float32(1) - ab_t)
            x = (x - c1 * eps) / np.sqrt(a_t)
            if s > 0:
                x = x + np.float32(dh["Sigma"][s]) * noise[v].numpy()
        else:
            k1, k2, k3, k4, k5 = (np.float32(c) for c in k[:, s])
            u = (x - k1 * eps) / k2
            x = k3 * u + k4 * eps
            if s > 0 and k5 > 0:
                x = x + k5 * noise[v].numpy()
        rep = (q[0, s] * yn) + (q[1, s] * kz[v].numpy()) if s > 0 else yn
        x = np.where(mn, rep, x)
        assert x.dtype == np.float32
    return torch.from_numpy(x).to(gpu)


def _kept(got, y, mask, gpu):
    md = mask.expand(got.shape).to(gpu)
    return torch.equal(got[md], y.expand(got.shape).to(gpu)[md])


@pytest.mark.parametrize("jr", PROGRAMS)
@pytest.mark.parametrize("kind", ["wavenet", "sashimi", "sashimi_cond"])
def test_resampling_equals_its_per_visit_loop_ddpm(gpu, kind, jr):
    from diffwave_sashimi_amd.sampling import sampling_aligned
    net, B, L, mel = _net(kind, gpu)
    dh, steps, q = _aligned()
    prog, jc = _program(6, jr, dh["Alpha_bar"])
    V = len(prog)
    x_T, noise = _inputs(B, L, V)
    y, kz, _ = _edit_inputs(B, L, V)
    mask = _mask(B, L)
    want = _loop(net, gpu, steps, prog, jc, x_T, noise, kz, q, y, mask, dh=dh, mel=mel)
    for g in (True, False):
        got = sampling_aligned(net, (B, 1, L), DCFG, mel, x_T=x_T, noise=noise, use_graph=g, known=y, mask=mask,
                               known_noise=kz, resample=jr)
        assert torch.equal(got, want), (g, float((got - want).abs().max()))
        assert _kept(got, y, mask, gpu)                                  # known samples survive exactly


@pytest.mark.parametrize("jr", PROGRAMS)
@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("kind", ["wavenet", "sashimi", "sashimi_cond"])
def test_resampling_equals_its_per_visit_loop_ddim(gpu, kind, eta, jr):
    from diffwave_sashimi_amd.sampling import sampling_ddim
    net, B, L, mel = _net(kind, gpu)
    dh, tau, k, q = _ddim(eta)
    prog, jc = _program(8, jr, dh["Alpha_bar"][tau])
    V = len(prog)
    x_T, noise = _inputs(B, L, V)
    y, kz, _ = _edit_inputs(B, L, V)
    mask = _mask(B, L, seed=2)
    want = _loop(net, gpu, tau, prog, jc, x_T, noise, kz, q, y, mask, k=k, mel=mel)
    for g in (True, False):
        got = sampling_ddim(net, (B, 1, L), dh, 8, eta, mel, x_T=x_T, noise=noise, use_graph=g, known=y, mask=mask,
                            known_noise=kz, resample=jr)
        assert torch.equal(got, want), (g, float((got - want).abs().max()))
        assert _kept(got, y, mask, gpu)


@pytest.mark.parametrize("jr", PROGRAMS)
def test_resampling_scalar_path(gpu, jr):
    """B C L = 3 x 601 is no multiple of 4: the scalar path of both new kernels; the mask's spans straddle the groups of
    four in every test of this file."""
    from diffwave_sashimi_amd.sampling import sampling_aligned, sampling_ddim
    cfg, _, _, wseed, _, _ = cases.WAVENET_CASES["wn_c64"]
    net = cases.build_ours(cfg, wseed).to(gpu)
    B, L = 3, 601
    assert (B * L) % 4 != 0
    mask = _mask(B, L)
    dh, steps, q = _aligned()
    prog, jc = _program(6, jr, dh["Alpha_bar"])
    x_T, noise = _inputs(B, L, len(prog))
    y, kz, _ = _edit_inputs(B, L, len(prog))
    want = _loop(net, gpu, steps, prog, jc, x_T, noise, kz, q, y, mask, dh=dh)
    for g in (True, False):
        got = sampling_aligned(net, (B, 1, L), DCFG, x_T=x_T, noise=noise, use_graph=g, known=y, mask=mask,
                               known_noise=kz, resample=jr)
        assert torch.equal(got, want), (g, float((got - want).abs().max()))
        assert _kept(got, y, mask, gpu)
    dht, tau, k, qd = _ddim(0.5)
    prog, jc = _program(8, jr, dht["Alpha_bar"][tau])
    x_T, noise = _inputs(B, L, len(prog))
    _, kz, _ = _edit_inputs(B, L, len(prog))
    want = _loop(net, gpu, tau, prog, jc, x_T, noise, kz, qd, y, mask, k=k)
    for g in (True, False):
        got = sampling_ddim(net, (B, 1, L), dht, 8, 0.5, x_T=x_T, noise=noise, use_graph=g, known=y, mask=mask,
                            known_noise=kz, resample=jr)
        assert torch.equal(got, want), (g, float((got - want).abs().max()))
        assert _kept(got, y, mask, gpu)
    ones = torch.ones(1, 1, L)                                   # all known: the output is `known` whatever the weights
    for g in (True, False):
        assert torch.equal(sampling_aligned(net, (B, 1, L), DCFG, seed=3, use_graph=g, known=y, mask=ones, resample=jr),
                           y.to(gpu))


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_one_resample_is_todays_run(gpu, kind):
    """resample=(j, 1) is the program K-1 .. 0 with v = s: the edited run, bit for bit, injected and seeded (seeded over
    the whole run, where V = S and every stream id coincides; with a partial start V = K < S numbers the known-region
    and start streams differently, so that case is compared with injected noise)."""
    from diffwave_sashimi_amd.sampling import sampling_aligned, sampling_ddim
    net, B, L, _ = _net(kind, gpu)
    dht = _ddim(0.5)[0]
    mask = _mask(B, L)
    runs = ((6, lambda **kw: sampling_aligned(net, (B, 1, L), DCFG, **kw)),
            (8, lambda **kw: sampling_ddim(net, (B, 1, L), dht, 8, 0.5, **kw)))
    for S, run in runs:
        x_T, noise = _inputs(B, L, S)
        y, kz, z0 = _edit_inputs(B, L, S)
        for g in (True, False):
            for j in (1, 2, S + 1):
                kw = dict(x_T=x_T, noise=noise, known=y, mask=mask, known_noise=kz, use_graph=g)
                assert torch.equal(run(**kw), run(resample=(j, 1), **kw)), (S, g, j)
                kw = dict(seed=17, known=y, mask=mask, use_graph=g)
                assert torch.equal(run(**kw), run(resample=(j, 1), **kw)), (S, g, j)
                # partial start: V = K = 4 rows, which are rows 0..3 of the edited run's (v = s)
                kw = dict(known=y, mask=mask, x_start=x_T, start_step=3, start_noise=z0, use_graph=g)
                assert torch.equal(run(noise=noise, known_noise=kz, **kw),
                                   run(resample=(j, 1), noise=noise[:4], known_noise=kz[:4], **kw)), (S, g, j)


def _abi_run(net, size, kind, steps, coef, q, seed, known, mask, prog=None, jc=None, use_graph=1, start_step=None):
    """dws_sampler_run_edit (prog None) or dws_sampler_run_program, seeded, x_T drawn.  Returns (status, x)."""
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.sampling import _prepare_run
    lib = _lib.load()
    fp = ctypes.POINTER(ctypes.c_float)
    steps = np.ascontiguousarray(steps, dtype=np.float32)
    coef, q = np.ascontiguousarray(coef, dtype=np.float32), np.ascontiguousarray(q, dtype=np.float32)
    S = len(steps)
    with torch.no_grad():
        x, init, _, seed = _prepare_run(net, size, S, None, None, None, seed)
    ed = _lib.SamplerEdit(q.ctypes.data_as(fp), known.data_ptr(), mask.data_ptr(), None, None,
                          S - 1 if start_step is None else start_step, _lib.DWS_START_AS_GIVEN)
    head = (net._handle, x.data_ptr(), kind, S, steps.ctypes.data_as(fp), coef.ctypes.data_as(fp))
    tail = (None, seed, init, use_graph, ctypes.byref(ed), _lib.current_stream())
    if prog is None:
        rc = lib.dws_sampler_run_edit(*head, *tail)
    else:
        prog, jc = np.ascontiguousarray(prog, dtype=np.int32), np.ascontiguousarray(jc, dtype=np.float32)
        assert jc.shape == (2, len(prog))
        rc = lib.dws_sampler_run_program(*head, len(prog), prog.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                         jc.ctypes.data_as(fp), *tail)
    torch.cuda.synchronize()
    return rc, x


def test_abi_trivial_program_is_run_edit_and_non_walks_are_invalid(gpu):
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.sampling import jump_coefficients
    net, B, L, _ = _net("wavenet", gpu)
    dh, steps, q = _aligned()
    coef = np.stack([dh[k].numpy() for k in ("Alpha", "Alpha_bar", "Sigma")])
    y, _, _ = _edit_inputs(B, L, 6)
    known = y.to(gpu).contiguous()
    mask = _mask(B, L).to(device=gpu, dtype=torch.uint8).contiguous()
    common = (net, (B, 1, L), _lib.DWS_SAMPLER_DDPM, steps, coef, q, 23, known, mask)
    trivial, zeros = [5, 4, 3, 2, 1, 0], np.zeros((2, 6), np.float32)
    for g in (1, 0):
        rc, a = _abi_run(*common, use_graph=g)
        assert rc == _lib.DWS_OK
        rc, b = _abi_run(*common, prog=trivial, jc=zeros, use_graph=g)
        assert rc == _lib.DWS_OK and torch.equal(a, b), g
    good = [5, 4, 3, 2, -2, 3, 2, 1, 0, -2, 1, 0]
    jc = jump_coefficients(dh["Alpha_bar"], good)
    rc, c = _abi_run(*common, prog=good, jc=jc)
    assert rc == _lib.DWS_OK and torch.isfinite(c).all() and not torch.equal(c, a)
    n0 = _graphs(net)

    def invalid(prog, jc=None, **kw):
        prog = list(prog)
        jc = np.full((2, len(prog)), 0.5, np.float32) if jc is None else jc
        rc, _ = _abi_run(*common, prog=prog, jc=jc, **kw)
        assert rc == _lib.DWS_ERR_INVALID, (prog, rc)
        with pytest.raises(RuntimeError):
            _lib.check(rc)

    invalid([4, 3, 2, 1, 0])                                     # the first reverse visit is not start_step
    invalid([5, 4, 3, 2, 1, 0], start_step=4)
    invalid([5, 4, 2, 1, 0])                                     # not one below the position reached
    invalid([5, 4, 3, 2, -2, 4, 3, 2, 1, 0])
    invalid([5, 4, -3, 5, 4, 3, 2, 1, 0])                        # lands above K = 6
    invalid([3, 2, -3, 4, 3, 2, 1, 0], start_step=3)             # lands above K = 4
    invalid([5, 4, 3, 2, 1])                                     # does not end in reverse step 0
    invalid([5, 4, 3, 2, 1, 0, -2])
    invalid([-2, 5, 4, 3, 2, 1, 0])                              # starts with a jump beyond K
    for bad in ((np.nan, 0.5), (0.5, np.inf), (0.0, 1.0), (-0.5, 0.5)):
        bjc = jc.copy()
        bjc[0, 7], bjc[1, 7] = bad                               # the jump at entry 4 is visit v = 7
        invalid(good, bjc)
    assert _graphs(net) == n0                                    # refused before anything was captured
    rc, d = _abi_run(*common, prog=good, jc=jc)                  # and the model still runs, to the same result
    assert rc == _lib.DWS_OK and torch.equal(c, d)


def _philox(n, seed, stream, gpu):
    from diffwave_sashimi_amd import _lib
    x = torch.empty(n, device=gpu, dtype=torch.float32)
    _lib.check(_lib.load().dws_philox_normal(x.data_ptr(), n, seed, stream, _lib.current_stream()))
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_seeded_streams_are_the_documented_ones(gpu, kind):
    """A seeded run equals the run whose x_T, noise, known_noise and start noise are dws_philox_normal at the documented
    stream ids: visit v -> v, known region after visit v -> V + 1 + v, x_T -> V, q-sample -> 2V + 1."""
    from diffwave_sashimi_amd.sampling import program_streams, repaint_program, sampling_aligned, sampling_ddim
    net, B, L, _ = _net(kind, gpu)
    dht = _ddim(0.5)[0]
    y, _, _ = _edit_inputs(B, L, 6)
    mask = _mask(B, L)
    md = mask.to(gpu)
    n = B * L
    runs = ((6, lambda **kw: sampling_aligned(net, (B, 1, L), DCFG, **kw)),
            (8, lambda **kw: sampling_ddim(net, (B, 1, L), dht, 8, 0.5, **kw)))
    for S, run in runs:
        for jr, s0 in (((2, 2), None), ((1, 3), None), ((2, 2), 4)):
            prog = repaint_program(S, jr[0], jr[1], s0)
            V = len(prog)
            st = program_streams(prog)
            assert st["x_T"] == V and st["start"] == 2 * V + 1
            seed = 31
            noise = torch.stack([_philox(n, seed, int(st["visit"][v]), gpu) for v in range(V)]).view(V, B, 1, L)
            kz = torch.stack([_philox(n, seed, V + 1 + v, gpu) for v in range(V)]).view(V, B, 1, L)
            ekw = dict(known=y, mask=mask, resample=jr)
            if s0 is None:
                seeded = dict(ekw, seed=seed)
                injected = dict(ekw, x_T=_philox(n, seed, V, gpu).view(B, 1, L), noise=noise, known_noise=kz)
            else:
                seeded = dict(ekw, seed=seed, x_start=y, start_step=s0)
                injected = dict(ekw, x_start=y, start_step=s0, start_noise=_philox(n, seed, 2 * V + 1, gpu).view(B, 1, L),
                                noise=noise, known_noise=kz)
            a = run(use_graph=True, **seeded)
            assert torch.isfinite(a).all() and _kept(a, y, mask, gpu)
            for g in (True, False):
                b = run(use_graph=g, **injected)
                assert torch.equal(a, b), (S, jr, s0, g, float((a - b).abs().max()))
            assert torch.equal(a, run(use_graph=False, **seeded))
            assert torch.equal(a, run(use_graph=True, **seeded))                         # one seed repeats
            other = run(use_graph=True, **dict(seeded, seed=seed + 1))
            assert not torch.equal(a[~md], other[~md]) and _kept(other, y, mask, gpu)    # two seeds differ


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_resampling_has_an_effect(gpu, kind):
    from diffwave_sashimi_amd.sampling import sampling_aligned
    net, B, L, _ = _net(kind, gpu)
    y, _, _ = _edit_inputs(B, L, 6)
    mask = _mask(B, L)
    md = mask.to(gpu)
    one = sampling_aligned(net, (B, 1, L), DCFG, seed=9, known=y, mask=mask, resample=(2, 1))
    two = sampling_aligned(net, (B, 1, L), DCFG, seed=9, known=y, mask=mask, resample=(2, 2))
    assert torch.isfinite(two).all() and not torch.equal(one[~md], two[~md])
    assert torch.equal(one[md], two[md])


def test_combined_resampling_partial_start_and_mel(gpu):
    from diffwave_sashimi_amd.sampling import sampling_aligned
    net, B, L, mel = _net("sashimi_cond", gpu)
    dh, steps, q = _aligned()
    prog, jc = _program(6, (2, 2), dh["Alpha_bar"], start_step=4)          # K = 5: jump points 0 and 2
    assert prog.tolist() == [4, 3, 2, -2, 3, 2, 1, 0, -2, 1, 0]
    V = len(prog)
    x, noise = _inputs(B, L, V)
    y, kz, z0 = _edit_inputs(B, L, V)
    mask = _mask(B, L, seed=1)
    want = _loop(net, gpu, steps, prog, jc, _qsample(q, 4, x, z0), noise, kz, q, y, mask, dh=dh, mel=mel)
    for g in (True, False):
        got = sampling_aligned(net, (B, 1, L), DCFG, mel, noise=noise, use_graph=g, known=y, mask=mask, known_noise=kz,
                               x_start=x, start_step=4, start_noise=z0, resample=(2, 2))
        assert torch.equal(got, want), (g, float((got - want).abs().max()))
        assert _kept(got, y, mask, gpu)


def test_float64_oracle(gpu):
    """The inputs of test_edit_sampling_gpu.test_float64_oracle (wn_tiny, aligned six steps, half-clip continuation, a
    q-sample start at step 3) under the program of (jump, resamples) = (1, 2): K = 4, jump points 0, 1, 2, seven network
    evaluations and three jumps, against the same walk in float64.  rel_err over the free samples."""
    from diffwave_sashimi_amd.sampling import repaint_program, sampling, spans_to_mask
    from oracle import wavenet as own
    cfg, B, L, wseed, _, _ = cases.WAVENET_CASES["wn_tiny"]
    net = cases.build_ours(cfg, wseed).to(gpu)
    sd64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu())
            for k, v in net.state_dict().items()}
    dh, steps, q = _aligned()
    prog = repaint_program(6, 1, 2, start_step=3)
    assert prog.tolist() == [3, 2, -1, 2, 1, -1, 1, 0, -1, 0]
    V = len(prog)
    x, noise = _inputs(B, L, V)
    y, kz, z0 = _edit_inputs(B, L, V)
    mask = spans_to_mask((B, 1, L), [[0, L // 2]])
    assert int(mask.sum()) * 2 <= L
    got = sampling(net, (B, 1, L), dh, noise=noise, net_steps=steps, known=y, mask=mask, known_noise=kz, x_start=x,
                   start_step=3, start_noise=z0, resample=(1, 2))
    al, ab, sg = (dh[k].double() for k in ("Alpha", "Alpha_bar", "Sigma"))
    P = torch.cat([torch.ones(1, dtype=torch.float64), dh["Alpha_bar"].double()])       # level of position k
    xd = torch.sqrt(P[4]) * x.double() + torch.sqrt(1 - P[4]) * z0.double()
    pos = 4
    with torch.no_grad():
        for i, a in enumerate(int(a) for a in prog):
            v = V - 1 - i
            if a < 0:
                ratio = P[pos - a] / P[pos]
                xd = torch.sqrt(ratio) * xd + torch.sqrt(1 - ratio) * noise[v].double()
                pos -= a
                continue
            s = pos = a
            eps = own.wavenet_forward(sd64, cfg, xd, torch.full((B, 1), float(steps[s]), dtype=torch.float64))
            xd = (xd - (1 - al[s]) / torch.sqrt(1 - ab[s]) * eps) / torch.sqrt(al[s])
            if s > 0:
                xd = xd + sg[s] * noise[v].double()
                rep = torch.sqrt(P[s]) * y.double() + torch.sqrt(1 - P[s]) * kz[v].double()
            else:
                rep = y.double()
            xd = torch.where(mask, rep, xd)
    free = ~mask.expand(B, 1, L)
    err = rel_err(got.cpu()[free], xd[free])
    print(f"resampled trajectory vs float64 oracle, free samples: rel_err {err:.3e}")
    assert err < REL_TOL, err
    assert torch.equal(got.cpu()[~free], y[~free])


@pytest.mark.parametrize("kind", ["wavenet", "sashimi"])
def test_graph_cache(gpu, kind):
    """After the first resampling call a new seed, output tensor, known clip, mask, start step or program of equal V
    replays the resampling graph; resampling, edited and unedited calls alternate on one model without a capture."""
    from diffwave_sashimi_amd.sampling import repaint_program, sampling_aligned
    net, B, L, _ = _net(kind, gpu)
    run = lambda g, **kw: sampling_aligned(net, (B, 1, L), DCFG, use_graph=g, **kw)
    y1, _, _ = _edit_inputs(B, L, 6, seed=1)
    y2, _, _ = _edit_inputs(B, L, 6, seed=2)
    m1, m2 = _mask(B, L, seed=0), _mask(B, L, seed=3)
    # four programs of V = 10 visits: (1, 2) and (2, 3) from K = 4, (4, 2) from K = 5, (3, 2) over the whole run
    same_V = [dict(resample=(1, 2), x_start=y1, start_step=3), dict(resample=(2, 3), x_start=y2, start_step=3),
              dict(resample=(4, 2), x_start=y1, start_step=4, start_noise=False), dict(resample=(3, 2))]
    progs = [repaint_program(6, *kw["resample"], kw.get("start_step")).tolist() for kw in same_V]
    assert [len(p) for p in progs] == [10] * 4 and len({tuple(p) for p in progs}) == 4
    plain = run(True, seed=21)                                   # the unedited graph
    edited = run(True, seed=22, known=y1, mask=m1)               # the edited graph
    n0 = _graphs(net)
    first = dict(seed=11, known=y1, mask=m1, **same_V[0])
    outs = [run(True, **first)]
    n1 = _graphs(net)
    assert n1 == n0 + 1                                          # the tap counts the third graph
    calls = [first, dict(first, seed=12), dict(first, known=y2), dict(first, mask=m2)]
    calls += [dict(seed=13, known=y2, mask=m2, **kw) for kw in same_V[1:]]               # start step and program, same V
    outs += [run(True, **kw) for kw in calls[1:]]
    assert _graphs(net) == n1
    assert len({o.data_ptr() for o in outs}) == len(outs)
    assert all(not torch.equal(outs[0], o) for o in outs[1:])
    for o, kw in zip(outs, calls):
        assert torch.equal(o, run(False, **kw))
    n2 = _graphs(net)
    for _ in range(2):                                           # alternating: all three graphs stay current
        assert torch.equal(run(True, seed=21), plain)
        assert torch.equal(run(True, **calls[-1]), outs[-1])
        assert torch.equal(run(True, seed=22, known=y1, mask=m1), edited)
    assert _graphs(net) == n2
    other = run(True, seed=11, known=y1, mask=m1, resample=(2, 2))                      # V = 12: a new capture
    assert _graphs(net) == n2 + 1 and torch.equal(other, run(False, seed=11, known=y1, mask=m1, resample=(2, 2)))


@pytest.mark.parametrize("precision", ["f32", "bf16x6"])
def test_resampling_at_the_vocoder_size(gpu, precision):
    """BASELINE config 4's network and shape (B = 32, L = 16000, mel [1, 80, 63]), aligned S = 6, continuation of the first
    8000 samples with resample=(2, 2): finite, kept samples exact, and the resampling changed the free samples."""
    from diffwave_sashimi_amd.sampling import sampling_aligned, spans_to_mask
    cfg, _, Tmel, wseed, iseed = cases.SASHIMI_C4
    B, L = 32, 16000
    net = cases.build_ours(cfg, wseed).to(gpu)
    if precision != "f32":
        net.set_option("precision", precision)
    mel = cases.mel_inputs(1, Tmel, iseed).to(gpu)
    y, _, _ = _edit_inputs(B, L, 1)
    mask = spans_to_mask((B, 1, L), [[0, 8000]])
    got = sampling_aligned(net, (B, 1, L), DCFG, mel, seed=5, known=y, mask=mask, resample=(2, 2))
    base = sampling_aligned(net, (B, 1, L), DCFG, mel, seed=5, known=y, mask=mask)
    free = ~mask.expand(B, 1, L).to(gpu)
    assert torch.isfinite(got).all() and torch.equal(got[~free], y.to(gpu)[~free])
    assert not torch.equal(got[free], base[free])
    assert torch.equal(got, sampling_aligned(net, (B, 1, L), DCFG, mel, seed=5, known=y, mask=mask, resample=(2, 2),
                                             use_graph=False))


@pytest.mark.parametrize("sampler", ["ddpm", "aligned", "ddim"])
def test_generate_cli_resampling(tmp_path, gpu, sampler, capsys):
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
          "generate.ckpt_iter=init", "generate.seed=4", f"generate.sampler={sampler}",
          "generate.known_name=clip", "generate.keep=[[0,801],[1203,1210]]", "generate.resample_jump=2",
          "generate.resample_n=2"]
    if sampler == "ddim":
        ov += ["generate.steps=6"]
    else:                                                        # six steps with every sampler: 6 + 1 * 2 * 2 evaluations
        ov += ["diffusion.beta=[0.0001,0.001,0.01,0.05,0.2,0.5]"]
    cfg = load_config(d, ov)
    root = str(tmp_path / "exp")
    _worker(0, cfg, root)
    assert "10 network evaluations per batch" in capsys.readouterr().out
    outdir = os.path.join(root, local_path_name(None, cfg["model"], cfg["diffusion"], cfg["dataset"]), "waveforms", "0")
    assert sorted(os.listdir(outdir)) == ["0k_0.wav", "0k_1.wav"]
    ws = []
    for f in ("0k_0.wav", "0k_1.wav"):
        sr, w = wavfile.read(os.path.join(outdir, f))
        assert sr == 16000 and w.dtype == np.float32 and w.shape == (1600,) and np.isfinite(w).all()
        ws.append(w)
    for w in ws:
        assert np.array_equal(w[:801], clip[:801]) and np.array_equal(w[1203:1210], clip[1203:1210])
    assert not np.array_equal(ws[0][801:1203], ws[1][801:1203])         # its own noise per clip

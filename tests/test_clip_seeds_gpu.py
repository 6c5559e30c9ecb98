"""GPU: per-clip seeds (``dws_sampler_set_clip_seeds`` / ``dws_philox_normal_clips``; ``seed=[...]`` on the samplers;
``generate.clip_seeds`` / ``generate.clips``).

The anchor every test leans on, which needs no new reference: clip b of a per-clip run with seeds [k_0 .. k_{B-1}] is
bit-equal to the scalar-seed run at B = 1 with seed = k_b -- the code path the samplers had before.

Cases: wn_tiny and ss_tiny, S = 6 steps; the schedules of tests/test_cfg_sampling_gpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.conftest import REL_TOL, rel_err
from tests.test_cfg_sampling_gpu import KINDS, LABELS, S, _graphs, _sample, _schedule
from tests.test_cfg_sampling_gpu import _net as _class_net

pytestmark = pytest.mark.gpu

SEEDS = [11, 11, 2 ** 63 + 5]


def _plain(name, gpu):
    """(net, L) of an unlabelled tiny model with the weights of every other test"""
    if name == "wn_tiny":
        cfg, _, L, wseed, _, _ = cases.WAVENET_CASES[name]
    else:
        cfg, _, wseed, _, _ = cases.SASHIMI_CASES[name]
        L = cfg["L"]
    return cases.build_ours(cfg, wseed).to(gpu), L


def _u64(vals):
    return (ctypes.c_uint64 * len(vals))(*vals)


def _normal(n, seed, stream, gpu):
    from diffwave_sashimi_amd import _lib
    z = torch.empty(n, device=gpu)
    _lib.check(_lib.load().dws_philox_normal(z.data_ptr(), n, seed, stream, _lib.current_stream()))
    return z


def _normal_clips(B, n, seeds, stream, gpu):
    from diffwave_sashimi_amd import _lib
    z = torch.full((B, n), float("nan"), device=gpu)
    _lib.check(_lib.load().dws_philox_normal_clips(z.data_ptr(), B, n, _u64(seeds), stream, _lib.current_stream()))
    return z


def _check_anchor(run, seeds):
    """``run(B, seed, **kw)``: the batch with the seed list against the B = 1 scalar-seed runs, the reversed list and the
    eager walk.  Returns the batch."""
    B = len(seeds)
    out = run(B, seeds)
    for b, k in enumerate(seeds):
        assert torch.equal(out[b:b + 1], run(1, k, clip=b)), f"clip {b} differs from the B = 1 run with seed {k}"
    assert torch.equal(run(B, seeds[::-1], flip=True), out.flip(0))
    assert torch.equal(run(B, seeds, use_graph=False), out)
    return out


# ------------------------------------------------------------------------------------------------- 1. the RNG itself
@pytest.mark.parametrize("n", [600, 602])
def test_rows_of_the_per_clip_draw_are_the_scalar_streams(gpu, n):
    for stream in (0, 13):
        z = _normal_clips(3, n, SEEDS, stream, gpu)
        for b, k in enumerate(SEEDS):
            assert torch.equal(z[b], _normal(n, k, stream, gpu))
        assert torch.equal(z[0], z[1]) and not torch.equal(z[0], z[2])
    # more clips than one launch carries as arguments (64): the rows keep their seeds across the chunks
    many = list(range(1000, 1070))
    z = _normal_clips(70, n, many, 2, gpu)
    for b in (0, 63, 64, 69):
        assert torch.equal(z[b], _normal(n, many[b], 2, gpu))


def test_neighbouring_keys_give_uncorrelated_streams(gpu):
    """Sample correlation of two independent N(0,1) rows of n values has standard deviation 1/sqrt(n): five of them."""
    n = 16384
    z = _normal_clips(8, n, list(range(100, 108)), 0, gpu).double().cpu()
    r = np.corrcoef(z.numpy())
    worst = float(np.abs(r - np.eye(8)).max())
    print(f"largest |r| among 28 pairs: {worst:.4f} (bound {5 / np.sqrt(n):.4f})")
    assert worst <= 5 / np.sqrt(n)
    assert abs(float(z.mean())) < 5 / np.sqrt(8 * n) and abs(float(z.std()) - 1) < 0.02


# ------------------------------------------------------------------------------------------------------ 2. the anchor
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["wn_tiny", "ss_tiny"])
def test_a_clip_is_the_b1_run_with_its_seed(gpu, name, kind):
    net, L = _plain(name, gpu)
    _, _, dh = _schedule(kind)
    run = lambda B, seed, clip=None, flip=False, **kw: _sample(net, kind, (B, 1, L), dh, seed=seed, **kw)
    out = _check_anchor(run, SEEDS)
    assert torch.equal(out[0], out[1]) and not torch.equal(out[0], out[2])
    assert torch.isfinite(out).all()


# --------------------------------------------------------------------------------------------- 3. straddling groups
def test_clips_whose_length_is_no_multiple_of_four(gpu):
    """L = 601: flat groups of four would straddle the clips; groups are numbered inside the clip and the element-wise
    path runs.  DDIM (eta 0.5), plain and with the replacement of a known region whose spans cross group borders."""
    from diffwave_sashimi_amd import sampling as smp
    net, _ = _plain("wn_tiny", gpu)
    L = 601
    _, _, dh = _schedule("ddim")
    run = lambda B, seed, clip=None, flip=False, **kw: smp.sampling_ddim(net, (B, 1, L), dh, S, eta=0.5, seed=seed, **kw)
    out = _check_anchor(run, SEEDS)
    assert torch.equal(out[0], out[1]) and not torch.equal(out[0], out[2])

    g = torch.Generator().manual_seed(5)
    known = torch.randn(3, 1, L, generator=g) * 0.3
    mask = smp.spans_to_mask((3, 1, L), [(3, 10), (14, 15), (297, 303), (598, 601)])

    def edited(B, seed, clip=None, flip=False, **kw):
        y = known if B == 3 else known[clip:clip + 1]
        return smp.sampling_ddim(net, (B, 1, L), dh, S, eta=0.5, seed=seed, known=y.flip(0) if flip else y, mask=mask, **kw)
    seeds = [11, 12, 2 ** 63 + 5]
    out = _check_anchor(edited, seeds)
    m = mask.expand(3, 1, L)
    assert torch.equal(out.cpu()[m], known[m]) and not torch.equal(out[0], out[1])


# ------------------------------------------------------------------------------------------- 4. every stream kind
STREAM_CASES = [("replace", "ddpm"), ("qsample", "ddpm"), ("program", "ddpm"), ("program", "dpmpp2m")]


@pytest.mark.parametrize("what,kind", STREAM_CASES)
def test_every_drawn_stream_is_per_clip(gpu, what, kind):
    """Known-region noise (stream S + 1 + s), start noise (2S + 1), jump noise (v) -- B = 2 against two B = 1 runs."""
    from diffwave_sashimi_amd import sampling as smp
    net, L = _plain("wn_tiny", gpu)
    _, _, dh = _schedule(kind)
    g = torch.Generator().manual_seed(9)
    known = torch.randn(2, 1, L, generator=g) * 0.3
    start = torch.randn(2, 1, L, generator=g) * 0.3
    mask = smp.spans_to_mask((2, 1, L), [(0, 90), (201, 250)])
    seeds = [21, 2 ** 63 + 9]

    def run(B, seed, clip=None, flip=False, **kw):
        pick = lambda t: (t.flip(0) if flip else t) if B == 2 else t[clip:clip + 1]
        if what == "replace":
            kw.update(known=pick(known), mask=mask)
        elif what == "qsample":
            kw.update(x_start=pick(start), start_step=3)
        else:
            kw.update(known=pick(known), mask=mask, resample=(2, 2))
        return _sample(net, kind, (B, 1, L), dh, seed=seed, **kw)
    out = _check_anchor(run, seeds)
    assert not torch.equal(out[0], out[1]) and torch.isfinite(out).all()
    if what == "qsample":       # one seed for both clips: they differ through their start alone
        same = run(2, [21, 21])
        assert torch.equal(same[0:1], out[0:1]) and not torch.equal(same[0], same[1])


# ------------------------------------------------------------------------------------------------------------ 5. CFG
@pytest.mark.parametrize("kind", KINDS)
def test_guided_clips_are_the_bc1_guided_runs(gpu, kind):
    net, cfg, L = _class_net("wn_tiny", gpu)
    _, _, dh = _schedule(kind)
    seeds = [31, 2 ** 63 + 1]

    def run(B, seed, clip=None, flip=False, **kw):
        labels = (LABELS[::-1] if flip else LABELS) if B == 2 else [LABELS[clip]]
        return _sample(net, kind, (B, 1, L), dh, labels=labels, cfg_scale=1.5, seed=seed, **kw)
    out = _check_anchor(run, seeds)
    assert not torch.equal(out[0], out[1])
    with pytest.raises(ValueError, match="clip seeds for a batch"):      # B is the caller's B, not the doubled batch
        run(2, seeds + seeds)


# ----------------------------------------------------------------------------------------- 6. graphs and the state
def test_seed_tables_replay_and_the_scalar_path_is_untouched(gpu):
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd import sampling as smp
    net, L = _plain("wn_tiny", gpu)
    _, _, dh = _schedule("ddim")
    run = lambda seed, **kw: smp.sampling_ddim(net, (3, 1, L), dh, S, eta=0.5, seed=seed, **kw)
    scalar = run(7)
    a = run(SEEDS)
    base = _graphs(net)
    b, c = run([1, 2, 3]), run([2 ** 64 - 1, 0, 2 ** 32])
    assert _graphs(net) == base                                  # three tables, one per-clip graph
    assert not torch.equal(a, b) and not torch.equal(b, c) and not torch.equal(a, scalar)
    assert torch.equal(run(7), scalar) and _graphs(net) == base  # the scalar form: its bits and its graph
    assert torch.equal(run(SEEDS), a) and torch.equal(run(7), scalar) and torch.equal(run([1, 2, 3]), b)
    assert _graphs(net) == base                                  # alternating captures nothing new
    assert torch.equal(run(7, use_graph=False), scalar)

    # the engine's own refusals, on the raw entry points
    lib, h, st = _lib.load(), net._handle, _lib.current_stream()
    fp = ctypes.POINTER(ctypes.c_float)
    steps, coef, _ = _schedule("ddim")
    steps, coef = np.ascontiguousarray(steps), np.ascontiguousarray(coef)
    x0 = torch.randn(3, 1, L)
    x = x0.to(gpu).clone()
    schedule = lambda: lib.dws_sampler_run_schedule(h, x.data_ptr(), _lib.DWS_SAMPLER_DDIM, S, steps.ctypes.data_as(fp),
                                                    coef.ctypes.data_as(fp), 0, 1, 0, 1, st)
    dhs = smp.calc_diffusion_hyperparams(S, 1e-4, 0.05)
    tabs = [smp._host_table(dhs[k]) for k in ("Alpha", "Alpha_bar", "Sigma")]
    assert lib.dws_sampler_set_clip_seeds(h, _u64([1, 2]), 0, st) == _lib.DWS_ERR_INVALID
    try:
        _lib.check(lib.dws_sampler_set_clip_seeds(h, _u64([1, 2]), 2, st))          # the model is prepared for 3 clips
        with pytest.raises(RuntimeError, match="clip seeds"):
            _lib.check(schedule())
        _lib.check(lib.dws_sampler_set_clip_seeds(h, _u64([1, 2, 3]), 3, st))
        with pytest.raises(NotImplementedError, match="per-clip seeds"):
            _lib.check(lib.dws_sampler_run(h, x.data_ptr(), tabs[0][1], tabs[1][1], tabs[2][1], S, 0, 1, 0, 1, st))
        with pytest.raises(NotImplementedError, match="per-clip seeds"):
            _lib.check(lib.dws_sampler_steps(h, x.data_ptr(), tabs[0][1], tabs[1][1], tabs[2][1], S, S - 1, 1, 1, 1, st))
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), x0)                          # nothing ran
        _lib.check(schedule())                                   # the table holds until it is changed: the seed (1) is ignored
        torch.cuda.synchronize()
        assert torch.equal(x, smp.sampling_ddim(net, (3, 1, L), dh, S, eta=0.5, x_T=x0, seed=[1, 2, 3]))
        _lib.check(lib.dws_sampler_set_clip_seeds(h, _u64([1, 2, 3]), 3, st))
        net._prepare(2, L)                                       # another shape drops the table
        net._prepare(3, L)
        x.copy_(x0)
        _lib.check(schedule())
        torch.cuda.synchronize()
        assert torch.equal(x, smp.sampling_ddim(net, (3, 1, L), dh, S, eta=0.5, x_T=x0, seed=1))
    finally:
        _lib.check(lib.dws_sampler_set_clip_seeds(h, None, 0, st))
    assert torch.equal(run(7), scalar)


# --------------------------------------------------------------------------------------------------------- 7. guided
def test_guided_run_with_a_seed_list(gpu):
    """``sampling_guided`` (declipping, DDPM): the noise a seed list draws is that of ``dws_philox_normal_clips``, bit
    for bit; a clip against its B = 1 run additionally needs the data-only backward to be independent of the batch."""
    from diffwave_sashimi_amd import sampling as smp
    net, L = _plain("wn_tiny", gpu)
    net.eval()
    _, _, dh = _schedule("ddpm")
    g = torch.Generator().manual_seed(41)
    y = smp.declip_operator(0.2)(torch.randn(2, 1, L, generator=g) * 0.3)
    op = smp.declip_operator(0.2)
    seeds = [51, 2 ** 63 + 3]
    run = lambda B, seed, y, **kw: smp.sampling_guided(net, (B, 1, L), dh, measurement=y, operator=op, scale=0.5, seed=seed,
                                                       **kw)
    out = run(2, seeds, y)
    x_T = _normal_clips(2, L, seeds, S, gpu).reshape(2, 1, L)
    noise = torch.stack([_normal_clips(2, L, seeds, s, gpu).reshape(2, 1, L) for s in range(S)])
    assert torch.equal(out, run(2, None, y, x_T=x_T, noise=noise))
    for b, k in enumerate(seeds):
        one = run(1, k, y[b:b + 1])
        err = rel_err(out[b:b + 1], one)
        print(f"guided clip {b} against its B = 1 run: rel err {err:.3e}, bitwise {torch.equal(out[b:b + 1], one)}")
        assert torch.equal(out[b:b + 1], one)


# ------------------------------------------------------------------------------------------------------------ 8. CLI
def test_generate_writes_the_same_clip_at_any_batch_size(tmp_path, gpu):
    from scipy.io import wavfile
    from diffwave_sashimi_amd.generate import generate
    cfg = cases.WAVENET_CASES["wn_tiny"][0]
    diff = dict(T=S, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="sc09", segment_length=300, sampling_rate=16000)

    def gen(tag, **kw):
        torch.manual_seed(3)            # ckpt_iter="init": the same random weights for every call
        written = []
        audio = generate(0, diff, dict(cfg), ds, ckpt_iter="init", n_samples=4, seed=5, clip_seeds=True,
                         exp_root=str(tmp_path / tag), written=written, **kw)
        return audio, written
    full, files = gen("b4", batch_size=4)
    assert [os.path.basename(f) for f in files] == [f"0k_{k}.wav" for k in range(4)]
    assert full.shape == (4, 1, 300) and torch.isfinite(full).all()
    assert len({full[k].cpu().numpy().tobytes() for k in range(4)}) == 4
    for bs in (2, 1):
        other, _ = gen(f"b{bs}", batch_size=bs)
        assert torch.equal(other, full)
    one, files = gen("clip2", batch_size=4, clips=[2])
    assert [os.path.basename(f) for f in files] == ["0k_2.wav"]
    assert os.listdir(os.path.dirname(files[0])) == ["0k_2.wav"]
    assert torch.equal(one, full[2:3])
    sr, w = wavfile.read(files[0])
    assert np.array_equal(w, full[2, 0].cpu().numpy())
    # rank 1 of a two-rank run at n_samples = 2 makes global clips 2 and 3
    torch.manual_seed(3)
    r1 = generate(1, diff, dict(cfg), ds, ckpt_iter="init", n_samples=2, seed=5, clip_seeds=True, num_ranks=2,
                  exp_root=str(tmp_path / "r1"))
    assert torch.equal(r1, full[2:4])

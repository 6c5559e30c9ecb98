"""GPU: the fused optimizer step (``dws_optim_step``, ``csrc/optim_kernels.hip``) and ``EngineAdam`` on top of it.

Reference: float64 Adam / EMA / clipping written out in numpy (tests/adam_reference.py).  Bound, for each of p, m, v, ema:
    max |got - f64| <= 2 x max |fp32 torch.optim.Adam(foreach=False) (+ lerp_, + clip_grad_norm_) on the CPU - f64| + 1 ulp32(max |f64|)
on the same inputs -- the factor 2 is the convention of the split-arithmetic tests, the ulp floor covers quantities the
baseline happens to hit exactly."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import cases
from tests.adam_reference import BETA1, BETA2, EPS, AdamPair, recipe
from tests.conftest import ROOT
from tests.test_generate_cli import _tree

pytestmark = pytest.mark.gpu

KINDS = ("p", "g", "m", "v", "ema", "mir")
SENTINEL = 0x7FC0BEEF      # a NaN payload no kernel produces
GAP = 4


def _chunk():
    from diffwave_sashimi_amd import _lib
    return int(_lib.load().dws_optim_chunk())


class Arena:
    """Every tensor of a model-free step -- parameter, gradient, both moments, shadow, mirror -- carved out of ONE flat
    buffer with sentinel words around each; ``misaligned[i]`` puts all six tensors of entry i one float past a 16-byte
    boundary (what a slice of a flat buffer or a data-parallel arena view looks like)."""

    def __init__(self, sizes, misaligned, dev):
        self.sizes, self.dev = list(sizes), dev
        self.off, off = {}, 0
        for i, n in enumerate(self.sizes):
            for k in KINDS:
                off = (off + GAP + 3) // 4 * 4 + (1 if misaligned[i] else 0)
                self.off[k, i] = off
                off += n
        self.total = off + GAP
        self.words = torch.full((self.total,), SENTINEL, dtype=torch.int32, device=dev)
        self.flat = self.words.view(torch.float32)
        assert self.flat.data_ptr() % 16 == 0
        self.is_tensor = torch.zeros(self.total, dtype=torch.bool)
        for (k, i), o in self.off.items():
            self.is_tensor[o:o + self.sizes[i]] = True
            assert (self.view(k, i).data_ptr() % 16 == 4) == bool(misaligned[i]) and self.view(k, i).data_ptr() % 4 == 0

    def view(self, k, i):
        o = self.off[k, i]
        return self.flat[o:o + self.sizes[i]]

    def fill(self, k, arrays):
        for i, a in enumerate(arrays):
            self.view(k, i).copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))

    def zero(self, k):
        for i in range(len(self.sizes)):
            self.view(k, i).zero_()

    def get(self, k):
        return [self.view(k, i).cpu().numpy() for i in range(len(self.sizes))]

    def bits(self, k):
        return [self.view(k, i).view(torch.int32).cpu().clone() for i in range(len(self.sizes))]

    def ptrs(self, k):
        return (ctypes.c_void_p * len(self.sizes))(*[self.view(k, i).data_ptr() for i in range(len(self.sizes))])

    def sentinels_intact(self):
        w = self.words.cpu()
        return bool((w[~self.is_tensor] == SENTINEL).all())


class RawStepper:
    """``dws_optim_step`` without a model, on an Arena."""

    def __init__(self, arena, lrs, ema_decay=None, max_norm=None, mirror=False, weight_decay=0.0):
        from diffwave_sashimi_amd import _lib
        self.lib, self._lib, self.a = _lib.load(), _lib, arena
        n = self.n = len(arena.sizes)
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.dws_optim_create(ctypes.byref(self.h)))
        self.P, self.G, self.M, self.V = (arena.ptrs(k) for k in ("p", "g", "m", "v"))
        self.E = arena.ptrs("ema") if ema_decay is not None else None
        self.R = arena.ptrs("mir") if mirror else None
        self.N = (ctypes.c_int64 * n)(*arena.sizes)
        self.LR = (ctypes.c_double * n)(*lrs)
        self.WD = (ctypes.c_double * n)(*([weight_decay] * n))
        self.d, self.max_norm, self.t = ema_decay, max_norm, 0
        self.norm = torch.full((1,), -1.0, device=arena.dev) if max_norm is not None else None

    def step(self):
        self.t += 1
        T = (ctypes.c_int64 * self.n)(*([self.t] * self.n))
        self._lib.check(self.lib.dws_optim_step(
            self.h, self.n, self.P, self.G, self.M, self.V, self.E, self.R, self.N, self.LR, T, self.WD, BETA1, BETA2, EPS,
            self.d or 0.0, self.max_norm or 0.0, None if self.norm is None else self.norm.data_ptr(), None, None,
            self._lib.current_stream()))

    def close(self):
        torch.cuda.synchronize()
        self.lib.dws_optim_destroy(self.h)


_RECIPE = {}


def _recipe():
    """The fixed recipe, computed once: sizes, initial parameters, 20 gradient lists; lr 2e-4, every other tensor in a
    second group at 1e-2; the tensors at indices 0, 3, 4, 7, 8 off 16-byte alignment (both kinds at every size class)."""
    if not _RECIPE:
        C = _chunk()
        sizes, params, grads = recipe(C)
        _RECIPE.update(C=C, sizes=sizes, params=params, grads=grads, lrs=[2e-4 if i % 2 == 0 else 1e-2 for i in range(len(sizes))],
                       misaligned=[i in (0, 3, 4, 7, 8) for i in range(len(sizes))])
    return _RECIPE


def _run_raw(gpu, ema_decay, max_norm, mirror=False, steps=None, collect_norms=False):
    r = _recipe()
    a = Arena(r["sizes"], r["misaligned"], gpu)
    a.fill("p", r["params"])
    a.zero("m")
    a.zero("v")
    if ema_decay is not None:
        a.fill("ema", r["params"])
    st = RawStepper(a, r["lrs"], ema_decay, max_norm, mirror)
    norms = []
    for gs in r["grads"][:steps]:
        a.fill("g", gs)
        st.step()
        if collect_norms:
            norms.append(st.norm.cpu().clone())
    st.close()
    return a, norms


_PAIRS = {}


def _pair(ema_decay, max_norm):
    """Float64 reference + CPU fp32 baseline of the recipe for one setting, computed once and left unchanged."""
    key = (ema_decay, max_norm)
    if key not in _PAIRS:
        r = _recipe()
        pair = AdamPair(r["params"], r["lrs"], ema_decay, max_norm)
        for gs in r["grads"]:
            pair.step(gs)
        _PAIRS[key] = pair
    return _PAIRS[key]


@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("ema_decay", [None, 0.999], ids=["noema", "ema"])
def test_model_free_step_against_float64(gpu, ema_decay, max_norm):
    """20 steps of the recipe, two learning rates, half the tensors one float off 16-byte alignment; p, m, v (and ema)
    against float64.  With max_norm = 1 the norm (0.17 .. 1750 over the five gradient scales) lies below the threshold in
    every fifth step and above it otherwise: the float64 reference is Adam fed with the scaled gradients."""
    a, _ = _run_raw(gpu, ema_decay, max_norm)
    pair = _pair(ema_decay, max_norm)
    if max_norm is not None:
        assert min(pair.norms) < max_norm < max(pair.norms)
    for name, kind in (("p", "p"), ("m", "m"), ("v", "v")) + ((("ema", "ema"),) if ema_decay is not None else ()):
        pair.check(name, a.get(kind), what=f"ema={ema_decay} clip={max_norm}: ")
    assert a.sentinels_intact()


@pytest.mark.parametrize("ema_decay,mirror", [(None, False), (0.9, False), (None, True), (0.9, True)],
                         ids=["plain", "ema", "mirror", "ema+mirror"])
def test_nothing_else_is_written(gpu, ema_decay, mirror):
    """Sentinel words between all tensors stay bit for bit; the gradients are never written; without a shadow / a mirror
    table those regions are untouched too; a given mirror ends up as the parameter, bit for bit."""
    r = _recipe()
    a, _ = _run_raw(gpu, ema_decay, 1.0, mirror=mirror, steps=3)
    assert a.sentinels_intact()
    want_g = [torch.from_numpy(np.ascontiguousarray(g)).view(torch.int32) for g in r["grads"][2]]
    assert all(torch.equal(x, y) for x, y in zip(a.bits("g"), want_g))
    for k, used in (("ema", ema_decay is not None), ("mir", mirror)):
        untouched = all(bool((b == SENTINEL).all()) for b in a.bits(k))
        assert untouched == (not used), k
    if mirror:
        assert all(torch.equal(x, y) for x, y in zip(a.bits("mir"), a.bits("p")))
    moved = [not np.array_equal(x, y) for x, y in zip(a.get("p"), r["params"])]
    assert all(moved)


def test_zero_parameter_with_zero_gradient_stays_zero(gpu):
    """The ZeroConv case: p = 0, g = 0 for every step -> p, m, v, the shadow and the mirror are exactly 0.0."""
    C = _chunk()
    sizes = [5, C + 3]
    a = Arena(sizes, [True, False], gpu)
    for k in ("p", "g", "m", "v", "ema"):
        a.zero(k)
    st = RawStepper(a, [2e-4, 2e-4], ema_decay=0.999, max_norm=1.0, mirror=True)
    for _ in range(3):
        st.step()
    st.close()
    assert float(st.norm.cpu()) == 0.0
    for k in ("p", "m", "v", "ema", "mir"):
        assert all(bool((b == 0).all()) for b in a.bits(k)), k          # +0.0 bit pattern everywhere
    assert a.sentinels_intact()


def test_clipping_norm_reproducibility_and_threshold(gpu):
    r = _recipe()
    pair = _pair(None, 1.0)
    a1, n1 = _run_raw(gpu, None, 1.0, collect_norms=True)
    a2, n2 = _run_raw(gpu, None, 1.0, collect_norms=True)
    # bitwise reproducible from run to run: the norm of every step and every tensor the step writes
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(n1, n2))
    for k in ("p", "m", "v"):
        assert all(torch.equal(x, y) for x, y in zip(a1.bits(k), a2.bits(k))), k
    # the norm against float64: at most twice the relative error of CPU torch.linalg.vector_norm on the concatenated fp32
    # gradients, floor 2^-22
    for k, (got, gs) in enumerate(zip(n1, r["grads"])):
        ref = pair.norms[k]
        cpu = float(torch.linalg.vector_norm(torch.from_numpy(np.concatenate(gs))))
        bound = max(2.0 * abs(cpu - ref) / ref, 2.0 ** -22)
        err = abs(float(got) - ref) / ref
        print(f"step {k}: norm {float(got):.6e}, rel err {err:.2e}, torch cpu {abs(cpu - ref) / ref:.2e}")
        assert err <= bound, (k, float(got), ref, err, bound)
    # p.grad is not rewritten (the scale is applied on the fly)
    want_g = [torch.from_numpy(np.ascontiguousarray(g)).view(torch.int32) for g in r["grads"][-1]]
    assert all(torch.equal(x, y) for x, y in zip(a1.bits("g"), want_g))
    # a threshold above every norm: bitwise the unclipped run
    big, _ = _run_raw(gpu, None, 1e9)
    plain, _ = _run_raw(gpu, None, None)
    assert max(pair.norms) < 1e9
    for k in ("p", "m", "v"):
        assert all(torch.equal(x, y) for x, y in zip(big.bits(k), plain.bits(k))), k
    assert not all(torch.equal(x, y) for x, y in zip(a1.bits("p"), plain.bits("p")))      # ... and clipping does change it


def test_more_chunks_than_workgroups(gpu):
    """One tensor of 2048 chunks + 5 elements (one float off alignment) and a small one: every workgroup of the capped
    grid loops (the first ones over two chunks), in the norm launch and in the step."""
    C = _chunk()
    sizes = [2048 * C + 5, 7]
    g = torch.Generator().manual_seed(11)
    params = [(0.1 * torch.randn(n, generator=g)).numpy() for n in sizes]
    a = Arena(sizes, [True, False], gpu)
    a.fill("p", params)
    a.fill("ema", params)
    a.zero("m")
    a.zero("v")
    pair = AdamPair(params, [2e-4, 1e-2], ema_decay=0.99, max_norm=1.0)
    st = RawStepper(a, [2e-4, 1e-2], ema_decay=0.99, max_norm=1.0)
    for k in range(2):
        gs = [(torch.randn(n, generator=g) * 10.0 ** (-3 * k)).numpy() for n in sizes]        # norm 2900, then 2.9
        a.fill("g", gs)
        st.step()
        pair.step(gs)
        assert abs(float(st.norm.cpu()) - pair.norms[-1]) <= 2.0 ** -22 * pair.norms[-1]
    st.close()
    for name in ("p", "m", "v", "ema"):
        pair.check(name, a.get(name), what="2048 chunks + 5: ")
    assert a.sentinels_intact()


def test_abi_errors_with_a_model(gpu):
    """Unknown names, wrong element counts and non-float32 parameters come back as DWS_ERR_INVALID with a message."""
    from diffwave_sashimi_amd import _lib
    lib = _lib.load()
    net = cases.build_ours(cases.ss_cfg(d_model=32, n_layers=1, L=512, diffusion_step_embed_dim_mid=64), 3).to(gpu).eval()
    with torch.no_grad():
        net((torch.zeros(1, 1, 512, device=gpu), torch.zeros(1, 1, device=gpu)))
    name = next(n for n, p in net.named_parameters() if p.numel() > 8)
    int_name = next(k for k, v in net.state_dict().items() if v.dtype == torch.int64)
    n = dict(net.named_parameters())[name].numel()
    t = [torch.zeros(n, device=gpu) for _ in range(4)]
    h = ctypes.c_void_p()
    _lib.check(lib.dws_optim_create(ctypes.byref(h)))

    def call(nm, numel):
        one = lambda x: (ctypes.c_void_p * 1)(x.data_ptr())
        return lib.dws_optim_step(h, 1, one(t[0]), one(t[1]), one(t[2]), one(t[3]), None, None, (ctypes.c_int64 * 1)(numel),
                                  (ctypes.c_double * 1)(1e-3), (ctypes.c_int64 * 1)(1), None, 0.9, 0.999, 1e-8, 0.0, 0.0, None,
                                  net._handle, (ctypes.c_char_p * 1)(nm.encode()), _lib.current_stream())
    for nm, numel, msg in (("no.such.weight", n, "unknown parameter"), (name, n - 1, "elements"), (int_name, n, "float32")):
        assert call(nm, numel) == _lib.DWS_ERR_INVALID
        assert msg in lib.dws_last_error().decode()
    assert call(name, n) == _lib.DWS_OK
    torch.cuda.synchronize()
    lib.dws_optim_destroy(h)


# ------------------------------------------------------------------------------------------------ EngineAdam on the engine
def _small_models():
    return {
        "wavenet": (cases.wn_cfg(res_channels=64, skip_channels=64, num_res_layers=8, dilation_cycle=8), 2e-3),
        "sashimi": (cases.ss_cfg(d_model=32, n_layers=2, L=1024, diffusion_step_embed_dim_mid=128), 1e-3),
    }


@pytest.mark.parametrize("name", ["wavenet", "sashimi"])
def test_engine_coherence_is_bitwise(gpu, name):
    """3 forward / backward / EngineAdam(module=net) rounds on the small models of tests/test_learning_gpu.py (B = 2,
    L = 1024): every round's parameters against float64 Adam on that round's gradients; then an eval forward, invalidate()
    (everything is sent again from the torch tensors) and the same forward: equal bit for bit -- the mirror the step wrote
    IS the torch tensors, and _sync_params was right to send nothing (counted: no dws_model_update_params after a step)."""
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.models import construct_model
    from diffwave_sashimi_amd.optim import EngineAdam
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    cfg, lr = _small_models()[name]
    B, L = 2, 1024
    torch.manual_seed(0)
    net = construct_model(dict(cfg)).to(gpu).train()
    params = list(net.parameters())
    opt = EngineAdam(params, lr=lr, ema_decay=0.9, max_grad_norm=1.0, module=net)
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    g = torch.Generator().manual_seed(1)
    lib = _lib.load()
    calls = []
    real = lib.dws_model_update_params
    pair = None
    try:
        lib.dws_model_update_params = lambda *a: (calls.append(int(a[1])), real(*a))[1]
        for rnd in range(3):
            audio = (0.3 * torch.randn(B, 1, L, generator=g)).to(gpu)
            opt.zero_grad()
            before = len(calls)
            loss = training_loss(net, nn.MSELoss(), audio, dh, generator=g)
            if rnd > 0:
                assert len(calls) == before, "the forward after an EngineAdam step re-sent parameters"
            loss.backward()
            if pair is None:      # (SaShiMi rewrites its C parameters at the first forward: the start is what they are now)
                pair = AdamPair([p.detach().cpu().numpy().ravel() for p in params], [lr] * len(params), 0.9, 1.0)
            grads = [p.grad.detach().clone() for p in params]
            versions = [p._version for p in params]
            opt.step()
            assert all(p._version > v for p, v in zip(params, versions))              # other observers see the write
            assert all(torch.equal(p.grad, g0) for p, g0 in zip(params, grads))       # p.grad is not rewritten
            pair.step([g0.cpu().numpy().ravel() for g0 in grads])
            pair.check("p", [p.detach().cpu().numpy().ravel() for p in params], what=f"{name} round {rnd}: ")
            assert abs(float(opt.grad_norm) - pair.norms[-1]) <= 2.0 ** -22 * pair.norms[-1]
            sd = opt.state_dict()         # (taking a checkpoint between steps must not detach the step counters)
            assert {float(st["step"]) for st in sd["state"].values()} == {rnd + 1.0}
            assert {float(opt.state[p]["step"]) for p in params} == {rnd + 1.0}
        pair.check("m", [opt.state[p]["exp_avg"].cpu().numpy().ravel() for p in params], what=f"{name}: ")
        pair.check("v", [opt.state[p]["exp_avg_sq"].cpu().numpy().ravel() for p in params], what=f"{name}: ")
        ema = opt.ema_state_dict()
        pair.check("ema", [ema[k].cpu().numpy().ravel() for k, _ in net.named_parameters()], what=f"{name}: ")
        net.eval()
        x = (0.3 * torch.randn(B, 1, L, generator=g)).to(gpu)
        steps = torch.tensor([[3.0], [41.0]], device=gpu)
        before = len(calls)
        with torch.no_grad():
            out_mirror = net((x, steps)).clone()
        assert len(calls) == before
        net.invalidate()
        with torch.no_grad():
            out_resent = net((x, steps)).clone()
        assert len(calls) == before + 1 and calls[-1] >= len(params)                  # invalidate() did re-send everything
    finally:
        lib.dws_model_update_params = real
    assert bool(torch.isfinite(out_mirror).all()) and float(out_mirror.abs().max()) > 0
    assert torch.equal(out_mirror, out_resent)


DP_WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["DWS_ROOT"])
import numpy as np, torch, torch.nn as nn, torch.distributed as dist
from tests import cases
from tests.adam_reference import AdamPair
from diffwave_sashimi_amd.distributed_util import apply_gradient_allreduce, init_distributed
from diffwave_sashimi_amd.optim import EngineAdam
from diffwave_sashimi_amd.training import training_loss
from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams

init_distributed(0, 1, "g", "nccl", "tcp://127.0.0.1:" + os.environ["MASTER_PORT"])
cfg, L = cases.ss_cfg(d_model=32, n_layers=1, L=512, diffusion_step_embed_dim_mid=64), 512
net = cases.build_ours(cfg, 300).cuda().train()
net = apply_gradient_allreduce(net, bucket_bytes=64 * 1024)
params = list(net.parameters())
opt = EngineAdam(params, lr=1e-3, ema_decay=0.9, max_grad_norm=1.0, module=net)
dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
data = torch.randn(2, 2, 1, L, generator=torch.Generator().manual_seed(7)) * 0.3
pair, rows, views, unaligned = None, [], 0, 0
for step in range(2):
    opt.zero_grad()
    loss = training_loss(net, nn.MSELoss(), data[step].cuda(), dh, generator=torch.Generator().manual_seed(1000 + step))
    loss.backward()
    if pair is None:
        pair = AdamPair([p.detach().cpu().numpy().ravel() for p in params], [1e-3] * len(params), 0.9, 1.0)
    arena = [(b.flat.data_ptr(), b.flat.data_ptr() + b.flat.numel() * 4) for b in net._dws_grad_reducer.buckets]
    views = sum(any(lo <= p.grad.data_ptr() < hi for lo, hi in arena) for p in params)
    unaligned = sum(p.grad.data_ptr() % 16 != 0 for p in params)
    grads = [p.grad.detach().clone() for p in params]
    opt.step()
    pair.step([g.cpu().numpy().ravel() for g in grads])
    row = {"same_grads": all(torch.equal(p.grad, g) for p, g in zip(params, grads))}
    for name, got in (("p", [p.detach() for p in params]), ("m", [opt.state[p]["exp_avg"] for p in params]),
                      ("v", [opt.state[p]["exp_avg_sq"] for p in params]),
                      ("ema", [opt.ema_state_dict()[k] for k, _ in net.named_parameters()])):
        row[name] = pair.errors(name, [t.cpu().numpy().ravel() for t in got])
    row["norm"] = [float(opt.grad_norm), pair.norms[-1]]
    rows.append(row)
torch.cuda.synchronize()
print(json.dumps({"rows": rows, "views": views, "unaligned": unaligned, "params": len(params)}))
dist.destroy_process_group()
'''


def test_dp_arena_views(gpu):
    """The 1-rank RCCL set-up of tests/test_rccl_gpu.py with apply_gradient_allreduce: p.grad are views of the flat
    all-reduce buckets (4-byte aligned).  Two EngineAdam steps, each against float64 on the cloned reduced gradients."""
    from tests.test_rccl_gpu import _free_port, _last_json
    env = dict(os.environ, DWS_ROOT=ROOT, MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", DP_WORKER], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    d = _last_json(r.stdout)
    assert d["views"] == d["params"] > 10, d                       # every gradient is an arena view
    print("arena views off 16-byte alignment:", d["unaligned"], "of", d["params"])
    for k, row in enumerate(d["rows"]):
        assert row["same_grads"]
        for name in ("p", "m", "v", "ema"):
            err, base, ulp = row[name]
            print(f"dp step {k} {name}: max abs error {err:.3e}, fp32 torch baseline {base:.3e}, ulp {ulp:.3e}")
            assert err <= 2.0 * base + ulp, (k, name, row[name])
        got, ref = row["norm"]
        assert abs(got - ref) <= 2.0 ** -22 * ref


# ------------------------------------------------------------------------------------------------ the drivers
def test_cli_train_generate_with_ema_and_clipping(tmp_path, gpu, capsys):
    """train.py with +train.optimizer=engine +train.ema_decay=0.9 +train.clip_grad_norm=1.0 on synthetic clips, 4
    iterations: the checkpoint's EMA, the optimizer state in torch.optim.Adam, a resume under train.optimizer=torch,
    generate.ema on both kinds of checkpoint."""
    from diffwave_sashimi_amd.generate import generate, load_config, local_path_name
    from diffwave_sashimi_amd.train import distributed_train

    def train_main(overrides, exp_root):      # train.py's main() behind its device count: one rank on this GPU
        distributed_train(0, 1, "g", load_config(d, overrides), exp_root)
    d = _tree(tmp_path / "configs")
    model = ["model=wavenet", "model.res_channels=64", "model.skip_channels=64", "model.num_res_layers=4",
             "model.dilation_cycle=4", "+model.in_channels=1", "+model.out_channels=1",
             "+model.diffusion_step_embed_dim_in=128", "+model.diffusion_step_embed_dim_mid=512",
             "+model.diffusion_step_embed_dim_out=512", "dataset._name_=synthetic", "dataset.segment_length=1024",
             "+dataset.n_items=8", "diffusion.T=8"]
    tr = ["+train.ckpt_iter=-1", "+train.n_iters=4", "+train.iters_per_ckpt=4", "+train.iters_per_logging=1",
          "+train.learning_rate=2e-3", "+train.batch_size_per_gpu=4", "+train.num_workers=0"]
    engine = ["+train.optimizer=engine", "+train.ema_decay=0.9", "+train.clip_grad_norm=1.0"]
    cfg = load_config(d, model)
    diffusion = {k: v for k, v in cfg["diffusion"].items() if k != "beta"}
    run = local_path_name(None, cfg["model"], cfg["diffusion"], cfg["dataset"])

    exp = str(tmp_path / "exp_engine")
    torch.manual_seed(0)
    train_main(model + tr + engine + ["generate.n_samples=2"], exp)
    assert "sampling from the EMA weights of iteration 4" in capsys.readouterr().out       # the in-loop generate call
    assert sorted(os.listdir(os.path.join(exp, run, "waveforms", "4"))) == ["0k_0.wav", "0k_1.wav"]
    ck = torch.load(os.path.join(exp, run, "checkpoint", "4.pkl"), map_location="cpu")
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "ema_state_dict"}
    msd, esd = ck["model_state_dict"], ck["ema_state_dict"]
    assert list(esd) == list(msd) and all(esd[k].shape == msd[k].shape and esd[k].dtype == msd[k].dtype for k in msd)
    assert all(bool(torch.isfinite(v).all()) for v in esd.values())
    assert sum(not torch.equal(esd[k], msd[k]) for k in msd) > len(msd) // 2
    log = [json.loads(l) for l in open(os.path.join(exp, run, "train_log.jsonl"))]
    norms = [r_["train/grad_norm"] for r_ in log if "train/loss" in r_]
    assert len(norms) == 5 and all(np.isfinite(norms)) and all(n_ > 0 for n_ in norms)
    # the optimizer state loads into torch.optim.Adam
    from diffwave_sashimi_amd.models import construct_model
    probe = construct_model(dict(cfg["model"]))
    stock = torch.optim.Adam(probe.parameters(), lr=1.0)
    stock.load_state_dict(ck["optimizer_state_dict"])
    first = next(iter(probe.parameters()))
    assert float(stock.state[first]["step"]) == 5.0 and stock.param_groups[0]["lr"] == 2e-3
    # a resume under the stock optimizer runs (and, without the EMA keys, writes no ema_state_dict)
    none = ["generate.n_samples=0"]
    train_main(model + none + ["+train.ckpt_iter=max", "+train.n_iters=5", "+train.iters_per_ckpt=5"] + tr[3:] +
               ["+train.optimizer=torch"], exp)
    resumed = torch.load(os.path.join(exp, run, "checkpoint", "5.pkl"), map_location="cpu")
    assert set(resumed) == {"model_state_dict", "optimizer_state_dict"}
    assert float(resumed["optimizer_state_dict"]["state"][0]["step"]) == 6.0
    # ... and back under the engine optimizer: the EMA starts from the loaded weights
    capsys.readouterr()
    train_main(model + none + ["+train.ckpt_iter=max", "+train.n_iters=6", "+train.iters_per_ckpt=6"] + tr[3:] + engine, exp)
    assert "holds no ema_state_dict: the EMA starts from the loaded weights" in capsys.readouterr().out
    again = torch.load(os.path.join(exp, run, "checkpoint", "6.pkl"), map_location="cpu")
    assert "ema_state_dict" in again and float(again["optimizer_state_dict"]["state"][0]["step"]) == 7.0
    w = next(k for k in msd if msd[k].dtype == torch.float32 and msd[k].numel() > 64)
    d_ema = float((again["ema_state_dict"][w] - resumed["model_state_dict"][w]).abs().max())
    d_raw = float((again["model_state_dict"][w] - resumed["model_state_dict"][w]).abs().max())
    assert 0 < d_ema < d_raw            # one step at decay 0.9 from the loaded weights: a tenth of the way
    gen = dict(diffusion_cfg=diffusion, model_cfg=cfg["model"], dataset_cfg=cfg["dataset"], n_samples=2, seed=5)
    with_ema = generate(0, ckpt_iter=4, exp_root=exp, ema=True, **gen).cpu()
    default = generate(0, ckpt_iter=4, exp_root=exp, **gen).cpu()
    raw = generate(0, ckpt_iter=4, exp_root=exp, ema=False, **gen).cpu()
    assert torch.equal(with_ema, default) and not torch.equal(with_ema, raw)
    assert bool(torch.isfinite(with_ema).all()) and bool(torch.isfinite(raw).all())
    with pytest.raises(ValueError, match="no ema_state_dict"):
        generate(0, ckpt_iter=5, exp_root=exp, ema=True, **gen)
    # a checkpoint written by a plain run: the same wav as ever, with and without generate.ema=false
    plain = generate(0, ckpt_iter=5, exp_root=exp, **gen).cpu()
    plain_false = generate(0, ckpt_iter=5, exp_root=exp, ema=False, **gen).cpu()
    net = construct_model(dict(cfg["model"])).to(gpu).eval()
    net.load_state_dict(resumed["model_state_dict"])
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling
    dh = calc_diffusion_hyperparams(**diffusion, fast=True)
    direct = torch.cat([sampling(net, (2, 1, 1024), dh, seed=5)], dim=0).cpu()
    assert torch.equal(plain, plain_false) and torch.equal(plain, direct)

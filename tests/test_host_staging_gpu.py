"""GPU: the pinned staging ring behind every per-call upload (csrc/host_util.h: StagingRing) -- labels, clip seeds,
parameter copies, the optimizer's job table -- driven past its slot count with no host synchronisation in between.

Every case makes 9 calls back to back (2 x 4 slots + 1), each with another payload, behind a stack of matrix products
that keeps the GPU busy, so the host runs ahead: the ring grows to its cap, then waits for its oldest slot, then reuses
slots.  Every intermediate result is compared bitwise with the same sequence run one call at a time with a
synchronisation after each.  A slot reused too early, or a slot believed larger than it is, shows up as another payload
in one of the nine results.

Fixtures: wn_tiny (tests/test_clip_seeds_gpu.py) and the tiny class-conditional model (tests/test_cfg_sampling_gpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import label_reference as lr
from tests.test_cfg_sampling_gpu import T_TRAIN
from tests.test_cfg_sampling_gpu import _net as _class_net
from tests.test_clip_seeds_gpu import _plain, _u64

pytestmark = pytest.mark.gpu

CALLS = 9


class _Busy:
    """Some tens of milliseconds of GPU work on the current stream: what is enqueued behind it waits, the host does not.
    ``still()``: that work has not finished yet, i.e. everything enqueued since is still in flight."""

    def __init__(self, gpu):
        a = torch.ones(4096, 4096, device=gpu)
        for _ in range(40):
            a = (a @ a).clamp_(0.0, 1.0)
        self.keep = a
        self.done = torch.cuda.Event()
        self.done.record()

    def still(self):
        return not self.done.query()


def _both_ways(gpu, call, results):
    """``call(i)`` enqueues call i; ``results(i)`` returns device tensors of its result (no synchronisation).  Runs the
    sequence one call at a time, then back to back behind ``_Busy``; returns (sequential, back to back) as host tensors."""
    seq = []
    for i in range(CALLS):
        call(i)
        torch.cuda.synchronize()
        seq.append([t.cpu() for t in results(i)])
    busy, ahead = _Busy(gpu), False
    held = []
    for i in range(CALLS):
        call(i)
        held.append(results(i))
        if i == 3:
            ahead = busy.still()
    torch.cuda.synchronize()
    assert ahead, "the host did not run ahead of the GPU: the first four calls were not in flight together"
    return seq, [[t.cpu() for t in r] for r in held]


def _assert_same(seq, b2b, what):
    for i, (a, b) in enumerate(zip(seq, b2b)):
        for k, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), f"{what}: result {k} of call {i} differs between the two runs"


def test_labels_back_to_back(gpu):
    from diffwave_sashimi_amd import _lib
    lib = _lib.load()
    net, cfg, L = _class_net("wn_tiny", gpu, unit_output=False)
    B = 3
    g = torch.Generator().manual_seed(3)
    audio = torch.randn(B, 1, L, generator=g).to(gpu)
    steps = torch.tensor(lr.STEPS, dtype=torch.float32).reshape(B).to(gpu)
    with torch.no_grad():
        net((audio, steps.reshape(B, 1)))            # parameters, shape and commit: nothing of that is left to the calls
    assign = [[0, 1, 2], [1, 2, 3], [2, 3, 0], [3, 0, 1], [0, 0, 3], [3, 3, 2], [2, 1, 2], [1, 1, 1], [2, 0, 0]]
    assert len({tuple(a) for a in assign}) == CALLS
    outs = [torch.empty(B, 1, L, device=gpu) for _ in range(2 * CALLS)]
    h, used = net._handle, [0]

    def call(i):
        st = _lib.current_stream()
        _lib.check(lib.dws_model_set_labels(h, (ctypes.c_int32 * B)(*assign[i]), B, st))
        out = outs[used[0]]
        used[0] += 1
        _lib.check(lib.dws_model_forward(h, audio.data_ptr(), steps.data_ptr(), out.data_ptr(), st))
        call.out = out

    seq, b2b = _both_ways(gpu, call, lambda i: [call.out])
    net._label_key = None          # (the shim's cache no longer describes what the engine holds)
    _assert_same(seq, b2b, "labels")
    assert len({r[0].numpy().tobytes() for r in seq}) == CALLS            # the payloads did reach the network
    with torch.no_grad():
        assert torch.equal(seq[4][0], net((audio, steps.reshape(B, 1)), labels=assign[4]).cpu())


def test_clip_seeds_back_to_back(gpu):
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd import sampling as smp
    lib = _lib.load()
    net, L = _plain("wn_tiny", gpu)
    S = 2
    dh = smp.calc_diffusion_hyperparams(T_TRAIN, 1e-4, 0.05)
    tau = smp.ddim_steps(T_TRAIN, S)
    steps = np.ascontiguousarray(np.asarray(tau, np.float32))
    coef = np.ascontiguousarray(smp.ddim_coefficients(dh["Alpha_bar"], tau, 0.5))
    fp = ctypes.POINTER(ctypes.c_float)
    h = net._handle if net._handle is not None else net._ensure_handle()
    net._sync_params(L)

    def run(x):
        _lib.check(lib.dws_sampler_run_schedule(h, x.data_ptr(), _lib.DWS_SAMPLER_DDIM, S, steps.ctypes.data_as(fp),
                                                coef.ctypes.data_as(fp), 0, 0, 0, 1, _lib.current_stream()))

    try:
        # the first shape sizes the first slot (2 seeds, doubled: room for 4); the second shape needs more
        net._prepare(2, L)
        x2 = torch.randn(2, 1, L, generator=torch.Generator().manual_seed(1)).to(gpu)
        _lib.check(lib.dws_sampler_set_clip_seeds(h, _u64([5, 6]), 2, _lib.current_stream()))
        run(x2)
        B = 5
        net._prepare(B, L)
        x_T = torch.randn(B, 1, L, generator=torch.Generator().manual_seed(2)).to(gpu)
        tables = [[1000 * i + b + (2 ** 63 if b == 4 else 0) for b in range(B)] for i in range(CALLS)]
        warm = x_T.clone()
        _lib.check(lib.dws_sampler_set_clip_seeds(h, _u64([7] * B), B, _lib.current_stream()))
        run(warm)                                    # step table and graph of this shape: not left to the calls
        xs = [x_T.clone() for _ in range(2 * CALLS)]
        used = [0]

        def call(i):
            _lib.check(lib.dws_sampler_set_clip_seeds(h, _u64(tables[i]), B, _lib.current_stream()))
            call.x = xs[used[0]]
            used[0] += 1
            run(call.x)

        seq, b2b = _both_ways(gpu, call, lambda i: [call.x])
    finally:
        _lib.check(lib.dws_sampler_set_clip_seeds(h, None, 0, _lib.current_stream()))
    _assert_same(seq, b2b, "clip seeds")
    assert len({r[0].numpy().tobytes() for r in seq}) == CALLS
    assert all(torch.isfinite(r[0]).all() for r in seq)
    # and the table did mean what the Python layer means by it
    assert torch.equal(seq[3][0], smp.sampling_ddim(net, (B, 1, L), dh, S, eta=0.5, x_T=x_T, seed=tables[3]).cpu())


def test_parameter_copies_back_to_back(gpu):
    """dws_model_update_params with 1, 3, all tensors, cycled: the job count grows past a slot's first allocation.  The
    reference is a second model that gets the same values through dws_model_set_param, one call at a time."""
    from diffwave_sashimi_amd import _lib
    lib = _lib.load()
    net, L = _plain("wn_tiny", gpu)
    ref, _ = _plain("wn_tiny", gpu)
    B = 2
    g = torch.Generator().manual_seed(8)
    audio = torch.randn(B, 1, L, generator=g).to(gpu)
    steps = torch.tensor([3.0, 17.0], device=gpu)
    run_ref = lambda: ref((audio, steps.reshape(B, 1)))
    with torch.no_grad():
        net((audio, steps.reshape(B, 1)))
        names = [k for k, t in net.state_dict().items() if t.dtype == torch.float32]
        assert len(names) > 3
        counts = [1, 3, len(names)] * 3
        # call i replaces the first counts[i] tensors by values of its own
        vals = [[(torch.randn(net.state_dict()[k].shape, generator=g) * 0.1).to(gpu) for k in names[:n]] for n in counts]
        outs = [torch.empty(B, 1, L, device=gpu) for _ in range(CALLS)]
        h = net._handle
        # (one call with every tensor first, so that the device table has its final size: growing it frees the old one,
        # which waits for the GPU)
        n = len(names)
        _lib.check(lib.dws_model_update_params(h, n, (ctypes.c_char_p * n)(*[k.encode() for k in names]),
                                               (ctypes.c_void_p * n)(*[net.state_dict()[k].data_ptr() for k in names]),
                                               _lib.current_stream()))
        _lib.check(lib.dws_model_forward(h, audio.data_ptr(), steps.data_ptr(), outs[0].data_ptr(), _lib.current_stream()))
        torch.cuda.synchronize()
        busy, ahead = _Busy(gpu), False
        for i, n in enumerate(counts):
            st = _lib.current_stream()
            c_names = (ctypes.c_char_p * n)(*[k.encode() for k in names[:n]])
            c_srcs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in vals[i]])
            _lib.check(lib.dws_model_update_params(h, n, c_names, c_srcs, st))
            _lib.check(lib.dws_model_forward(h, audio.data_ptr(), steps.data_ptr(), outs[i].data_ptr(), st))
            if i == 3:
                ahead = busy.still()
        torch.cuda.synchronize()
        assert ahead, "the host did not run ahead of the GPU: the first four calls were not in flight together"
        net.invalidate()               # (the shim's version counters no longer describe what the engine holds)
        sd = ref.state_dict()
        for i, n in enumerate(counts):
            for k, t in zip(names[:n], vals[i]):
                sd[k].copy_(t)
            ref._versions = {}         # every tensor goes through dws_model_set_param again
            want = run_ref()
            torch.cuda.synchronize()
            assert torch.equal(outs[i].cpu(), want.cpu()), f"parameter copies: forward after call {i} ({n} tensors) differs"
        assert len({o.cpu().numpy().tobytes() for o in outs}) == CALLS


def test_optimizer_steps_back_to_back(gpu):
    """Alternating 5 and 1 tensors of 5 and 4097 elements (no multiple of 4; one past a chunk): parameters and moments
    after every step."""
    from diffwave_sashimi_amd import _lib
    lib = _lib.load()
    assert lib.dws_optim_chunk() == 4096
    numels = [4097, 5, 5, 4097, 5]
    g = torch.Generator().manual_seed(12)
    p0 = [torch.randn(n, generator=g) for n in numels]
    grads = [[torch.randn(n, generator=g).to(gpu) for n in numels] for _ in range(CALLS)]     # another payload per call
    vp = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def sequence(back_to_back):
        h = ctypes.c_void_p()
        _lib.check(lib.dws_optim_create(ctypes.byref(h)))
        P = [t.clone().to(gpu) for t in p0]
        M = [torch.zeros_like(t) for t in P]
        V = [torch.zeros_like(t) for t in P]
        t_of = [0] * len(P)
        snaps = []
        torch.cuda.synchronize()
        busy, ahead = (_Busy(gpu) if back_to_back else None), True
        try:
            for i in range(CALLS):
                n = 5 if i % 2 == 0 else 1      # (the first call sizes the device table: no later call frees and synchronises)
                for k in range(n):
                    t_of[k] += 1
                N = (ctypes.c_int64 * n)(*numels[:n])
                LR = (ctypes.c_double * n)(*[1e-2 * (1 + i)] * n)
                T = (ctypes.c_int64 * n)(*t_of[:n])
                _lib.check(lib.dws_optim_step(h, n, vp(P[:n]), vp(grads[i][:n]), vp(M[:n]), vp(V[:n]), None, None, N, LR, T,
                                              None, 0.9, 0.999, 1e-8, 0.0, 0.0, None, None, None, _lib.current_stream()))
                snaps.append([t.clone() for t in P + M + V])
                if not back_to_back:
                    torch.cuda.synchronize()
                elif i == CALLS - 1:
                    ahead = busy.still()
            torch.cuda.synchronize()
            assert ahead, "the host did not run ahead of the GPU: the nine steps were not in flight together"
        finally:
            _lib.check(lib.dws_optim_destroy(h))
        return [[t.cpu() for t in s] for s in snaps]

    seq, b2b = sequence(False), sequence(True)
    _assert_same(seq, b2b, "optimizer")
    # the steps did something, tensor by tensor: call 0 moves all five, call 1 tensor 0 alone
    assert all(not torch.equal(seq[0][k], p0[k]) for k in range(5))
    assert not torch.equal(seq[1][0], seq[0][0]) and all(torch.equal(seq[1][k], seq[0][k]) for k in range(1, 5))
    assert all(torch.isfinite(t).all() for s in seq for t in s)

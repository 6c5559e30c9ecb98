"""Function-level GPU parity of the ADJOINT of one WaveNet residual layer (SURVEY.md section 8, row a4 backwards: what every
WaveNet training step and every guided sampling step runs), against torch autograd through the CPU oracle in FLOAT64.

Nets A and B of tests/wnlayer.py in their adjoint form: `res_conv` = 0 in the layers before k (they are x -> x sqrt(1/2) exactly),
both ReLUs held open by 0.25, so everything around layer k is pointwise in time and a cotangent of eps reaches the layer with its
own support.  What the test sees, per case, net and cotangent (dense; N(0, 1) on the first / last w = max(2, min(d, L // 16))
positions and exact zeros elsewhere):

  audio.grad                       the data gradient of the dilated conv (`tapconv_mfma` direct, `tapwino_mfma`, generic `conv_t`),
                                   the gate adjoint epilogue, dskip = Wf^T dy
  fc_t.*, dilated_conv_layer.*,    `wgrad_mfma`, `wgrad_wino`, `wgrad_dma4` plain and split, the generic `wgrad`; the weight
  res_conv.*, skip_conv.*          gradient's in-range mask (h is zero-padded AFTER fc_t(e) was added)

  measure    `tensor_error`: max |got - ref| / max |ref| per tensor: audio.grad and layer k's eleven tensors (net A's res_conv
             gradients are exactly zero in the reference -- the last layer's residual output is unused -- and must be exactly zero)
  bounds     2e-5 for audio.grad, fc_t.weight and the three weight_v; 1e-4 for the weight_g and every bias gradient (the
             constants of tests/test_s4_convolution_adjoint_gpu.py)
  paths      f32 x {winograd, direct} and bf16x6 x {winograd, direct} on the MFMA widths; (16, 16) runs the generic adjoints.
             bf16x6 must launch split instances (launch profile "bx6"), f32 none; the paths' bits differ.
  support    where the float64 audio.grad is EXACTLY zero the engine's must be exactly zero: every product there has a zero
             factor on every path; a nonzero is stale workspace or a read outside the row
  data-only  the eval()-mode backward on the dense cotangent gives the full backward's audio.grad bit for bit

The reference side (the explicit adjoint, the support, the fp32 CPU oracle's own distance from float64 at a quarter of each
bound, seven wrong layers that break the bounds) is tests/test_wavenet_layer_reference.py.  Every test prints "WNLAYER-ADJ ..."
with the engine's error, the fp32 oracle's and their ratio before it asserts.
"""
import ctypes
import hashlib

import pytest
import torch

from tests import wnlayer as wl

pytestmark = pytest.mark.gpu

PATHS = ("f32/winograd", "f32/direct", "bf16x6/winograd", "bf16x6/direct")
GENERIC = "f32/generic"


def paths_of(C, S):
    return (GENERIC,) if (C, S) == wl.WIDTH_GENERIC else PATHS


PARAMS = [(c, w, p) for c in wl.CASES for w in ("A", "B") for p in paths_of(c[0], c[1])]
_ONE = {}             # the net, references and results of the (case, net) being tested
_DIGESTS = {}         # (case, net, path) -> digest of the dense cotangent's gradients: outlives the case's net


def _state(case, which, gpu):
    if _ONE.get("key") != (case, which):
        _ONE.clear()
        C, S, d, L, B = case
        cfg, net, audio, steps, cots, minima = wl.prepare_adjoint_case(C, S, d, L, B, which)
        assert min(minima) >= 0.25
        refs = wl.host_adjoint_references(net.state_dict(), cfg, audio, steps, d.bit_length() - 1, cots)
        net = net.to(gpu)
        net.invalidate()
        _ONE.update(key=(case, which), cfg=cfg, net=net, audio=audio, steps=steps, cots=cots, refs=refs, results={})
    return _ONE


def _backward(net, gpu, audio, steps, cot, k):
    """One forward / backward of (eps * cot).sum() with the launch profile counting the split instances ("bx6"):
    ((audio.grad, layer k's gradients or None after a data-only backward), split launches of forward + backward)."""
    from diffwave_sashimi_amd import _lib
    lib = _lib.load()
    net.zero_grad(set_to_none=True)
    a = audio.to(gpu).requires_grad_(True)
    _lib.check(lib.dws_profile_enable(b"bx6"))
    try:
        eps = net((a, steps.to(gpu)))
        eps.backward(cot.to(gpu))
        torch.cuda.synchronize()
        n, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
        _lib.check(lib.dws_profile_query(ctypes.byref(n), ctypes.byref(ms)))
    finally:
        lib.dws_profile_disable()
    named = dict(net.named_parameters())
    p = wl.block(k) + "."
    grads = None
    if named[p + wl.LAYER_KEYS[0]].grad is not None:
        grads = {key: named[p + key].grad.detach().cpu() for key in wl.LAYER_KEYS}
    return (a.grad.detach().cpu(), grads), int(n.value)


def run(case, which, path, gpu):
    st = _state(case, which, gpu)
    if path in st["results"]:
        return st["results"][path]
    k = case[2].bit_length() - 1
    net = st["net"]
    prec, _, algo = path.partition("/")
    net.set_option("precision", prec)
    net.set_option("conv_algo", "direct" if algo == "direct" else "winograd")
    net.set_option("bx6_mfma", "16x16x32")
    net.train()
    full = {name: _backward(net, gpu, st["audio"], st["steps"], st["cots"][name], k) for name in wl.COTANGENTS}
    net.eval()
    data = _backward(net, gpu, st["audio"], st["steps"], st["cots"]["dense"], k)
    st["results"][path] = dict(full=full, data=data)
    h = hashlib.sha1()
    for t in [full["dense"][0][0]] + [full["dense"][0][1][key] for key in wl.LAYER_KEYS]:
        h.update(t.contiguous().numpy().tobytes())
    _DIGESTS[(case, which, path)] = h.hexdigest()
    return st["results"][path]


@pytest.mark.parametrize("case,which,path", PARAMS, ids=[f"{wl.case_id(c)}-{w}-{p}" for c, w, p in PARAMS])
def test_layer_adjoint_against_float64(gpu, case, which, path):
    C, S, d, L, B = case
    r = run(case, which, path, gpu)
    refs = _ONE["refs"]
    failures, lines = [], []
    for name in wl.COTANGENTS:
        (got, split) = r["full"][name]
        assert got[1] is not None and torch.isfinite(got[0]).all() and got[0].shape == (B, 1, L)
        if (split > 0) != path.startswith("bf16x6"):
            failures.append(f"{name}: {split} split launches under {path}")
        ref, o32 = refs["ref"][name], refs["oracle32"][name]
        e, eo = wl.adjoint_errors(got, ref), wl.adjoint_errors(o32, ref)
        for key, v in e.items():
            if not v < wl.bound_of(key):
                failures.append(f"{name} {key}: {v:.2e} >= {wl.bound_of(key):g} (fp32 oracle {eo[key]:.2e})")
        zero = ref[0] == 0
        if name != "dense":
            assert bool(zero.any())
            stray = got[0][zero]
            if bool(stray.any()):
                failures.append(f"{name}: audio.grad holds {int((stray != 0).sum())} nonzero values (largest {float(stray.abs().max()):.2e}) "
                                f"where the float64 gradient is exactly zero")
        groups = {"audio": ("audio",), "2e-5 tensors": [q for q in wl.LAYER_KEYS if wl.bound_of(q) == wl.TIGHT_BOUND],
                  "1e-4 tensors": [q for q in wl.LAYER_KEYS if wl.bound_of(q) == wl.LOOSE_BOUND]}
        parts = []
        for g, keys in groups.items():
            key = max(keys, key=lambda q: e[q])
            parts.append(f"{g}: engine {e[key]:.2e} ({key}), fp32 oracle {max(eo[q] for q in keys):.2e}, "
                         f"ratio {e[key] / max(max(eo[q] for q in keys), 1e-300):.1f}")
        lines.append(f"{name}: " + " | ".join(parts))
    (dgot, _) = r["data"]
    assert dgot[1] is None                                             # the backward was data-only
    if not torch.equal(dgot[0], r["full"]["dense"][0][0]):
        failures.append(f"data-only and full backward differ in audio.grad by {float((dgot[0] - r['full']['dense'][0][0]).abs().max()):.2e}")
    print(f"WNLAYER-ADJ {wl.case_id(case)} net {which} {path}: " + " || ".join(lines))
    assert not failures, f"{wl.case_id(case)} net {which} {path}:\n" + "\n".join(failures)


@pytest.mark.parametrize("case,which", [(c, w) for c in wl.CASES if c[:2] != wl.WIDTH_GENERIC for w in ("A", "B")],
                         ids=lambda v: wl.case_id(v) if isinstance(v, tuple) else v)
def test_every_adjoint_path_ran_its_own_kernels(gpu, case, which):
    """conv_algo and precision switch kernels in the training step: no two paths return the same gradients bit for bit."""
    for p in PATHS:
        if (case, which, p) not in _DIGESTS:
            run(case, which, p, gpu)
    same = [(p, q) for i, p in enumerate(PATHS) for q in PATHS[:i] if _DIGESTS[(case, which, p)] == _DIGESTS[(case, which, q)]]
    assert not same, same

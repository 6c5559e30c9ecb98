"""Function-level GPU parity of ONE WaveNet residual layer, `Residual_block.forward` (`models/wavenet.py:82-121`; SURVEY.md
section 8, row a4: the code the headline benchmark runs), on every forward kernel family, against FLOAT64 and resolved by
position.

The layer with dilation d = 2^k is isolated as tests/wnlayer.py describes: net A (layer k last) gives its exact input x_k
(tap "x") and its skip output (tap "skip"), net B (layer k in the middle) its residual output (tap "x") and the middle
instance's skip output.  The float64 reference is `oracle.wavenet.residual_block` on the engine's own x_k and e (tap "emb_mlp")
of the same path, so what is judged is one layer's arithmetic and indexing, not what k layers before it left.

  measure    max |got - ref| over a position class / max |ref| over the tensor; classes head (l < d), tail (l >= L - d), seam
             (within one position of a multiple of 2d or of 64), interior (the rest); every class printed, asserted where non-empty
  paths      f32 x {winograd, direct}; bf16x6 on 32x32x16 everywhere and on gemm2-16x16x32 / 16x16x32 at (256, 256); f16x3; bf16x3;
             the generic kernel at (16, 16).  The tap "split_launches" confirms which arithmetic ran, and the paths' bits differ.
  bounds     f32, bf16x6, f16x3: 1e-5; bf16x3: 1e-4; bf16x6 in every shape: <= 2 x the f32 Winograd path's error on the same
             case, tensor and class (the rule of tests/test_bf16x6_gpu.py)
  also       a second run returns the same bits; at (d, L) = (64, 600) clip b alone equals clip b inside the batch;
             `hsave[k]` of net A after forward_train -- the gate pre-activation, the dilated conv of the zero-padded h plus bias --
             within 1e-5 of float64 under f32 / winograd, f32 / direct and bf16x6

Every case prints a line "WNLAYER ..." with each figure before anything is asserted.
"""
import hashlib

import pytest
import torch

from tests import wnlayer as wl

pytestmark = pytest.mark.gpu

F32W, F32D, GENERIC = "f32/winograd", "f32/direct", "f32/generic"
BX6 = {"bf16x6/32x32x16": "32x32x16", "bf16x6/gemm2-16x16x32": "gemm2-16x16x32", "bf16x6/16x16x32": "16x16x32"}
TRAINED = (F32W, F32D, GENERIC) + tuple(BX6)            # forward_train exists for f32 and bf16x6


def options(path):
    prec, _, rest = path.partition("/")
    return {"precision": prec, "conv_algo": "direct" if rest == "direct" else "winograd", "bx6_mfma": BX6.get(path, "32x32x16")}


def paths_of(C, S):
    if (C, S) == wl.WIDTH_GENERIC:
        return [GENERIC]                  # no MFMA instance at this width: conv_algo and the splits play no part
    wide = (C, S) == (256, 256)
    return [F32W, F32D] + [p for p in BX6 if wide or p == "bf16x6/32x32x16"] + ["f16x3", "bf16x3"]


CASE_PATHS = [(c, p) for c in wl.CASES for p in paths_of(c[0], c[1])]
_ONE_CASE = {}        # the nets and measures of the case being tested (one case at a time: the tests come case by case)
_DIGESTS = {}         # (case, path) -> digest of the bits of (x of B, skip of B, skip of A): outlives the case's nets


def _digest(tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _case_state(case, gpu):
    if _ONE_CASE.get("case") != case:
        _ONE_CASE.clear()
        C, S, d, L, B = case
        nets = {w: (cfg, net.to(gpu)) for w, (cfg, net) in wl.build_nets(C, S, d, wl.seed_of(C, S, d, L)).items()}
        for _, net in nets.values():
            net.invalidate()
        audio, steps = wl.inputs(B, L)
        _ONE_CASE.update(case=case, nets=nets, audio=audio.to(gpu), steps=steps.to(gpu), measures={},
                         sd64=wl.to_float64(nets["B"][1].state_dict()))
    return _ONE_CASE


def _forward(net, audio, steps, C, S):
    B, _, L = audio.shape
    with torch.no_grad():
        eps = net((audio, steps))
    return dict(eps=eps, x=net.read_tap("x", (B, C, L)), skip=net.read_tap("skip", (B, S, L)),
                e=net.read_tap("emb_mlp", (B, net.embed_dims[2])))


def _forward_train_hsave(net, audio, steps, k, C):
    """`hsave[k]` after dws_model_forward_train, as tests/test_bx6_pipeline_gpu.py calls it (the shape is prepared already)."""
    from diffwave_sashimi_amd import _lib
    B, _, L = audio.shape
    NL = net.num_res_layers
    x, st = audio.contiguous(), steps.float().reshape(-1).contiguous()
    out = torch.empty(B, net.out_channels, L, device=audio.device)
    _lib.check(_lib.load().dws_model_forward_train(net._handle, x.data_ptr(), st.data_ptr(), out.data_ptr(), _lib.current_stream()))
    return out, net.read_tap("hsave", (NL, B, 2 * C, L))[k]


def measure(case, path, gpu):
    """Everything one path gives on one case: dict(errors={tensor: {class: error}}, hsave={class: error} or None,
    failures=[...]).  Cached for the case; the digest of its bits is kept in _DIGESTS."""
    st = _case_state(case, gpu)
    if path in st["measures"]:
        return st["measures"][path]
    C, S, d, L, B = case
    k = d.bit_length() - 1
    audio, steps = st["audio"], st["steps"]
    failures, runs = [], {}
    split = not path.startswith("f32")
    for which, (cfg, net) in st["nets"].items():
        for key, value in options(path).items():
            net.set_option(key, value)
        r = runs[which] = _forward(net, audio, steps, C, S)
        NL = cfg["num_res_layers"]
        ran = net.read_tap("split_launches", (2,)).cpu().tolist()
        if ran != ([NL, 0] if split else [0, NL]):
            failures.append(f"net {which}: split_launches {ran}, expected {'split' if split else 'exact f32'} on {NL} layers")
        r2 = _forward(net, audio, steps, C, S)
        if not all(torch.equal(r[t], r2[t]) for t in ("eps", "x", "skip")):
            failures.append(f"net {which}: a second run gives other bits")
        if (d, L) == (64, 600):                                     # tile numbers of a clip's workgroups differ alone / in a batch
            for b in range(B):
                one = _forward(net, audio[b:b + 1].contiguous(), steps[b:b + 1].contiguous(), C, S)
                if not all(torch.equal(one[t][0], r[t][b]) for t in ("eps", "x", "skip")):
                    failures.append(f"net {which}: clip {b} alone differs from clip {b} in the batch")
            _forward(net, audio, steps, C, S)                       # (the batch's shape and taps again)
    a, b = runs["A"], runs["B"]
    assert torch.equal(a["e"], b["e"])
    x_k, e = a["x"].cpu(), a["e"].cpu()
    ref = wl.forward_reference(st["sd64"], k, x_k, e)
    errors = {"B.x": wl.class_errors(b["x"].cpu(), ref["x_out"], d), "B.skip": wl.class_errors(b["skip"].cpu(), ref["skip"], d),
              "A.skip": wl.class_errors(a["skip"].cpu(), ref["skip"], d)}
    hsave = None
    if path in TRAINED:
        net = st["nets"]["A"][1]
        out, H = _forward_train_hsave(net, audio, steps, k, C)
        hsave = wl.class_errors(H.cpu(), ref["H"], d)
        if not torch.isfinite(out).all():
            failures.append("forward_train: eps is not finite")
    m = st["measures"][path] = dict(errors=errors, hsave=hsave, failures=failures)
    _DIGESTS[(case, path)] = _digest((b["x"], b["skip"], a["skip"]))
    fmt = lambda ce: " ".join(f"{c} {'-' if v is None else format(v, '.2e')}" for c, v in ce.items())
    print(f"WNLAYER {wl.case_id(case)} {path}: " + " | ".join(f"{t}: {fmt(ce)}" for t, ce in errors.items())
          + (f" | hsave[k]: {fmt(hsave)}" if hsave else ""))
    return m


@pytest.mark.parametrize("case,path", CASE_PATHS, ids=[f"{wl.case_id(c)}-{p}" for c, p in CASE_PATHS])
def test_layer_outputs_against_float64(gpu, case, path):
    m = measure(case, path, gpu)
    bound = wl.BF16X3_BOUND if path == "bf16x3" else wl.FORWARD_BOUND
    failures = list(m["failures"])
    judged = dict(m["errors"], **({"hsave[k]": m["hsave"]} if m["hsave"] else {}))
    for tensor, ce in judged.items():
        assert any(v is not None for v in ce.values())
        for cls, v in ce.items():
            if v is not None and not v < bound:
                failures.append(f"{tensor} {cls}: {v:.2e} >= {bound:g}")
    if path in BX6:
        base = measure(case, F32W, gpu)["errors"]
        for tensor, ce in m["errors"].items():
            for cls, v in ce.items():
                if v is not None and not v <= wl.BX6_OVER_F32 * base[tensor][cls]:
                    failures.append(f"{tensor} {cls}: {v:.2e} > 2 x the f32 Winograd path's {base[tensor][cls]:.2e}")
    assert not failures, f"{wl.case_id(case)} {path}:\n" + "\n".join(failures)


@pytest.mark.parametrize("case", [c for c in wl.CASES if c[:2] != wl.WIDTH_GENERIC], ids=wl.case_id)
def test_every_path_ran_its_own_kernel(gpu, case):
    """The options switch kernels: no two paths of a case return the same bits."""
    paths = paths_of(case[0], case[1])
    for p in paths:
        if (case, p) not in _DIGESTS:
            measure(case, p, gpu)
    same = [(p, q) for i, p in enumerate(paths) for q in paths[:i] if _DIGESTS[(case, p)] == _DIGESTS[(case, q)]]
    assert not same, same

"""Shared pieces of the WaveNet layer tests (tests/test_wavenet_layer_reference.py, test_wavenet_layer_gpu.py,
test_wavenet_layer_adjoint_gpu.py): ONE residual layer (`models/wavenet.py:82-121`) and its adjoint,
isolated inside a network, against float64.

Isolation.  The dilation of layer n is 1 << (n % cycle): d = 2^k is first reached at layer k.  With cycle = k + 1
  net A   num_res_layers = k + 1: layer k is the LAST layer (no residual row stored; first and last at once for k = 0),
          tap "x" = its exact input x_k, tap "skip" = its skip output
  net B   num_res_layers = k + 2: layer k is a MIDDLE layer, followed by an ordinary d = 1 layer,
          tap "x" = its residual output (x_k + res) sqrt(1/2), tap "skip" = its skip output
once `skip_conv.weight_g` and `skip_conv.bias` are zero in every layer but k (an all-zero weight matrix is a legal state).
A holds B's tensors, so x_k is the same in both.  For the adjoint `res_conv.weight_g` / `.bias` of layers 0 .. k-1 are zero as
well: those layers are x -> x sqrt(1/2) exactly, both ReLUs are held open (`open_relus`), and everything around layer k is
pointwise in time -- except, in net B, layer k + 1, which keeps its skip output and widens a cotangent's footprint by one
position on either side.

The zero-padding rule: h = x + fc_t(e) is padded with ZEROS, i.e. fc_t(e) belongs to the padded tensor.  `layer_block` writes
the layer out tap by tap on the padded h (the oracle's `residual_block` is the same function; asserted on the CPU), with the
switches that make it wrong on purpose (MUTATIONS), the adjoint ones through `_Conv3`, an explicit adjoint of the three-tap
convolution."""
import contextlib
import math

import torch
import torch.nn.functional as F

from oracle import wavenet as own
from tests import cases
from tests.s4conv import tensor_error, to_float64          # noqa: F401  (re-exported: the tests' measures)

SQH = math.sqrt(0.5)
WEIGHT_SEED, INPUT_SEED, COTANGENT_SEED = 5, 78, 91
RELU_BIASES = ("init_conv.0.conv.bias", "final_conv.0.conv.bias")
COTANGENTS = ("dense", "head", "tail")
CLASSES = ("head", "tail", "seam", "interior")

# bounds: what the project already holds these kernels to (tests/test_bx6_pipeline_gpu.py, test_wavenet_gpu.py; the S4 adjoint
# tests' constants), now per layer and against float64
FORWARD_BOUND = 1e-5            # f32 direct / winograd, bf16x6, f16x3
BF16X3_BOUND = 1e-4
BX6_OVER_F32 = 2.0              # bf16x6 error <= 2 x the f32 Winograd path's, same case and class (tests/test_bf16x6_gpu.py)
TIGHT_BOUND, LOOSE_BOUND = 2e-5, 1e-4
LAYER_KEYS = ("fc_t.weight", "fc_t.bias") + tuple(f"{m}.{t}" for m in ("dilated_conv_layer.conv", "res_conv", "skip_conv")
                                                   for t in ("bias", "weight_g", "weight_v"))


def bound_of(key):
    """audio.grad, fc_t.weight and the three weight_v: 2e-5; the weight_g and every bias gradient (position sums): 1e-4."""
    return TIGHT_BOUND if key in ("audio", "fc_t.weight") or key.endswith("weight_v") else LOOSE_BOUND


# (C, S): generic kernels | 2 waves | skip tiles fetched in the epilogue | the preloading instance | 8 waves, chunks by halves
WIDTHS_ALL, WIDTHS_SOME, WIDTH_GENERIC = ((256, 256), (64, 64)), ((128, 256), (128, 128)), (16, 16)
# (d, L): one partial tile, L % 4 != 0 | d < 32: interleaved pairs | last d on the contiguous-row form, L % 2d != 0 | first d
# with separate halves | block-fastest tile order, halos in both neighbours | one and a half blocks | d > L: the fc_t
# indicator and the centre tap alone | exactly four positions own an in-range outer tap
SHAPES = ((1, 63), (4, 200), (16, 333), (32, 336), (64, 600), (256, 600), (2048, 600), (2048, 2052))
SHAPES_SOME = ((1, 63), (64, 600), (2048, 2052))


def _batch(d, L):
    return 3 if (d, L) == (64, 600) else 2


CASES = ([(C, S, d, L, _batch(d, L)) for C, S in WIDTHS_ALL for d, L in SHAPES]
         + [(C, S, d, L, _batch(d, L)) for C, S in WIDTHS_SOME for d, L in SHAPES_SOME]
         + [WIDTH_GENERIC + (d, L, _batch(d, L)) for d, L in SHAPES_SOME if d <= 64])
# Weight seeds other than WEIGHT_SEED, (C, S, d, L) -> seed: the first seed from 5 on at which the case meets the fp32-oracle
# conditions of tests/test_wavenet_layer_reference.py with 20 % room (fp32 CPU oracle <= 0.8 x a quarter of every adjoint bound,
# nets A and B, the three cotangents; <= 0.8 x an eighth of the forward bound in every class) -- conditions on the float64
# reference and the fp32 CPU oracle alone.  No entry: with cotangents that pass `cotangent_sum_is_typical` every case meets
# the adjoint condition at seed 5 (worst 6.3e-6 of 2.5e-5 on a weight_g, 2.0e-6 of 5e-6 on a 2e-5 tensor) and, with the fp32
# oracle of the forward on one thread (`one_thread`), the forward condition too (worst 7.7e-7 of 1.25e-6).
SEEDS = {}


def seed_of(C, S, d, L):
    return SEEDS.get((C, S, d, L), WEIGHT_SEED)


def case_id(c):
    return "C%d_S%d_d%d_L%d_B%d" % tuple(c)


def block(n):
    return f"residual_layer.residual_blocks.{n}"


def layer_cfg(C, S, k, which):
    return cases.wn_cfg(res_channels=C, skip_channels=S, num_res_layers=k + (2 if which == "B" else 1), dilation_cycle=k + 1)


def build_nets(C, S, d, seed, adjoint=False):
    """{"A": (cfg, net), "B": (cfg, net)} on the host, eval mode.  Forward form: skip_conv = 0 in every layer but k.  Adjoint
    form: layer k + 1 of net B keeps its skip output, res_conv = 0 in layers 0 .. k-1."""
    k = d.bit_length() - 1
    assert d == 1 << k
    cfgA, cfgB = layer_cfg(C, S, k, "A"), layer_cfg(C, S, k, "B")
    netA, netB = cases.build_ours(cfgA, seed), cases.build_ours(cfgB, seed)
    sdA, sdB = netA.state_dict(), netB.state_dict()
    with torch.no_grad():
        for n in range(k + 2):
            if n != k and not (adjoint and n == k + 1):
                sdB[block(n) + ".skip_conv.weight_g"].zero_()
                sdB[block(n) + ".skip_conv.bias"].zero_()
            if adjoint and n < k:
                sdB[block(n) + ".res_conv.weight_g"].zero_()
                sdB[block(n) + ".res_conv.bias"].zero_()
        for key, v in sdA.items():
            if v.is_floating_point():
                v.copy_(sdB[key])
    netA.invalidate(), netB.invalidate()
    return {"A": (cfgA, netA), "B": (cfgB, netB)}


def inputs(B, L):
    audio, steps = cases.wavenet_inputs(B, L, 1, INPUT_SEED)
    assert all(not torch.equal(audio[a], audio[b]) for a in range(B) for b in range(a))      # clips of a batch differ
    return audio, steps


# ------------------------------------------------------------------------------------------------- the layer, written out
MUTATIONS = ("fc_t leaks into the padding", "outer tap dropped at l = L - 1 - d", "W0 and W2 swapped",
             "tanh and sigmoid halves swapped", "sqrt(1/2) missing on the residual output",
             "weight gradient's outer taps see the unmasked h", "data gradient correlates with +d")
FORWARD_MUTATIONS, ADJOINT_MUTATIONS = MUTATIONS[:5], MUTATIONS[5:]


class _Conv3(torch.autograd.Function):
    """H[b, o, l] = bias[o] + sum_t sum_c W[o, c, t] hp[b, c, l + (t - 1) d], hp = h outside [0, L) replaced by `padval`
    [B, C, 1] (zeros: the layer's rule), with its adjoint written out:
        dh[b, c, l]  = sum_t sum_o W[o, c, t] dH[b, o, l - (t - 1) d]            (dH zero outside [0, L))
        dW[o, c, t]  = sum_{b, l} dH[b, o, l] hp[b, c, l + (t - 1) d]
    `wrong`: one of ADJOINT_MUTATIONS, or None; `leak` [B, C, 1] is fc_t(e), what an unmasked h holds in the padding."""

    @staticmethod
    def forward(ctx, h, W, bias, padval, leak, d, wrong):
        L = h.shape[-1]
        hp = F.pad(h - padval, (d, d)) + padval if bool(padval.any()) else F.pad(h, (d, d))
        ctx.save_for_backward(hp, W, leak)
        ctx.d, ctx.wrong, ctx.L = d, wrong, L
        H = bias.reshape(1, -1, 1)
        for t in range(3):
            H = H + torch.einsum("oc,bcl->bol", W[:, :, t], hp[..., t * d:t * d + L])
        return H

    @staticmethod
    def backward(ctx, dH):
        hp, W, leak = ctx.saved_tensors
        d, L, wrong = ctx.d, ctx.L, ctx.wrong
        dHp = F.pad(dH, (d, d))
        dh = torch.zeros_like(hp[..., :L])
        dW = torch.zeros_like(W)
        hpw = hp
        if wrong == ADJOINT_MUTATIONS[0]:          # the padding holds fc_t(e), as if the in-range indicator were missing
            hpw = hp.clone()
            hpw[..., :d] += leak
            hpw[..., d + L:] += leak
        for t in range(3):
            shift = (t - 1) * d if wrong == ADJOINT_MUTATIONS[1] else -(t - 1) * d
            dh = dh + torch.einsum("oc,bol->bcl", W[:, :, t], dHp[..., d + shift:d + shift + L])
            dW[:, :, t] = torch.einsum("bol,bcl->oc", dH, (hp if t == 1 else hpw)[..., t * d:t * d + L])
        return dh, dW, dH.sum((0, 2)), None, None, None, None


def layer_block(sd, prefix, x, e, d, wrong=None):
    """`Residual_block.forward` tap by tap on the zero-padded h: dict(x_out, skip, H, h), H the gate pre-activation.
    wrong: one of MUTATIONS (None: the layer)."""
    B, C, L = x.shape
    part_t = F.linear(e, sd[prefix + ".fc_t.weight"], sd[prefix + ".fc_t.bias"]).reshape(B, C, 1)
    h = x + part_t
    W = own.weight_norm_weight(sd, prefix + ".dilated_conv_layer.conv")
    if wrong == MUTATIONS[2]:
        W = W.flip(-1)
    padval = part_t.detach() if wrong == MUTATIONS[0] else torch.zeros_like(part_t)
    H = _Conv3.apply(h, W, sd[prefix + ".dilated_conv_layer.conv.bias"], padval, part_t.detach(), d,
                     wrong if wrong in ADJOINT_MUTATIONS else None)
    if wrong == MUTATIONS[1] and L - 1 - d >= 0:          # the last position that owns a +d tap loses it
        H = H.clone()
        H[..., L - 1 - d] -= torch.einsum("oc,bc->bo", W[:, :, 2], h[..., L - 1])
    a, g = (H[:, C:], H[:, :C]) if wrong == MUTATIONS[3] else (H[:, :C], H[:, C:])
    out = torch.tanh(a) * torch.sigmoid(g)
    res = own.wn_conv1d(sd, prefix + ".res_conv", out)
    skip = own.wn_conv1d(sd, prefix + ".skip_conv", out)
    return dict(x_out=(x + res) * (1.0 if wrong == MUTATIONS[4] else SQH), skip=skip, H=H, h=h)


def layer_forward(sd, cfg, audio, steps, k, wrong=None, explicit=None):
    """The isolated layer's network in the ADJOINT form from the oracle's pieces, in sd's precision, every node in the graph:
    x_k = sqrt(1/2)^k relu(init conv), layer k, layer k + 1 in net B, the final stage.  dict(x_k, e, x_out, skip_k, pre, eps)
    (+ H, h of layer k when it goes through `layer_block`: explicit=True, or a mutation)."""
    dt = sd[RELU_BIASES[0]].dtype
    NL, d = cfg["num_res_layers"], 1 << k
    assert NL in (k + 1, k + 2) and cfg["dilation_cycle"] == k + 1
    pre0 = own.wn_conv1d(sd, "init_conv.0.conv", audio.to(dt))
    e = own.step_embedding_mlp(sd, "residual_layer.", steps, cfg["diffusion_step_embed_dim_in"])
    x_k = F.relu(pre0) * SQH ** k
    n = dict(x_k=x_k, e=e, pre0=pre0)
    if explicit or wrong is not None:
        n.update(layer_block(sd, block(k), x_k, e, d, wrong))
    else:
        n["x_out"], n["skip"] = own.residual_block(sd, block(k), x_k, e, d)
    skip = n["skip"]
    if NL == k + 2:
        skip = skip + own.residual_block(sd, block(k + 1), n["x_out"], e, 1)[1]
    n["pre"] = own.wn_conv1d(sd, "final_conv.0.conv", skip * math.sqrt(1.0 / NL))
    n["eps"] = F.conv1d(F.relu(n["pre"]), sd["final_conv.2.conv.weight"], sd["final_conv.2.conv.bias"])
    return n


def relu_minima(sd, cfg, audio, steps, k):
    """The smallest float64 pre-activation of the init conv's ReLU and of the final conv's."""
    with torch.no_grad():
        n = layer_forward(to_float64(sd), cfg, audio.double(), steps, k)
    return float(n["pre0"].min()), float(n["pre"].min())


def open_relus(sd, cfg, audio, steps, k, margin=0.25):
    """Adds one constant to every entry of `init_conv.0.conv.bias` and one to `final_conv.0.conv.bias` (in place: pass the
    module's own state_dict): the smallest shifts, multiples of 1/16 (exact in fp32), that leave every float64 pre-activation
    of both ReLUs >= margin on these inputs.  Returns the two minima after the shift."""
    with torch.no_grad():
        for i, key in enumerate(RELU_BIASES):         # the init conv first: the final conv sees the shifted x
            lo = relu_minima(sd, cfg, audio, steps, k)[i]
            if lo < margin + 0.05:
                sd[key].add_(math.ceil((margin + 0.05 - lo) * 16.0) / 16.0)
    lo = relu_minima(sd, cfg, audio, steps, k)
    assert min(lo) >= margin, lo
    return lo


# ------------------------------------------------------------------------------------------------- cotangents, support
def support_width(d, L):
    return max(2, min(d, L // 16))


def _draw_cotangents(B, d, L, seed):
    g = torch.Generator().manual_seed(seed)
    w = support_width(d, L)
    dense, head, tail = torch.randn(B, 1, L, generator=g), torch.zeros(B, 1, L), torch.zeros(B, 1, L)
    head[..., :w] = torch.randn(B, 1, w, generator=g)
    tail[..., L - w:] = torch.randn(B, 1, w, generator=g)
    return {"dense": dense, "head": head, "tail": tail}


def cotangent_sum_is_typical(c):
    """|sum c| >= half its standard deviation sqrt(n) over the n entries drawn.  With both ReLUs open the network around layer
    k is affine in time-constant coefficients, so every bias gradient -- and with x carrying the opened ReLU's constant shift,
    the bulk of every weight gradient -- is (a per-channel constant) x sum_l c[l]: a draw whose own sum cancels to 1e-3 of
    sum |c| (seed 91 gives -0.7 against 968 at B = 2, L = 600) leaves gradients that are cancellation residue in ANY fp32
    summation, the CPU oracle's included (5e-5 on skip_conv.bias there).  A condition on the cotangent alone."""
    n = int((c != 0).sum())
    return abs(float(c.double().sum())) >= 0.5 * math.sqrt(n)


def cotangent_seed(B, d, L):
    """The first seed from COTANGENT_SEED on whose three cotangents all pass `cotangent_sum_is_typical`."""
    seed = COTANGENT_SEED
    while not all(cotangent_sum_is_typical(c) for c in _draw_cotangents(B, d, L, seed).values()):
        seed += 1
    return seed


def edge_cotangents(B, d, L):
    """{"dense": N(0, 1), "head": N(0, 1) on the first w = max(2, min(d, L // 16)) positions and exact zeros elsewhere,
    "tail": the same on the last w}, each [B, 1, L]: the window fits the stencil (w <= d keeps the two images apart)."""
    return _draw_cotangents(B, d, L, cotangent_seed(B, d, L))


def footprint(name, which, d, L):
    """Bool mask [L] of the positions a cotangent's audio gradient may occupy (None: all).  The cotangent reaches layer k's
    gate pre-activation on its own window -- net A: [0, w) for the head; net B: one position more on each side, layer k + 1
    being a d = 1 convolution -- and the transposed convolution adds the window's image at +d (what of the other image, at -d,
    is not before the clip lies inside the window).  The tail is the mirror image."""
    if name == "dense":
        return None
    w, m = support_width(d, L), torch.zeros(L, dtype=torch.bool)
    grow = 1 if which == "B" else 0
    lo, hi = (0, min(L, w + grow)) if name == "head" else (max(0, L - w - grow), L)
    for s in (0, d if name == "head" else -d):
        a, b = max(0, lo + s), min(L, hi + s)
        if a < b:
            m[a:b] = True
    return m


def position_classes(d, L):
    """{"head": l < d, "tail": l >= L - d, "seam": within one position of a multiple of 2d or of 64, "interior": the rest}
    as bool masks [L] (head, tail and seam may overlap)."""
    l = torch.arange(L)
    near = lambda m: (l % m <= 1) | (l % m == m - 1)
    head, tail, seam = l < d, l >= L - d, near(2 * d) | near(64)
    return {"head": head, "tail": tail, "seam": seam, "interior": ~(head | tail | seam)}


def class_errors(got, ref, d):
    """max |got - ref| over the class / max |ref| over the tensor, per position class (None: the class is empty)."""
    diff = (got.double() - ref.double()).abs()
    top = max(float(ref.abs().max()), 1e-300)
    return {c: (float(diff[..., m].max()) / top if bool(m.any()) else None) for c, m in position_classes(d, ref.shape[-1]).items()}


# ------------------------------------------------------------------------------------------------- references
def forward_reference(sd64, k, x_k, e):
    """Float64 layer k on the engine's own input: dict(x_out, skip, H) from x_k (net A's tap "x") and e (tap "emb_mlp")."""
    with torch.no_grad():
        x_out, skip = own.residual_block(sd64, block(k), x_k.double(), e.double(), 1 << k)
        H = layer_block(sd64, block(k), x_k.double(), e.double(), 1 << k)["H"]
    return dict(x_out=x_out, skip=skip, H=H)


def oracle_input(sd, cfg, audio, steps, k):
    """(x_k, e) of the FORWARD form by the fp32 CPU oracle: the init conv and layers 0 .. k-1 with their random res_conv."""
    sd32 = {key: v.detach().cpu() for key, v in sd.items()}
    with torch.no_grad():
        x = F.relu(own.wn_conv1d(sd32, "init_conv.0.conv", audio))
        e = own.step_embedding_mlp(sd32, "residual_layer.", steps, cfg["diffusion_step_embed_dim_in"])
        for n in range(k):
            x, _ = own.residual_block(sd32, block(n), x, e, 1 << n)
    return x, e


def _leaves(sd, dtype):
    return {k: (v.detach().cpu().clone().to(dtype).requires_grad_(True) if v.is_floating_point() else v.detach().cpu().clone())
            for k, v in sd.items()}


def adjoint_reference(sd, cfg, audio, steps, k, cots, dtype=torch.float64, wrong=None, explicit=None):
    """{cotangent: (audio.grad, {key of LAYER_KEYS: gradient})} of the loss (eps * cot).sum() by torch autograd through
    `layer_forward` on the `dtype` copy of sd, in float64.  cots: a dict of cotangents [B, 1, L] served by one forward."""
    leaf = _leaves(sd, dtype)
    a = audio.detach().to(dtype).requires_grad_(True)
    eps = layer_forward(leaf, cfg, a, steps, k, wrong, explicit)["eps"]
    params = [leaf[block(k) + "." + key] for key in LAYER_KEYS]
    out = {}
    for i, (name, c) in enumerate(cots.items()):
        gs = torch.autograd.grad((eps * c.to(dtype)).sum(), [a] + params, retain_graph=i + 1 < len(cots), allow_unused=True)
        out[name] = (gs[0].detach().double(), {key: (torch.zeros_like(p) if g is None else g).detach().double()
                                               for key, p, g in zip(LAYER_KEYS, params, gs[1:])})
    return out


def prepare_adjoint_case(C, S, d, L, B, which):
    """(cfg, net on the host with both ReLUs opened, audio, steps, cotangents, the two ReLU minima) of one case and net."""
    cfg, net = build_nets(C, S, d, seed_of(C, S, d, L), adjoint=True)[which]
    audio, steps = inputs(B, L)
    minima = open_relus(net.state_dict(), cfg, audio, steps, d.bit_length() - 1)
    net.invalidate()
    return cfg, net, audio, steps, edge_cotangents(B, d, L), minima


def adjoint_errors(got, ref):
    """{"audio": ..., key: ...}: `tensor_error` of the audio gradient and of layer k's tensors.  got / ref: (audio.grad, grads).
    A tensor whose reference is exactly zero (net A: the last layer's res_conv) must be exactly zero: error 0 or inf."""
    out = {"audio": tensor_error(got[0], ref[0])}
    for key in LAYER_KEYS:
        g, r = got[1][key], ref[1][key]
        out[key] = tensor_error(g, r) if bool(r.any()) else (0.0 if not bool(g.any()) else float("inf"))
    return out


@contextlib.contextmanager
def one_thread():
    """torch's intra-op pool at one thread, for the fp32 oracle of the forward.  `F.conv1d` with a kernel of one tap and a bias
    runs oneDNN's jit_1x1 convolution, which on more than one thread starts every accumulator from the bias: behind many layers
    the res / skip outputs are |bias| 0.06 plus a 256-term sum of 0.01, so each addition rounds at the bias's ulp and the error is
    8.6e-7 of sum |a||b| where the same call on one thread -- or `F.conv1d(x, W) + b`, or a matmul, on any number -- leaves
    2.9e-7 (random operands of those sizes, 2 x 256 x 600 outputs).  Which of the two a run gets depends on the host's CPU
    count; a condition on the reference must not."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def host_adjoint_references(sd, cfg, audio, steps, k, cots):
    """dict(ref, oracle32): the float64 reference and the fp32 CPU oracle through the same graph, per cotangent."""
    sd = {key: v.detach().cpu() for key, v in sd.items()}
    return dict(ref=adjoint_reference(sd, cfg, audio, steps, k, cots),
                oracle32=adjoint_reference(sd, cfg, audio, steps, k, cots, dtype=torch.float32))


def oracle_figures(C, S, d, L, B, seed):
    """What the fp32 CPU oracle leaves against float64 on one case at one weight seed, in the GPU tests' measures:
    dict(forward={class: worst of x_out / skip}, adjoint={key: worst over nets and cotangents}, minima={net: (min, min)}).
    `forward` is evaluated on one intra-op thread (`one_thread` says why), `forward_pool` on the pool as it stands."""
    k = d.bit_length() - 1
    audio, steps = inputs(B, L)
    cfg, net = build_nets(C, S, d, seed)["B"]
    sd = net.state_dict()
    x_k, e = oracle_input(sd, cfg, audio, steps, k)
    ref = forward_reference(to_float64(sd), k, x_k, e)
    sd32 = {key: v.detach() for key, v in sd.items()}

    def forward_errors():
        with torch.no_grad():
            x32, s32 = own.residual_block(sd32, block(k), x_k, e, d)
        out = {}
        for got, want in ((x32, ref["x_out"]), (s32, ref["skip"])):
            for c, v in class_errors(got, want, d).items():
                if v is not None:
                    out[c] = max(out.get(c, 0.0), v)
        return out

    with one_thread():
        fwd = forward_errors()
    fwd_pool = forward_errors()
    adj, minima = {}, {}
    for which, (cfg, net) in build_nets(C, S, d, seed, adjoint=True).items():
        sd = net.state_dict()
        minima[which] = open_relus(sd, cfg, audio, steps, k)
        refs = host_adjoint_references(sd, cfg, audio, steps, k, edge_cotangents(B, d, L))
        for name in COTANGENTS:
            for key, v in adjoint_errors(refs["oracle32"][name], refs["ref"][name]).items():
                adj[key] = max(adj.get(key, 0.0), v)
    return dict(forward=fwd, forward_pool=fwd_pool, adjoint=adj, minima=minima)


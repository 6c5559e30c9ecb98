"""Shared pieces of the S4 long-convolution tests (tests/test_s4_convolution_gpu.py, tests/test_s4_convolution_reference.py):
a one-block network whose tail is transparent to the S4 branch, and the float64 host evaluation of that branch

    GELU(conv(u, k) + D u),   conv(u, k)[i] = sum_{j<=i} k0[j] u[i-j] + sum_{m>=1} k1[m-1] u[i+m]      (`s4.py:1391-1437`)

with u = LN1(x) + fc_t(e), x = relu(init_conv(audio)).  The taps k come from the caller (the engine's own `k:` tap in the
GPU tests), so the comparison judges the convolution, not the kernel generator.  The second half of the file is the
reference of the convolution's adjoint (tests/test_s4_convolution_adjoint_gpu.py, ..._adjoint_reference.py)."""
import math

import torch
import torch.nn.functional as F

from oracle import sashimi as oss
from oracle import wavenet as own
from tests import cases

BLOCK = "c_layers.0"
WEIGHT_SEED, INPUT_SEED = 5, 78
GATE_BIAS = 30.0            # sigmoid(30) = 1 - 9.4e-14: 1.0 in fp32, the GLU returns its first half unchanged


def block_cfg(H, Lcfg):
    return cases.ss_cfg(d_model=H, n_layers=1, L=Lcfg, pool=[], unet=False, diffusion_step_embed_dim_mid=64)


def build_isolated_block(H, Lcfg, weight_seed=WEIGHT_SEED):
    """(cfg, net) on the host: FF branch exactly 0, output_linear = [I; 0] with the gate held open, kernels with long
    memory (dt = linspace(0.5, 4, H) / Lcfg: the far taps carry weight), C through `_setup_C` at l_max = Lcfg."""
    cfg = block_cfg(H, Lcfg)
    net = cases.build_ours(cfg, weight_seed)
    sd = net.state_dict()
    with torch.no_grad():
        sd[BLOCK + ".ff.ff.2.conv.weight_g"].zero_()
        sd[BLOCK + ".ff.ff.2.conv.bias"].zero_()
        W, b = sd[BLOCK + ".layer.output_linear.0.weight"], sd[BLOCK + ".layer.output_linear.0.bias"]
        W.zero_()
        W[:H, :, 0] = torch.eye(H)
        b[:H] = 0.0
        b[H:] = GATE_BIAS
        sd[BLOCK + ".layer.kernel.kernel.log_dt"].copy_(torch.log(torch.linspace(0.5, 4.0, H) / Lcfg))
    net._setup_C()
    net.invalidate()
    return cfg, net


def tail_is_transparent(sd, H):
    """The identity / gate / zero-FF parameters read back exactly (sd: a state_dict on any device)."""
    W = sd[BLOCK + ".layer.output_linear.0.weight"].detach().cpu()
    b = sd[BLOCK + ".layer.output_linear.0.bias"].detach().cpu()
    return (tuple(W.shape) == (2 * H, H, 1) and torch.equal(W[:H, :, 0], torch.eye(H)) and not bool(W[H:].any())
            and not bool(b[:H].any()) and bool((b[H:] == GATE_BIAS).all())
            and not bool(sd[BLOCK + ".ff.ff.2.conv.weight_g"].any()) and not bool(sd[BLOCK + ".ff.ff.2.conv.bias"].any())
            and float(torch.sigmoid(torch.tensor(GATE_BIAS))) == 1.0)


def two_sided_conv_fft(u, k0, k1):
    """conv(u, k) in float64 through one FFT of size n >= L + Lt (a power of two).  u [..., H, L], k0 / k1 [H, Lt]: the
    causal taps sit at 0 .. Lt-1 of the circular kernel, the anti-causal tap m at n - m; u's zero padding of n - L >= Lt
    samples keeps either half from wrapping onto the row."""
    assert u.dtype == k0.dtype == k1.dtype == torch.float64
    L, Lt = u.shape[-1], k0.shape[-1]
    n = 1 << (L + Lt - 1).bit_length()
    assert n >= L + Lt
    kk = torch.zeros(k0.shape[:-1] + (n,), dtype=torch.float64)
    kk[..., :Lt] = k0
    kk[..., n - Lt:] += k1.flip(-1)
    return torch.fft.irfft(torch.fft.rfft(u, n=n) * torch.fft.rfft(kk, n=n), n=n)[..., :L]


def two_sided_conv_direct(u, k0, k1):
    """The definition, term by term (O(L^2) per row; small shapes only)."""
    L, Lt = u.shape[-1], k0.shape[-1]
    uf = u.reshape(-1, u.shape[-2], L)
    y = torch.zeros_like(uf)
    for b in range(uf.shape[0]):
        for h in range(uf.shape[1]):
            ur, c, a = uf[b, h].tolist(), k0[h].tolist(), k1[h].tolist()
            for i in range(L):
                acc = 0.0
                for j in range(min(i + 1, Lt)):
                    acc += c[j] * ur[i - j]
                for m in range(1, min(L - 1 - i, Lt) + 1):
                    acc += a[m - 1] * ur[i + m]
                y[b, h, i] = acc
    return y.reshape(u.shape)


def gelu_erf(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


def s4_branch(u, k0, k1, D, conv=two_sided_conv_fft):
    """(GELU(conv + D u), conv, D u) in float64; D [1, H]."""
    c = conv(u, k0, k1)
    du = D.reshape(-1, 1) * u
    return gelu_erf(c + du), c, du


def to_float64(sd):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in sd.items()}


def block_input(sd, cfg, audio, steps):
    """(x, e, u) from the oracle's pieces, in sd's precision: x = relu(init_conv(audio)), e the embedding MLP's output,
    u = LN1(x) + fc_t(e)."""
    dt = sd["init_conv.0.conv.bias"].dtype
    x = F.relu(own.wn_conv1d(sd, "init_conv.0.conv", audio.to(dt)))
    e = own.step_embedding_mlp(sd, "", steps, cfg["diffusion_step_embed_dim_in"])
    u = oss.transposed_ln(x, sd[BLOCK + ".norm1.m"], sd[BLOCK + ".norm1.s"])
    u = u + F.linear(e, sd[BLOCK + ".fc_t.weight"], sd[BLOCK + ".fc_t.bias"]).unsqueeze(-1)
    return x, e, u


def taps_from_engine(k_tap, L):
    """The engine's `k:` tap holds Lk * k, [2, H, Lk]: float64 taps, the first Lt = min(L, Lk) per direction."""
    Lk = k_tap.shape[-1]
    k = k_tap.detach().cpu().double() / Lk
    Lt = min(L, Lk)
    return k[0, :, :Lt].contiguous(), k[1, :, :Lt].contiguous()


def reference(sd, cfg, audio, steps, k_tap):
    """Float64 reference of `out:c_layers.0 - 2x` for the isolated block: dict(x, u, k0, k1, conv, du, ref)."""
    sd64 = to_float64(sd)
    with torch.no_grad():
        x, _, u = block_input(sd64, cfg, audio, steps)
        k0, k1 = taps_from_engine(k_tap, audio.shape[-1])
        ref, conv, du = s4_branch(u, k0, k1, sd64[BLOCK + ".layer.D"])
    return dict(x=x, u=u, k0=k0, k1=k1, conv=conv, du=du, ref=ref)


def oracle_fp32_branch(sd, cfg, audio, steps, x64):
    """The fp32 CPU oracle through the same isolation: (diffwave_block(x) + x) - 2 x, the subtraction as for the engine."""
    sd32 = {k: v.detach().cpu() for k, v in sd.items()}
    with torch.no_grad():
        x, e, _ = block_input(sd32, cfg, audio, steps)
        out = oss.diffwave_block(sd32, BLOCK, x, e) + x
    return out.double() - 2.0 * x64


def row_errors(got, ref):
    """max_l |got - ref| / max_l |ref| per (b, h) row."""
    return (got.double() - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-300)


def far_tap_kernels(k0, k1, frac=0.01):
    """How many of the 2H (direction, channel) kernels still hold `frac` of their largest tap at their last tap."""
    k = torch.cat([k0, k1], 0)
    return int((k[:, -1].abs() >= frac * k.abs().amax(-1)).sum())


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


# ------------------------------------------------------------------------------------------------- the adjoint
# Reference of the convolution ADJOINT (tests/test_s4_convolution_adjoint_gpu.py, ..._adjoint_reference.py): with both ReLUs
# held open everything around the convolution is pointwise in time and smooth, so for a cotangent `cot` of eps
#   da = d loss / d a (a = conv(u, k) + D u) has exactly cot's support,    du = conv^T(da) + D da,
#   audio.grad = init_conv^T (2 dx1 + LN1^T du),     dk0[j] = sum u[i-j] da[i],     dk1[m-1] = sum u[i+m] da[i].
RELU_BIASES = ("init_conv.0.conv.bias", "final_conv.0.conv.bias")
OUT_W = BLOCK + ".layer.output_linear.0.weight"
KERNEL = BLOCK + ".layer.kernel.kernel."
# per-tensor bounds of the GPU test; `kernel.log_dt` goes through gradcheck.compare (the project's cancelling-sum rule)
READOUT_KEYS = (BLOCK + ".layer.D", BLOCK + ".fc_t.weight", BLOCK + ".fc_t.bias")
SPECTRUM_KEYS = tuple(KERNEL + n for n in ("C", "B", "P", "inv_w_real", "w_imag")) + (BLOCK + ".norm1.m", BLOCK + ".norm1.s")
LOG_DT = KERNEL + "log_dt"
AUDIO_BOUND = READOUT_BOUND = 2e-5
SPECTRUM_BOUND = 1e-4
COTANGENTS = ("dense", "head", "tail")


def final_stage(sd, out, pre_activation=False):
    """The oracle's final stage on the block's output: LN -> final_conv.0 (-> ReLU -> final_conv.2)."""
    pre = own.wn_conv1d(sd, "final_conv.0.conv", oss.transposed_ln(out, sd["norm.m"], sd["norm.s"]))
    if pre_activation:
        return pre
    return F.conv1d(F.relu(pre), sd["final_conv.2.conv.weight"], sd["final_conv.2.conv.bias"])


def relu_minima(sd, cfg, audio, steps, taps=None):
    """The smallest float64 pre-activation of the init conv's ReLU and of the final conv's (taps: the block's float64
    (k0, k1) where the caller has them; they do not depend on the biases `open_relus` moves)."""
    sd64 = to_float64(sd)
    if taps is None:
        taps = taps_from_engine(oracle_taps(sd, int(sd[KERNEL + "L"])), audio.shape[-1])
    with torch.no_grad():
        pre0 = own.wn_conv1d(sd64, "init_conv.0.conv", audio.double())
        n = block_forward(sd64, cfg, audio.double(), steps, *taps)
        pre1 = final_stage(sd64, 2.0 * n["x"] + n["s"], pre_activation=True)
    return float(pre0.min()), float(pre1.min())


def open_relus(sd, cfg, audio, steps, margin=0.25):
    """Adds one constant to every entry of `init_conv.0.conv.bias` and one to `final_conv.0.conv.bias` (in place: pass the
    module's own state_dict) so that every float64 pre-activation of both ReLUs is >= margin on these inputs; returns the two
    minima after the shift.  A common shift of the init conv leaves LN1(x) unchanged (it removes the channel mean); x itself
    is no longer clipped, so u differs from the forward test's and the weight conditions are asserted again by the callers."""
    taps = taps_from_engine(oracle_taps(sd, int(sd[KERNEL + "L"])), audio.shape[-1])
    with torch.no_grad():
        for i, key in enumerate(RELU_BIASES):        # the init conv first: the final conv sees the shifted x
            lo = relu_minima(sd, cfg, audio, steps, taps)[i]
            if lo < margin + 0.05:
                sd[key].add_(math.ceil((margin + 0.05 - lo) * 16.0) / 16.0)      # (exact in fp32, with room for its rounding)
    lo = relu_minima(sd, cfg, audio, steps, taps)
    assert min(lo) >= margin, lo
    return lo


def edge_cotangents(B, L, seed):
    """{"dense": N(0, 1), "head": N(0, 1) on the first w = max(2, L // 16) positions and exact zeros elsewhere, "tail": the
    same on the last w}, each [B, 1, L].  (A 2-sample window at L = 16384 leaves an off-support gradient 2e-4 of the
    on-support one: below what an fp32 FFT product resolves relative to it.)"""
    g = torch.Generator().manual_seed(seed)
    w = support_width(L)
    dense, head, tail = torch.randn(B, 1, L, generator=g), torch.zeros(B, 1, L), torch.zeros(B, 1, L)
    head[..., :w] = torch.randn(B, 1, w, generator=g)
    tail[..., L - w:] = torch.randn(B, 1, w, generator=g)
    return {"dense": dense, "head": head, "tail": tail}


def support_width(L):
    return max(2, L // 16)


def off_support(name, L):
    """The positions outside the cotangent's support as a slice (None for the dense one)."""
    w = support_width(L)
    return {"dense": None, "head": slice(w, L), "tail": slice(0, L - w)}[name]


def oracle_conv(u, k0, k1):
    """conv(u, k) in u's precision, as `oracle.sashimi.s4_forward` evaluates it (one FFT of n = Lt + L)."""
    L, Lt = u.shape[-1], k0.shape[-1]
    kk = F.pad(k0, (0, L)) + F.pad(k1.flip(-1), (L, 0))
    return torch.fft.irfft(torch.fft.rfft(u, n=Lt + L) * torch.fft.rfft(kk, n=Lt + L), n=Lt + L)[..., :L]


def block_forward(sd, cfg, audio, steps, k0, k1, conv=None, branch=True, D=None):
    """The isolated block with the taps given, from the oracle's pieces in sd's precision, every node kept in the graph:
    dict(x, e, u, a, s, eps) with a = conv(u, k) + D u, s = GELU(a), eps = final stage(2 x + s).  (The transparent tail is
    taken as exact: the oracle's own carries the GLU gate sigmoid(30) = 1 - 9.4e-14 and an FF branch of exact zeros.)
    branch=False: eps of the direct path 2 x alone.  D: another D than sd's, [1, H] or per sample [B, H]."""
    if conv is None:
        conv = two_sided_conv_fft if audio.dtype == torch.float64 else oracle_conv
    x, e, u = block_input(sd, cfg, audio, steps)
    if not branch:
        return dict(x=x, e=e, u=u, eps=final_stage(sd, 2.0 * x))
    D = sd[BLOCK + ".layer.D"] if D is None else D
    a = conv(u, k0, k1) + D.unsqueeze(-1) * u
    s = gelu_erf(a) if a.dtype == torch.float64 else F.gelu(a)
    return dict(x=x, e=e, u=u, a=a, s=s, eps=final_stage(sd, 2.0 * x + s))


def _leaves(sd, dtype):
    return {k: (v.detach().cpu().clone().to(dtype).requires_grad_(True) if v.is_floating_point() else v.detach().cpu().clone())
            for k, v in sd.items()}


def adjoint_reference(sd, cfg, audio, steps, cot, dtype=torch.float64, k_tap=None, branch=True, taps=None, conv=None):
    """(audio.grad, {parameter: gradient}) of the loss (eps * cot).sum() by torch autograd on the `dtype` copy of sd, both
    returned in float64.  cot: one cotangent [B, 1, L], or a dict of them -- then one forward serves them all and a dict of
    such pairs comes back.  Without taps the graph is `oracle.sashimi.sashimi_forward`, kernel generator included.  With
    `k_tap` (the engine's `k:` tap, or the oracle's taps in its layout) or `taps` = (k0, k1) the taps are constants and the
    block goes through `block_forward`: the kernel parameters then get no gradient and are left out (for the shapes at
    which autograd through the generator is too large, and for deliberately wrong taps or a wrong `conv`).  branch=False: the
    direct path."""
    leaf = _leaves(sd, dtype)
    a = audio.detach().to(dtype).requires_grad_(True)
    if k_tap is None and taps is None and branch:
        eps = oss.sashimi_forward(leaf, cfg, a, steps)
    else:
        if taps is None and branch:
            taps = taps_from_engine(k_tap, audio.shape[-1])
        k0, k1 = (t.to(dtype) for t in taps) if branch else (None, None)     # (the direct path needs no taps)
        eps = block_forward(leaf, cfg, a, steps, k0, k1, conv=conv, branch=branch)["eps"]
        for n in ("C", "B", "P", "inv_w_real", "w_imag", "log_dt"):
            leaf.pop(KERNEL + n)
    params = {k: v for k, v in leaf.items() if v.is_floating_point()}
    cots = cot if isinstance(cot, dict) else {"": cot}
    out = {}
    for i, (name, c) in enumerate(cots.items()):
        gs = torch.autograd.grad((eps * c.to(dtype)).sum(), [a] + list(params.values()), retain_graph=i + 1 < len(cots),
                                 allow_unused=True)
        out[name] = (gs[0].double(), {k: (torch.zeros_like(v) if g is None else g).detach().double()
                                      for (k, v), g in zip(params.items(), gs[1:])})
    return out if isinstance(cot, dict) else out[""]


def branch_part(sd, cfg, audio, steps, cot, ref):
    """ref - ref_direct per cotangent (`ref`: adjoint_reference's audio gradient, or the dict of its pairs): the part of the
    audio gradient that passed the S4 branch.  The direct part is the same gradient with `output_linear.0.weight` zeroed --
    GLU(.) = 0 then, the branch is off and 2 x is all the final stage sees."""
    sd0 = {k: v.detach().cpu().clone() for k, v in sd.items()}
    sd0[OUT_W].zero_()
    direct = adjoint_reference(sd0, cfg, audio, steps, cot, branch=False)
    if isinstance(cot, dict):
        return {n: ref[n][0] - direct[n][0] for n in cot}
    return ref - direct[0]


def audio_errors(got, ref, ref_branch, off=None):
    """The two audio measures, each the worst batch row as (error, row, position): max_l |got - ref| / max_l |ref_branch| over
    all positions, and (off: the slice outside the cotangent's support) max |got - ref| / max |ref| over those positions."""
    d = (got.double() - ref).abs()[:, 0]

    def worst(d, scale):
        e = d.amax(-1) / scale.clamp_min(1e-300)
        b = int(e.argmax())
        return float(e[b]), b, int(d[b].argmax())

    every = worst(d, ref_branch.abs()[:, 0].amax(-1))
    if off is None:
        return every, None
    e, b, pos = worst(d[:, off], ref.abs()[:, 0, off].amax(-1))
    return every, (e, b, pos + (off.start or 0))


def tensor_error(got, ref):
    """max |got - ref| / max |ref| of one parameter gradient."""
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def oracle_taps(sd, Lcfg, dtype=torch.float64, rows=16):
    """The oracle's taps in the layout of the engine's `k:` tap (Lk * k, [2, H, Lk]), generated `rows` channels at a time
    (the Cauchy intermediates of 64 channels at 16384 nodes are gigabytes in float64)."""
    src = {k: v.detach().cpu().to(dtype) for k, v in sd.items() if k.startswith(KERNEL) and v.is_floating_point()}
    H, out = src[KERNEL + "log_dt"].shape[0], []
    with torch.no_grad():
        for h in range(0, H, rows):
            part = {k: (v[h:h + rows] if k.endswith(("log_dt", "inv_w_real", "w_imag")) else v[:, h:h + rows]) for k, v in src.items()}
            part[KERNEL + "L"] = torch.tensor(Lcfg)
            out.append(oss.ss_kernel_nplr(part, KERNEL[:-1], Lcfg))
    return torch.cat(out, 1) * Lcfg


# The cases of the adjoint tests, (H, B, L) by group (Lcfg = L: training needs the kernels' own length).
ADJOINT_PLAN_EDGES = [16, 18, 250, 1022, 1024, 1026, 2046, 2048, 2050, 4094, 4096, 4098, 8190, 8192, 8194, 16382, 16384]
ADJOINT_CASES = {
    "plan_edges": [(8, 2, L) for L in ADJOINT_PLAN_EDGES],                       # the forward test's PLAN_EDGES
    "batch_chunks": [(64, 9, 1024), (64, 17, 1024), (64, 9, 2048), (64, 9, 8192), (64, 9, 16384)],
    "rocfft": [(8, 2, 14), (8, 2, 125), (8, 3, 125), (8, 2, 1025), (8, 1, 16386)],
    "row_counts": [(6, 3, 1024), (6, 3, 8192)],
}
# Taps as constants (adjoint_reference's k_tap mode; audio.grad, D, fc_t.*, norm1.* only): float64 autograd through the
# generator holds 1.6 GB per Cauchy intermediate at H = 64, L = 16384, and at (64, 9, 8192) a case's host passes take 14 s
# (float64 9.5 s, the fp32 oracle 4.6 s; 4 s with constant taps).
K_TAP_CASES = {(64, 9, 8192), (64, 9, 16384)}
COTANGENT_SEED = 91
# Weight seeds other than WEIGHT_SEED: the first seed from 5 on at which the case meets every condition of
# test_case_conditions_hold_on_the_reference with 20 % room (fp32 oracle <= 0.8 x a quarter of each bound, off-support
# gradient >= 1.25e-2 of the on-support one, branch share >= 0.125) -- conditions on the float64 reference and the fp32 CPU
# oracle alone.  What fails at the seeds passed over: norm1.m / norm1.s (scalar sums over all channels and positions that
# cancel; where a seed leaves one small the fp32 oracle is 3e-5 .. 8e-4 from float64 on it), the audio gradient of the fp32
# oracle just above 4e-6, and at L >= 8192 the off-support share (5e-3 .. 1e-2 at most seeds of (8, 2, 16382), (6, 3, 8192)).
ADJOINT_SEEDS = {(8, 2, 250): 6, (8, 2, 2046): 6, (8, 2, 2048): 8, (8, 2, 2050): 9, (8, 2, 4094): 6, (8, 2, 4098): 8,
                 (8, 2, 8190): 6, (8, 2, 16382): 18, (8, 2, 125): 6, (8, 2, 1025): 6, (6, 3, 1024): 6, (6, 3, 8192): 33,
                 (64, 9, 1024): 6, (64, 17, 1024): 6, (64, 9, 2048): 7, (64, 9, 8192): 7, (64, 9, 16384): 7}


def prepare_adjoint_case(H, B, L):
    """(cfg, net on the host with both ReLUs opened, audio, steps, cotangents, the two ReLU minima) of one case."""
    cfg, net = build_isolated_block(H, L, ADJOINT_SEEDS.get((H, B, L), WEIGHT_SEED))
    audio, steps = cases.wavenet_inputs(B, L, 1, INPUT_SEED)
    minima = open_relus(net.state_dict(), cfg, audio, steps)
    net.invalidate()
    return cfg, net, audio, steps, edge_cotangents(B, L, COTANGENT_SEED), minima


def host_references(sd, cfg, audio, steps, cots, k_tap=None):
    """dict(ref, branch, oracle32) per cotangent: the float64 reference (audio.grad, gradients), its branch part, and the
    fp32 CPU oracle through the same graph."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    ref = adjoint_reference(sd, cfg, audio, steps, cots, k_tap=k_tap)
    return dict(ref=ref, branch=branch_part(sd, cfg, audio, steps, cots, ref),
                oracle32=adjoint_reference(sd, cfg, audio, steps, cots, dtype=torch.float32, k_tap=k_tap))


def on_support_max(da, name):
    """max |da| per batch row over the cotangent's support."""
    L = da.shape[-1]
    w = support_width(L)
    return da.abs()[:, 0, :w if name == "head" else L - w:].amax(-1) if name != "dense" else da.abs()[:, 0].amax(-1)


def fftcorr_chunks(B, H):
    """(bchunk, size of the last chunk) of the batch loop of `fftcorr` as `kernel_backward` (sashimi_model.hip) sets it up:
    nbs = min(B, ceil(512 / H)) partial spectra, bchunk = ceil(B / nbs) samples per workgroup."""
    nbs = max(1, min(B, -(-512 // H)))
    bchunk = -(-B // nbs)
    nchunks = -(-B // bchunk)
    return bchunk, B - (nchunks - 1) * bchunk

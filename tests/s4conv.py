"""Shared pieces of the S4 long-convolution tests (tests/test_s4_convolution_gpu.py, tests/test_s4_convolution_reference.py):
a one-block network whose tail is transparent to the S4 branch, and the float64 host evaluation of that branch

    GELU(conv(u, k) + D u),   conv(u, k)[i] = sum_{j<=i} k0[j] u[i-j] + sum_{m>=1} k1[m-1] u[i+m]      (`s4.py:1391-1437`)

with u = LN1(x) + fc_t(e), x = relu(init_conv(audio)).  The taps k come from the caller (the engine's own `k:` tap in the
GPU tests), so the comparison judges the convolution, not the kernel generator."""
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

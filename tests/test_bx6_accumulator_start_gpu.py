"""GPU: the accumulator start values of the bf16x6 WaveNet layer kernel on 16x16x32 at C = S = 256 (`csrc/wavenet_bx6.hip`).

On that shape the step-embedding row, the conv bias and the [res; skip] biases no longer pass through the matrix cores as a
correction k-block: every accumulator register STARTS at its rank-1 fp32 value (one rounding), fetched in accumulator layout --
four consecutive rows per 16-byte load from the layer's correction row (per clip, or per (step, clip) in a labelled step table)
and from the bias vectors.  A wrong row, a wrong column's in-range indicator or a row of another clip shows where the start
value carries the result, so:

  start value dominates   one layer isolated as tests/wnlayer.py describes (net A: the last layer, net B: a middle one) with
                          `fc_t.weight`, `fc_t.bias` and the dilated conv's bias of that layer scaled by one power of two so that
                          rms fc_t(e) is about 30 x rms x.  Shapes (d, L): (1, 63) rows not 16-byte aligned, (16, 333) the
                          contiguous staging form, (64, 600) block-fastest tiles with both halos, (2048, 600) d > L, where the
                          indicator and the centre tap act alone.  Per position class of `wnlayer.CLASSES`: the 16x16x32 error
                          against float64 <= 2 x the f32 Winograd path's (`wnlayer.BX6_OVER_F32`), and < 1e-5
                          (`wnlayer.FORWARD_BOUND`) against the f32 Winograd path's output.
  weight seeds            as `wnlayer.SEEDS`: the first seed from 5 on at which the fp32 CPU oracle ALONE meets the forward
                          condition of tests/test_wavenet_layer_reference.py on the scaled weights (one thread, every class <=
                          1e-5 / 8, x 0.8 for a seed other than 5).  Evaluated on the CPU: seed 5 meets it in all four cases --
                          (1, 63) 8.5e-7, (16, 333) 1.02e-6, (64, 600) 9.6e-7, (2048, 600) 8.9e-7 of 1.25e-6 (worst class on one
                          host: the figure moves with the host's fp32 kernels; the factors are 512, 128, 64, 32 and the ratios
                          reached 37.5, 35.2, 30.6, 36.5) -- and every GPU case asserts the condition again before it judges
                          the kernel.
  per-clip rows           a class-conditional network of 3 layers, B = 3 distinct labels, L = 2052, through the step-table sampler
                          for T = 4 (rows per (step, clip): the table's batch and step strides): captured and eager runs give
                          equal bits, each clip alone equals the clip inside the batch bit for bit, and the result is within
                          1e-5 of precision = f32.

Every case prints its figures before anything is asserted.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import wavenet as own
from tests import cases
from tests import label_reference as lr
from tests import wnlayer as wl
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

C = S = 256
RATIO = 30.0                                   # rms fc_t(e) / rms x of the isolated layer
SHAPES = ((1, 63), (16, 333), (64, 600), (2048, 600))
SEEDS = {}                                     # (d, L) -> weight seed other than wnlayer.WEIGHT_SEED (none needed: see above)
SCALED_KEYS = ("fc_t.weight", "fc_t.bias", "dilated_conv_layer.conv.bias")
F32W = {"precision": "f32", "conv_algo": "winograd", "bx6_mfma": "32x32x16"}
NEW = {"precision": "bf16x6", "conv_algo": "winograd", "bx6_mfma": "16x16x32"}


def scaled_nets(d, L, seed):
    """`wnlayer.build_nets` with layer k's fc_t and dilated-conv bias times 2^n, n the integer nearest to
    log2(RATIO rms x_k / rms fc_t(e)) on the fp32 CPU oracle's x_k and e (a power of two: the scaling itself rounds nothing).
    Returns (nets, the factor, the ratio reached)."""
    k = d.bit_length() - 1
    nets = wl.build_nets(C, S, d, seed)
    audio, steps = wl.inputs(wl._batch(d, L), L)
    cfg, net = nets["B"]
    sd = net.state_dict()
    x_k, e = wl.oracle_input(sd, cfg, audio, steps, k)
    p = wl.block(k) + "."
    rms = lambda t: float(t.double().pow(2).mean().sqrt())
    with torch.no_grad():
        part = F.linear(e, sd[p + "fc_t.weight"].cpu(), sd[p + "fc_t.bias"].cpu())
        factor = 2.0 ** round(math.log2(RATIO * rms(x_k) / rms(part)))
        for _, n in nets.values():
            for key in SCALED_KEYS:
                n.state_dict()[p + key].mul_(factor)
            n.invalidate()
    return nets, factor, factor * rms(part) / rms(x_k)


def oracle_forward_figures(nets, d, L):
    """{class: error} of the fp32 CPU oracle's layer against float64 on the same fp32 (x_k, e), worst of x_out / skip, on one
    thread: the forward part of `wnlayer.oracle_figures`, on the nets handed in."""
    k = d.bit_length() - 1
    audio, steps = wl.inputs(wl._batch(d, L), L)
    cfg, net = nets["B"]
    sd = {key: v.detach().cpu() for key, v in net.state_dict().items()}
    x_k, e = wl.oracle_input(sd, cfg, audio, steps, k)
    ref = wl.forward_reference(wl.to_float64(sd), k, x_k, e)
    with wl.one_thread(), torch.no_grad():
        x32, s32 = own.residual_block(sd, wl.block(k), x_k, e, d)
    out = {}
    for got, want in ((x32, ref["x_out"]), (s32, ref["skip"])):
        for c, v in wl.class_errors(got, want, d).items():
            if v is not None:
                out[c] = max(out.get(c, 0.0), v)
    return out


def oracle_condition(fig, seed):
    room = 0.8 if seed != wl.WEIGHT_SEED else 1.0
    return all(v <= room * wl.FORWARD_BOUND / 8 for v in fig.values())


def first_seed(d, L, limit=40):
    """The first seed from `wnlayer.WEIGHT_SEED` on that meets `oracle_condition` on the scaled weights (CPU only)."""
    for seed in range(wl.WEIGHT_SEED, wl.WEIGHT_SEED + limit):
        fig = oracle_forward_figures(scaled_nets(d, L, seed)[0], d, L)
        if oracle_condition(fig, seed):
            return seed, fig
    raise AssertionError((d, L))


def _forward(net, opts, audio, steps):
    B, _, L = audio.shape
    for key, value in opts.items():
        net.set_option(key, value)
    with torch.no_grad():
        eps = net((audio, steps))
    return dict(eps=eps, x=net.read_tap("x", (B, C, L)), skip=net.read_tap("skip", (B, S, L)),
                e=net.read_tap("emb_mlp", (B, net.embed_dims[2])), ran=net.read_tap("split_launches", (2,)).cpu().tolist())


@pytest.mark.parametrize("d,L", SHAPES, ids=[f"d{d}_L{L}" for d, L in SHAPES])
def test_start_value_dominates(gpu, d, L):
    k, B = d.bit_length() - 1, wl._batch(d, L)
    seed = SEEDS.get((d, L), wl.WEIGHT_SEED)
    nets, factor, ratio = scaled_nets(d, L, seed)
    fig = oracle_forward_figures(nets, d, L)
    fmt = lambda ce: " ".join(f"{c} {'-' if v is None else format(v, '.2e')}" for c, v in ce.items())
    print(f"BX6START d={d} L={L} seed {seed}: fc_t x {factor:g}, rms fc_t(e) / rms x = {ratio:.1f}; fp32 CPU oracle {fmt(fig)}")
    assert 20.0 <= ratio <= 45.0, ratio                      # a power of two lands within sqrt(2) of RATIO
    assert oracle_condition(fig, seed), fig
    sd64 = wl.to_float64({key: v.detach().cpu() for key, v in nets["B"][1].state_dict().items()})
    audio, steps = wl.inputs(B, L)
    audio, steps = audio.to(gpu), steps.to(gpu)
    nets = {w: (cfg, net.to(gpu)) for w, (cfg, net) in nets.items()}
    for _, net in nets.values():
        net.invalidate()
    runs, errors, failures = {}, {}, []
    for name, opts in (("f32", F32W), ("new", NEW)):
        r = runs[name] = {w: _forward(net, opts, audio, steps) for w, (_, net) in nets.items()}
        for w, (cfg, _) in nets.items():
            NL = cfg["num_res_layers"]
            if r[w]["ran"] != ([NL, 0] if name == "new" else [0, NL]):
                failures.append(f"{name} net {w}: split_launches {r[w]['ran']}")
        ref = wl.forward_reference(sd64, k, r["A"]["x"].cpu(), r["A"]["e"].cpu())
        errors[name] = {"B.x": wl.class_errors(r["B"]["x"].cpu(), ref["x_out"], d),
                        "B.skip": wl.class_errors(r["B"]["skip"].cpu(), ref["skip"], d),
                        "A.skip": wl.class_errors(r["A"]["skip"].cpu(), ref["skip"], d)}
    between = {"B.x": wl.class_errors(runs["new"]["B"]["x"].cpu(), runs["f32"]["B"]["x"].cpu(), d),
               "B.skip": wl.class_errors(runs["new"]["B"]["skip"].cpu(), runs["f32"]["B"]["skip"].cpu(), d),
               "A.skip": wl.class_errors(runs["new"]["A"]["skip"].cpu(), runs["f32"]["A"]["skip"].cpu(), d)}
    for t in between:
        print(f"BX6START d={d} L={L} {t}: f32/winograd vs float64 {fmt(errors['f32'][t])} | 16x16x32 vs float64 "
              f"{fmt(errors['new'][t])} | 16x16x32 vs f32/winograd {fmt(between[t])}")
    for t in between:
        assert any(v is not None for v in between[t].values())
        for cls in wl.CLASSES:
            e_new, e_f32, e_btw = errors["new"][t][cls], errors["f32"][t][cls], between[t][cls]
            if e_new is None:
                continue
            if not e_new <= wl.BX6_OVER_F32 * e_f32:
                failures.append(f"{t} {cls}: {e_new:.2e} > 2 x the f32 Winograd path's {e_f32:.2e}")
            if not e_btw < wl.FORWARD_BOUND:
                failures.append(f"{t} {cls}: {e_btw:.2e} >= {wl.FORWARD_BOUND:g} against the f32 Winograd path")
    assert not failures, "\n".join(failures)


def test_per_clip_rows_of_a_labelled_step_table(gpu):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling
    B, L, T = 3, 2052, 4
    labels = [2, 0, 1]
    cfg = cases.wn_cfg(res_channels=C, skip_channels=S, num_res_layers=3, dilation_cycle=3)
    net = lr.build(cfg, 91).to(gpu)
    dh = calc_diffusion_hyperparams(T, 1e-4, 0.05)
    g = torch.Generator().manual_seed(92)
    x_T, noise = torch.randn(B, 1, L, generator=g), torch.randn(T, B, 1, L, generator=g)
    run = lambda graph: sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise, use_graph=graph, labels=labels)
    for key, value in NEW.items():
        net.set_option(key, value)
    captured, eager = run(True), run(False)
    alone = [sampling(net, (1, 1, L), dh, x_T=x_T[b:b + 1].contiguous(), noise=noise[:, b:b + 1].contiguous(), use_graph=False,
                      labels=[labels[b]]) for b in range(B)]
    other = sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise, use_graph=False, labels=[labels[0]] * B)
    for key, value in F32W.items():
        net.set_option(key, value)
    exact = run(False)
    e = rel_err(eager, exact)
    print(f"BX6START labelled sampler T={T} B={B} L={L}: rel err 16x16x32 vs f32 {e:.3e}; captured == eager "
          f"{torch.equal(captured, eager)}; alone == in batch {[torch.equal(alone[b][0], eager[b]) for b in range(B)]}")
    assert torch.isfinite(eager).all()
    assert torch.equal(captured, eager)
    for b in range(B):
        assert torch.equal(alone[b][0], eager[b]), b
    assert not torch.equal(other[1], eager[1])               # the rows are per clip: another label gives another clip
    assert e < 1e-5, e

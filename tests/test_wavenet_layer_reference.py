"""CPU: the float64 reference of tests/test_wavenet_layer_gpu.py and tests/test_wavenet_layer_adjoint_gpu.py (tests/wnlayer.py)
-- every condition that involves the reference alone, and that the bounds have teeth.

  explicit adjoint      float64 autograd through `wnlayer.layer_forward` against the adjoint of the three-tap convolution
                        written as loops over (clip, position, tap): the data gradient as the transposed convolution, the weight
                        gradient as sum_l dH[o, l] h_pad[c, l + (t - 1) d] with h zero-padded AFTER fc_t(e) was added
  layer_block           the layer written out tap by tap (what the mutations are applied to) is the oracle's `residual_block`,
                        and `_Conv3`'s hand-written backward is autograd's
  case conditions       for EVERY GPU case, nets A and B: both ReLUs open by 0.25; the float64 audio gradient of a head / tail
                        cotangent exactly zero outside `wnlayer.footprint`; every gradient the GPU test judges nonzero; the
                        fp32 CPU oracle through the same graph within a quarter of each adjoint bound, in the GPU test's measure
  forward eighth        the fp32 CPU oracle of the layer within an eighth of the forward bound per position class
  mutations             seven wrong layers / adjoints, each applied to the float64 reference, move the measure they target to
                        at least 10 x its bound
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import wavenet as own
from tests import cases
from tests import wnlayer as wl


def _graph_by_hand(leaf, cfg, audio, steps, k):
    """`layer_forward` once more from the oracle's pieces with the convolution's nodes kept: dict(h, W, H, eps)."""
    d, p = 1 << k, wl.block(k)
    B = audio.shape[0]
    x_k = F.relu(own.wn_conv1d(leaf, "init_conv.0.conv", audio)) * wl.SQH ** k
    e = own.step_embedding_mlp(leaf, "residual_layer.", steps, cfg["diffusion_step_embed_dim_in"])
    h = x_k + F.linear(e, leaf[p + ".fc_t.weight"], leaf[p + ".fc_t.bias"]).reshape(B, -1, 1)
    W = own.weight_norm_weight(leaf, p + ".dilated_conv_layer.conv")
    H = F.conv1d(h, W, leaf[p + ".dilated_conv_layer.conv.bias"], dilation=d, padding=d)
    C = h.shape[1]
    out = torch.tanh(H[:, :C]) * torch.sigmoid(H[:, C:])
    x_out = (x_k + own.wn_conv1d(leaf, p + ".res_conv", out)) * wl.SQH
    skip = own.wn_conv1d(leaf, p + ".skip_conv", out)
    NL = cfg["num_res_layers"]
    if NL == k + 2:
        skip = skip + own.residual_block(leaf, wl.block(k + 1), x_out, e, 1)[1]
    pre = own.wn_conv1d(leaf, "final_conv.0.conv", skip * (1.0 / NL) ** 0.5)
    eps = F.conv1d(F.relu(pre), leaf["final_conv.2.conv.weight"], leaf["final_conv.2.conv.bias"])
    for t in (h, W, H):
        t.retain_grad()
    return dict(h=h, W=W, H=H, eps=eps)


@pytest.mark.parametrize("C,S,d,L,B,which", [(16, 16, 1, 63, 2, "A"), (16, 16, 64, 600, 3, "B"), (16, 16, 256, 200, 2, "B")])
def test_autograd_equals_the_explicit_adjoint_of_the_three_tap_convolution(C, S, d, L, B, which):
    k = d.bit_length() - 1
    cfg, net, audio, steps, cots, minima = wl.prepare_adjoint_case(C, S, d, L, B, which)
    assert min(minima) >= 0.25
    sd = net.state_dict()
    leaf = wl._leaves(sd, torch.float64)
    n = _graph_by_hand(leaf, cfg, audio.double(), steps, k)
    (n["eps"] * cots["dense"].double()).sum().backward()
    h, W, dH = n["h"].detach(), n["W"].detach(), n["H"].grad
    dh, dW = torch.zeros_like(h), torch.zeros_like(W)
    for b in range(B):
        for l in range(L):
            for t in range(3):
                j = l + (t - 1) * d                        # the padded h is zero outside [0, L): fc_t(e) included
                if 0 <= j < L:
                    dW[:, :, t] += torch.outer(dH[b, :, l], h[b, :, j])
                    dh[b, :, j] += W[:, :, t].t() @ dH[b, :, l]
    rel = lambda g, w: float((g - w).abs().max()) / max(1.0, float(w.abs().max()))
    errs = {"dh": rel(n["h"].grad, dh), "dW": rel(n["W"].grad, dW)}
    assert float(dH.abs().max()) > 1e-6 and (d >= L or float(dW[:, :, 0].abs().max()) > 0)
    if d >= L:
        assert not bool(dW[:, :, 0].any()) and not bool(dW[:, :, 2].any())       # no position owns an outer tap
    # the same gradients through layer_forward, on the oracle's residual_block and on the written-out layer_block / _Conv3
    p = wl.block(k) + "."
    by_hand = {key: leaf[p + key].grad for key in wl.LAYER_KEYS}
    for explicit in (False, True):
        ref = wl.adjoint_reference(sd, cfg, audio, steps, k, {"dense": cots["dense"]}, explicit=explicit)["dense"]
        for key in wl.LAYER_KEYS:
            want = by_hand[key] if by_hand[key] is not None else torch.zeros_like(ref[1][key])
            errs[f"{key} explicit={explicit}"] = rel(ref[1][key], want)
    print(f"{which} C={C} d={d} L={L}: autograd vs the explicit adjoint: " + ", ".join(f"{k_} {e:.1e}" for k_, e in errs.items()))
    assert all(e < 1e-12 for e in errs.values()), errs


@pytest.mark.parametrize("C,S,d,L,B", [(16, 16, 4, 50, 2), (64, 64, 64, 600, 3), (64, 64, 2048, 600, 2)])
def test_the_written_out_layer_is_the_oracles_residual_block(C, S, d, L, B):
    k = d.bit_length() - 1
    cfg, net = wl.build_nets(C, S, d, wl.WEIGHT_SEED)["B"]
    sd64 = wl.to_float64(net.state_dict())
    audio, steps = wl.inputs(B, L)
    x_k, e = wl.oracle_input(net.state_dict(), cfg, audio, steps, k)
    with torch.no_grad():
        x_out, skip = own.residual_block(sd64, wl.block(k), x_k.double(), e.double(), d)
        n = wl.layer_block(sd64, wl.block(k), x_k.double(), e.double(), d)
        Href = own.wn_conv1d(sd64, wl.block(k) + ".dilated_conv_layer.conv", n["h"], dilation=d)
    assert wl.tensor_error(n["x_out"], x_out) < 1e-13 and wl.tensor_error(n["skip"], skip) < 1e-13
    assert wl.tensor_error(n["H"], Href) < 1e-13
    assert float(skip.abs().max()) > 1e-3 and float(x_out.abs().max()) > 1e-3


def test_cotangents_classes_and_footprints_are_what_they_claim():
    for d, L in wl.SHAPES:
        w = wl.support_width(d, L)
        assert w == max(2, min(d, L // 16))
        c = wl.edge_cotangents(2, d, L)
        assert bool((c["head"][..., :w] != 0).all()) and not bool(c["head"][..., w:].any())
        assert bool((c["tail"][..., L - w:] != 0).all()) and not bool(c["tail"][..., :L - w].any())
        cl = wl.position_classes(d, L)
        assert bool((cl["head"] | cl["tail"] | cl["seam"] | cl["interior"]).all())
        assert int(cl["head"].sum()) == min(d, L) == int(cl["tail"].sum())
        assert bool(cl["seam"][0]) and (L <= 64 or bool(cl["seam"][63] & cl["seam"][64] & cl["seam"][65]))
        fa, fb = wl.footprint("head", "A", d, L), wl.footprint("head", "B", d, L)
        assert int(fa.sum()) == w + (w if d + w <= L else max(0, L - d)) - max(0, w - d) and bool((fb | ~fa).all())
        assert torch.equal(wl.footprint("tail", "A", d, L), fa.flip(0)) and torch.equal(wl.footprint("tail", "B", d, L), fb.flip(0))
    assert wl.position_classes(1, 63)["interior"].sum() == 0                    # d = 1: every position is a seam
    assert [wl.case_id(c) for c in wl.CASES].count("C256_S256_d64_L600_B3") == 1 and len(wl.CASES) == 24
    assert all(B == (3 if (d, L) == (64, 600) else 2) for _, _, d, L, B in wl.CASES)


def _figures(case):
    C, S, d, L, B = case
    return cases.cached(("wnlayer_oracle_figures", case), lambda: wl.oracle_figures(C, S, d, L, B, wl.seed_of(C, S, d, L)))


@pytest.mark.parametrize("case", wl.CASES, ids=wl.case_id)
def test_case_conditions_hold_on_the_reference(case):
    """Both ReLUs open by 0.25; the fp32 CPU oracle through the same graph within a quarter of every adjoint bound (nets A and B,
    the three cotangents); the float64 audio gradient of a head / tail cotangent exactly zero outside `wnlayer.footprint` and
    nonzero everywhere inside; every gradient the GPU test judges nonzero.  Weight seeds: `wnlayer.SEEDS` (empty: every case
    meets the adjoint condition at seed 5 once the cotangents pass `wnlayer.cotangent_sum_is_typical`)."""
    C, S, d, L, B = case
    k, seed = d.bit_length() - 1, wl.seed_of(C, S, d, L)
    fig = _figures(case)
    assert all(min(m) >= 0.25 for m in fig["minima"].values()), fig["minima"]
    print(f"WNLAYER-REF {wl.case_id(case)} seed {seed}, cotangent seed {wl.cotangent_seed(B, d, L)}: ReLU minima "
          + " ".join(f"{w} {m[0]:.3f} {m[1]:.3f}" for w, m in fig["minima"].items())
          + " | fp32 oracle adjoint " + " ".join(f"{key} {v:.2e}" for key, v in fig["adjoint"].items()))
    room = 0.8 if seed != wl.WEIGHT_SEED else 1.0
    late = {key: v for key, v in fig["adjoint"].items() if not v <= room * wl.bound_of(key) / 4}
    assert not late, late
    for which in ("A", "B"):
        cfg, net, audio, steps, cots, minima = wl.prepare_adjoint_case(C, S, d, L, B, which)
        assert all(wl.cotangent_sum_is_typical(c) for c in cots.values())
        ref = wl.adjoint_reference(net.state_dict(), cfg, audio, steps, k, cots)
        for name in wl.COTANGENTS:
            da, grads = ref[name]
            assert float(da.abs().max()) > 0
            fp = wl.footprint(name, which, d, L)
            if fp is not None:
                assert not bool(da[..., ~fp].any()), (which, name)              # exactly zero
                assert bool(fp.any()) and not bool(fp.all())
                assert bool((da[..., fp] != 0).all()), (which, name)            # and the footprint is no wider than it must be
            for key in wl.LAYER_KEYS:
                last_res = which == "A" and key.startswith("res_conv")           # the last layer's residual output is not used
                assert bool(grads[key].any()) != last_res, (which, name, key)


@pytest.mark.parametrize("case", wl.CASES, ids=wl.case_id)
def test_fp32_oracle_keeps_an_eighth_of_the_forward_bound(case):
    """`oracle.wavenet.residual_block` in fp32 against float64 on the same fp32 (x_k, e), worst of x_out / skip per position
    class: <= 1e-5 / 8 = 1.25e-6.  The fp32 side runs on one intra-op thread (`wnlayer.one_thread`): on more threads torch's
    one-tap convolution starts its accumulators from the bias, and at (256, 256), d = 2048, where the skip output is mostly
    bias, that summation order alone leaves 1.65e-6 (L = 600) and 1.48e-6 (L = 2052) at every weight seed from 5 to 44, against
    3.9e-7 and 3.0e-7 for the same weights on one thread.  Over the 24 cases: 1.2e-7 .. 7.7e-7 on one thread, 2.5e-7 .. 1.65e-6 on
    eight (printed beside it, not asserted: it is a property of the host's thread count)."""
    fig = _figures(case)
    print(f"WNLAYER-REF {wl.case_id(case)}: fp32 oracle forward " + " ".join(f"{c} {v:.2e}" for c, v in fig["forward"].items())
          + f" | on the pool's {torch.get_num_threads()} threads " + " ".join(f"{c} {v:.2e}" for c, v in fig["forward_pool"].items()))
    room = 0.8 if wl.seed_of(*case[:4]) != wl.WEIGHT_SEED else 1.0
    assert all(v <= room * wl.FORWARD_BOUND / 8 for v in fig["forward"].values()), fig["forward"]


# ----------------------------------------------------------------------------------------------------- mutations
D_LT_L, D_GT_L, FOUR_OWNERS = (64, 64, 64, 600, 3), (64, 64, 2048, 600, 2), (64, 64, 2048, 2052, 2)
# wrong layers that cannot differ where no position owns an outer tap (d > L): every term they touch has a zero factor
NEED_AN_OUTER_TAP = (wl.MUTATIONS[1], wl.MUTATIONS[2], wl.MUTATIONS[6])


def _forward_moved(case, wrong):
    """Worst class error of (x_out, skip) between the wrong float64 layer and the right one, in the GPU test's measure."""
    C, S, d, L, B = case
    k = d.bit_length() - 1
    cfg, net = wl.build_nets(C, S, d, wl.seed_of(C, S, d, L))["B"]
    audio, steps = wl.inputs(B, L)
    x_k, e = wl.oracle_input(net.state_dict(), cfg, audio, steps, k)
    sd64 = wl.to_float64(net.state_dict())
    ref = wl.forward_reference(sd64, k, x_k, e)
    with torch.no_grad():
        bad = wl.layer_block(sd64, wl.block(k), x_k.double(), e.double(), d, wrong)
    errs = {f"{t} {c}": v for t in ("x_out", "skip") for c, v in wl.class_errors(bad[t], ref[t], d).items() if v is not None}
    return max(errs.items(), key=lambda kv: kv[1])


def _adjoint_moved(case, wrong, key):
    """Worst `tensor_error` of `key` between the wrong float64 adjoint and the right one over nets and cotangents."""
    C, S, d, L, B = case
    k, worst = d.bit_length() - 1, ("", 0.0)
    for which in ("A", "B"):
        cfg, net, audio, steps, cots, _ = wl.prepare_adjoint_case(C, S, d, L, B, which)
        sd = net.state_dict()
        ref = wl.adjoint_reference(sd, cfg, audio, steps, k, cots)
        bad = wl.adjoint_reference(sd, cfg, audio, steps, k, cots, wrong=wrong)
        for name in wl.COTANGENTS:
            e = wl.adjoint_errors(bad[name], ref[name])[key]
            if e > worst[1]:
                worst = (f"{which} {name}", e)
    return worst


@pytest.mark.parametrize("case", [D_LT_L, D_GT_L, FOUR_OWNERS], ids=wl.case_id)
@pytest.mark.parametrize("wrong", wl.MUTATIONS)
def test_the_measures_catch_a_wrong_layer(wrong, case):
    """Each mutation must move the measure it targets to >= 10 x its bound: the forward ones a class error of x_out or skip
    (bound 1e-5), "unmasked h" the dilated conv's weight_v gradient and "+d" the audio gradient (2e-5).  At d > L three of the
    seven are the right layer (no position owns an outer tap, so a dropped, swapped or mirrored outer tap multiplies zeros):
    there they must change NOTHING, and the case at which exactly four positions own one (d = 2048, L = 2052) judges them."""
    d, L = case[2], case[3]
    if wrong in wl.FORWARD_MUTATIONS:
        where, moved = _forward_moved(case, wrong)
        bound = wl.FORWARD_BOUND
    else:
        key = "dilated_conv_layer.conv.weight_v" if wrong == wl.ADJOINT_MUTATIONS[0] else "audio"
        where, moved = _adjoint_moved(case, wrong, key)
        where, bound = f"{key} {where}", wl.bound_of(key)
    print(f"{wl.case_id(case)}: {wrong}: {moved:.2e} ({where}), {moved / bound:.0f} x the bound")
    if d > L and wrong in NEED_AN_OUTER_TAP:
        assert moved == 0.0, (wrong, moved)
    else:
        assert moved >= 10 * bound, (wrong, where, moved)

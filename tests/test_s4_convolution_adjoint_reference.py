"""CPU: the float64 reference of tests/test_s4_convolution_adjoint_gpu.py (the adjoint part of tests/s4conv.py).

  explicit adjoint      autograd's du, dk0, dk1, dD, d fc_t(e) on the isolated block against the adjoint of the definition in
                        `s4conv.two_sided_conv_direct`, written out as double loops: which half is which, independently of
                        the FFT form
  read-out identity     a delta in da at the last / first position reads k0 / k1 back through du
  k_tap mode            the graph with constant taps gives the oracle graph's gradients
  case conditions       for EVERY GPU case, on the reference alone: both ReLUs open by 0.25, far taps and a convolution term
                        that carry weight, a branch share of at least 0.1 of the audio gradient per row, an off-support
                        gradient of at least 1e-2 of the on-support one, and the fp32 CPU oracle within a quarter of every
                        bound the GPU test holds the engine to, in the same measures
  sensitivity           four wrong adjoints (last tap of k0 dropped, k0 and k1 swapped, circular wrap at n = L, a sample of
                        a batch chunk missing from dD) each move a measure of the GPU test above its bound on the head or
                        the tail cotangent: a bound that lets one of them through cannot be committed
"""
import pytest
import torch

from tests import cases, s4conv

H = 8
ALL_CASES = [c for group in s4conv.ADJOINT_CASES.values() for c in group]


def _small_block(Lcfg, L, B=2):
    """The isolated block with open ReLUs in float64, taps as leaves: (cfg, leaves, audio, steps, k0, k1)."""
    cfg, net = s4conv.build_isolated_block(H, Lcfg)
    sd = net.state_dict()
    audio, steps = cases.wavenet_inputs(B, L, 1, s4conv.INPUT_SEED)
    assert min(s4conv.open_relus(sd, cfg, audio, steps)) >= 0.25
    k0, k1 = s4conv.taps_from_engine(s4conv.oracle_taps(sd, Lcfg), L)
    leaf = {k: (v.detach().double().requires_grad_(True) if v.is_floating_point() else v.detach().clone()) for k, v in sd.items()}
    return cfg, leaf, audio.double().requires_grad_(True), steps, k0.requires_grad_(True), k1.requires_grad_(True)


@pytest.mark.parametrize("Lcfg,L", [(16, 16), (18, 18), (64, 64), (250, 250)])
def test_autograd_equals_the_explicit_adjoint_of_the_definition(Lcfg, L):
    """du[i] = sum_j k0[j] da[i+j] + sum_{m>=1} k1[m-1] da[i-m] + D da[i];  dk0[j] = sum_{b,i} u[i-j] da[i];
    dk1[m-1] = sum_{b,i} u[i+m] da[i];  dD[h] = sum u da;  d fc_t(e)[b, h] = sum_l du -- as double loops, against autograd
    through the FFT form, to 1e-12 of each quantity's largest value (1e-12 absolute below 1)."""
    B = 2
    cfg, leaf, audio, steps, k0, k1 = _small_block(Lcfg, L, B)
    n = s4conv.block_forward(leaf, cfg, audio, steps, k0, k1)
    n["u"].retain_grad(), n["a"].retain_grad()
    (n["eps"] * s4conv.edge_cotangents(B, L, s4conv.COTANGENT_SEED)["dense"].double()).sum().backward()
    u, da, D = n["u"].detach(), n["a"].grad, leaf[s4conv.BLOCK + ".layer.D"].detach()[0]
    du, dk0, dk1, dD = torch.zeros_like(u), torch.zeros_like(k0), torch.zeros_like(k1), torch.zeros_like(D)
    for h in range(H):
        c, a, Dh = k0[h].tolist(), k1[h].tolist(), float(D[h])
        g0, g1, gD = [0.0] * L, [0.0] * L, 0.0
        for b in range(B):
            ur, dr = u[b, h].tolist(), da[b, h].tolist()
            for i in range(L):
                acc = Dh * dr[i]
                for j in range(L - i):              # y[i + j] holds k0[j] u[i]
                    acc += c[j] * dr[i + j]
                for m in range(1, i + 1):           # y[i - m] holds k1[m - 1] u[i]
                    acc += a[m - 1] * dr[i - m]
                du[b, h, i] = acc
                gD += ur[i] * dr[i]
            for j in range(L):
                g0[j] += sum(ur[i - j] * dr[i] for i in range(j, L))
            for m in range(1, L):
                g1[m - 1] += sum(ur[i + m] * dr[i] for i in range(L - m))
        dk0[h], dk1[h], dD[h] = torch.tensor(g0, dtype=torch.float64), torch.tensor(g1, dtype=torch.float64), gD
    dpt = du.sum(-1)                                                   # d fc_t(e) [B, H]
    pairs = {"du": (n["u"].grad, du), "dk0": (k0.grad, dk0), "dk1": (k1.grad, dk1),
             "dD": (leaf[s4conv.BLOCK + ".layer.D"].grad[0], dD),
             "d fc_t.bias": (leaf[s4conv.BLOCK + ".fc_t.bias"].grad, dpt.sum(0)),
             "d fc_t.weight": (leaf[s4conv.BLOCK + ".fc_t.weight"].grad, dpt.t() @ n["e"].detach())}
    errs = {k: float((g - w).abs().max()) / max(1.0, float(w.abs().max())) for k, (g, w) in pairs.items()}
    print(f"L={L}: autograd vs explicit adjoint: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert float(da.abs().max()) > 1e-3 and float(dk1[:, L - 2].abs().max()) > 0          # (k1[L - 1] never lands on the row)
    assert all(e < 1e-12 for e in errs.values()), errs


@pytest.mark.parametrize("L", [16, 18, 250])
def test_a_delta_in_da_reads_the_taps_back(L):
    """da = delta at L - 1: du[i] - D da[i] = k0[L - 1 - i] da[L - 1];  delta at 0: k1[i - 1] da[0] for i >= 1."""
    cfg, leaf, audio, steps, k0, k1 = _small_block(L, L)
    n = s4conv.block_forward(leaf, cfg, audio, steps, k0, k1)
    D = leaf[s4conv.BLOCK + ".layer.D"].detach()[0]
    for pos, amp in ((L - 1, 0.7), (0, -1.3)):
        da = torch.zeros_like(n["a"])
        da[..., pos] = amp
        (du,) = torch.autograd.grad(n["a"], n["u"], da, retain_graph=True)
        conv_t = du - D[:, None] * da
        want = torch.zeros_like(conv_t)
        if pos:
            want[:] = amp * k0.detach().flip(-1)
        else:
            want[..., 1:] = amp * k1.detach()[:, :L - 1]
            want[..., 0] = amp * k0.detach()[:, 0]          # (the zero lag belongs to the causal half)
        assert float((conv_t - want).abs().max()) < 1e-13


@pytest.mark.parametrize("Hc,B,L", [(8, 2, 18), (8, 2, 1024), (6, 3, 1024)])
def test_constant_taps_give_the_gradients_of_the_oracle_graph(Hc, B, L):
    """adjoint_reference's k_tap mode (the block from the oracle's pieces, the transparent tail taken as exact) against
    `oracle.sashimi.sashimi_forward` with the generator in the graph, on the oracle's own float64 taps: 1e-10 of each
    tensor's largest value (the oracle's GLU gate is 1 - 9.4e-14)."""
    cfg, net, audio, steps, cots, _ = s4conv.prepare_adjoint_case(Hc, B, L)
    sd = net.state_dict()
    full = s4conv.adjoint_reference(sd, cfg, audio, steps, cots)
    fixed = s4conv.adjoint_reference(sd, cfg, audio, steps, cots, k_tap=s4conv.oracle_taps(sd, L))
    for name in s4conv.COTANGENTS:
        assert s4conv.tensor_error(fixed[name][0], full[name][0]) < 1e-10
        assert s4conv.KERNEL + "C" in full[name][1] and s4conv.KERNEL + "C" not in fixed[name][1]
        for k in s4conv.READOUT_KEYS + s4conv.SPECTRUM_KEYS[-2:]:
            assert s4conv.tensor_error(fixed[name][1][k], full[name][1][k]) < 1e-10, (name, k)


def test_edge_cotangents_have_the_support_they_claim():
    for L in (14, 16, 250, 16384):
        c, w = s4conv.edge_cotangents(3, L, 1), max(2, L // 16)
        assert all(t.shape == (3, 1, L) for t in c.values()) and set(c) == set(s4conv.COTANGENTS)
        assert bool((c["head"][..., :w] != 0).all()) and not bool(c["head"][..., w:].any())
        assert bool((c["tail"][..., L - w:] != 0).all()) and not bool(c["tail"][..., :L - w].any())
        assert s4conv.off_support("head", L) == slice(w, L) and s4conv.off_support("tail", L) == slice(0, L - w)


def test_batch_chunk_cases_enter_the_loop_a_second_time():
    """(`fftcorr_chunks` restates `kernel_backward`.)  Every other case runs one sample per workgroup."""
    assert [s4conv.fftcorr_chunks(B, Hc) for Hc, B, _ in s4conv.ADJOINT_CASES["batch_chunks"]] == [(2, 1), (3, 2), (2, 1), (2, 1), (2, 1)]
    assert all(s4conv.fftcorr_chunks(B, Hc) == (1, 1) for g, cs in s4conv.ADJOINT_CASES.items() if g != "batch_chunks" for Hc, B, _ in cs)
    assert s4conv.fftcorr_chunks(32, 128) == (8, 8)                 # config 5 per GPU


def case_conditions(Hc, B, L, cfg, sd, audio, steps, cots, minima, k_tap, refs):
    """The conditions of one case on the reference alone (asserted), and the fp32 oracle's figures: dict measure -> worst."""
    r = s4conv.reference(sd, cfg, audio, steps, k_tap)
    far, weight = s4conv.far_tap_kernels(r["k0"], r["k1"]), s4conv.rms(r["conv"]) / s4conv.rms(r["du"])
    assert min(minima) >= 0.25, minima
    assert far >= Hc, f"only {far} of {2 * Hc} kernels hold 1 % of their peak at the last tap"
    assert weight >= 0.5, f"conv term RMS is {weight:.2f} x the RMS of D u"
    worst = dict(audio=0.0, off=0.0, readout=0.0, spectrum=0.0, share=1e30, off_on=1e30)
    for name in s4conv.COTANGENTS:
        da, grads = refs["ref"][name]
        off = s4conv.off_support(name, L)
        share = refs["branch"][name].abs()[:, 0].amax(-1) / da.abs()[:, 0].amax(-1)
        assert float(share.min()) >= 0.1, (name, share)
        worst["share"] = min(worst["share"], float(share.min()))
        if off is not None:
            ratio = da.abs()[:, 0, off].amax(-1) / s4conv.on_support_max(da, name)
            assert float(ratio.min()) >= 1e-2, (name, ratio)
            worst["off_on"] = min(worst["off_on"], float(ratio.min()))
        da32, grads32 = refs["oracle32"][name]
        every, offs = s4conv.audio_errors(da32, da, refs["branch"][name], off)
        worst["audio"] = max(worst["audio"], every[0])
        worst["off"] = max(worst["off"], offs[0] if offs else 0.0)
        worst["readout"] = max([worst["readout"]] + [s4conv.tensor_error(grads32[k], grads[k]) for k in s4conv.READOUT_KEYS])
        worst["spectrum"] = max([worst["spectrum"]] + [s4conv.tensor_error(grads32[k], grads[k]) for k in s4conv.SPECTRUM_KEYS if k in grads])
        assert all(float(grads[k].abs().max()) > 0 for k in grads if k in s4conv.READOUT_KEYS + s4conv.SPECTRUM_KEYS)
    worst.update(far=far, weight=weight)
    return worst


@pytest.mark.parametrize("Hc,B,L", ALL_CASES)
def test_case_conditions_hold_on_the_reference(Hc, B, L):
    """Weight seeds: `s4conv.ADJOINT_SEEDS` names the first seed from 5 on at which every condition here holds with a fifth
    to spare (the scalar LayerNorm gradients norm1.m / norm1.s are cancelling sums: where a seed leaves one of them small,
    the fp32 oracle itself misses a quarter of 1e-4 on it; at 16382 .. 16386 samples the off-support share decides)."""
    cfg, net, audio, steps, cots, minima = s4conv.prepare_adjoint_case(Hc, B, L)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    assert s4conv.tail_is_transparent(sd, Hc)
    taps = s4conv.oracle_taps(sd, L)
    k_tap = taps if (Hc, B, L) in s4conv.K_TAP_CASES else None
    refs = s4conv.host_references(sd, cfg, audio, steps, cots, k_tap)
    w = case_conditions(Hc, B, L, cfg, sd, audio, steps, cots, minima, taps, refs)
    print(f"S4ADJ-REF H={Hc} B={B} L={L} seed {s4conv.ADJOINT_SEEDS.get((Hc, B, L), s4conv.WEIGHT_SEED)}: ReLU minima "
          f"{minima[0]:.3f} {minima[1]:.3f}, far taps {w['far']}/{2 * Hc}, conv/Du {w['weight']:.2f}, branch share >= "
          f"{w['share']:.2f}, off/on >= {w['off_on']:.1e} | fp32 oracle: audio {w['audio']:.2e}, off support {w['off']:.2e}, "
          f"D / fc_t {w['readout']:.2e}, kernel / norm1 {w['spectrum']:.2e}")
    assert w["audio"] <= s4conv.AUDIO_BOUND / 4 and w["off"] <= s4conv.AUDIO_BOUND / 4
    assert w["readout"] <= s4conv.READOUT_BOUND / 4 and w["spectrum"] <= s4conv.SPECTRUM_BOUND / 4
    if k_tap is None:      # log_dt: the project's rule has a floor of 1e-3; the oracle must not need the cap
        from tests import gradcheck
        e = max(s4conv.tensor_error(refs["oracle32"][n][1][s4conv.LOG_DT], refs["ref"][n][1][s4conv.LOG_DT]) for n in s4conv.COTANGENTS)
        assert 3.0 * e < gradcheck.MAX_TOL, e


# ----------------------------------------------------------------------------------------------------- sensitivity
def _circular_conv(u, k0, k1):
    """The correlation wrapped at n = L: no zero padding between the two halves."""
    L = u.shape[-1]
    kk = k0.clone()
    kk[..., 1:] += k1[..., :L - 1].flip(-1)
    kk[..., 0] += k1[..., L - 1]
    return torch.fft.irfft(torch.fft.rfft(u, n=L) * torch.fft.rfft(kk, n=L), n=L)


def _moved(sd, cfg, audio, steps, cots, ref, branch, wrong):
    """The measures of the GPU test between a wrong reference and the right one, per edge cotangent:
    {name: (audio, off support, worst of D / fc_t, worst of norm1)}."""
    out = {}
    for name in ("head", "tail"):
        da, g = wrong[name]
        every, off = s4conv.audio_errors(da, ref[name][0], branch[name], s4conv.off_support(name, audio.shape[-1]))
        out[name] = (every[0], off[0], max(s4conv.tensor_error(g[k], ref[name][1][k]) for k in s4conv.READOUT_KEYS),
                     max(s4conv.tensor_error(g[k], ref[name][1][k]) for k in s4conv.SPECTRUM_KEYS[-2:]))
    return out


@pytest.mark.parametrize("Hc,B,L", [(64, 9, 1024), (8, 2, 16384)])
def test_the_measures_catch_a_wrong_adjoint(Hc, B, L):
    """Reference side only: the float64 reference on constant taps, then with the taps or the transform made wrong the way an
    adjoint kernel would be.  Each must move a measure above its bound on the head or the tail cotangent."""
    cfg, net, audio, steps, cots, _ = s4conv.prepare_adjoint_case(Hc, B, L)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    k0, k1 = s4conv.taps_from_engine(s4conv.oracle_taps(sd, L), L)
    ref = s4conv.adjoint_reference(sd, cfg, audio, steps, cots, taps=(k0, k1))
    branch = s4conv.branch_part(sd, cfg, audio, steps, cots, ref)
    k0_short = k0.clone()
    k0_short[:, -1] = 0.0
    wrongs = {"last tap of k0 dropped": dict(taps=(k0_short, k1)), "k0 and k1 swapped": dict(taps=(k1, k0)),
              "circular wrap at n = L": dict(taps=(k0, k1), conv=_circular_conv)}
    bounds = (s4conv.AUDIO_BOUND, s4conv.AUDIO_BOUND, s4conv.READOUT_BOUND, s4conv.SPECTRUM_BOUND)
    for what, kw in wrongs.items():
        m = _moved(sd, cfg, audio, steps, cots, ref, branch, s4conv.adjoint_reference(sd, cfg, audio, steps, cots, **kw))
        print(f"H={Hc} B={B} L={L}: {what}: " + "; ".join(f"{n}: audio {v[0]:.1e}, off support {v[1]:.1e}, D / fc_t {v[2]:.1e}, "
                                                          f"norm1 {v[3]:.1e}" for n, v in m.items()))
        assert any(v > b for vals in m.values() for v, b in zip(vals, bounds)), (what, m)
        if what != "last tap of k0 dropped":         # one tap of 2 H L moves one position; the others move everything
            assert all(vals[0] > 10 * bounds[0] for vals in m.values()), (what, m)
    # dD with the last sample of the first batch chunk missing: dD[h] = sum_b sum_l u da, per sample through a D of its own
    bchunk, _ = s4conv.fftcorr_chunks(B, Hc)
    leaf = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    Db = leaf[s4conv.BLOCK + ".layer.D"].expand(B, Hc).clone().requires_grad_(True)
    eps = s4conv.block_forward(leaf, cfg, audio.double(), steps, k0, k1, D=Db)["eps"]
    for name in ("head", "tail"):
        (g,) = torch.autograd.grad((eps * cots[name].double()).sum(), Db, retain_graph=True)
        want = ref[name][1][s4conv.BLOCK + ".layer.D"]
        assert s4conv.tensor_error(g.sum(0, keepdim=True), want) < 1e-12
        e = s4conv.tensor_error(g.sum(0, keepdim=True) - g[bchunk - 1], want)
        print(f"H={Hc} B={B} L={L}: sample {bchunk - 1} missing from dD, {name}: {e:.1e}")
        assert e > 100 * s4conv.READOUT_BOUND

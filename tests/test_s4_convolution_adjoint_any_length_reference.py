"""CPU: the reference side of tests/test_s4_convolution_adjoint_any_length_gpu.py (the convolution adjoint at l_max != L).

  segment identity      the float64 restatement of the segment scheme (tests/s4conv_any_length.py) equals the definition
                        `s4conv.two_sided_conv_direct`, and its adjoint -- the same accumulation on the conjugated spectra,
                        causal' and anti-causal' swapped -- equals the adjoint of the definition, term by term and through
                        <conv(u), da> = <u, conv^T(da)>; at segment sizes small enough for the double loops, with one, two
                        and three segments, a 2-sample last segment and as many taps as a segment holds
  case conditions       for EVERY GPU case, on the reference alone, with the thresholds of
                        tests/test_s4_convolution_adjoint_reference.py: both ReLUs open by 0.25, the fp32 CPU oracle within a
                        quarter of the bound on both audio measures, a branch share of at least 0.125 per row, and for the
                        head cotangent an off-support gradient of at least 1.25e-2 of the on-support one
  sensitivity           an adjoint with the causal' and anti-causal' spectra NOT swapped, and one with the spectra NOT
                        conjugated, each move both audio measures above 2e-5 on every segmented case; the right segment
                        adjoint, through the same hook, stays at float64 rounding
"""
import pytest
import torch

from tests import s4conv
from tests import s4conv_any_length as anyl


def _definition_adjoint(da, k0, k1):
    """du[i] = sum_j k0[j] da[i + j] + sum_{m >= 1} k1[m - 1] da[i - m], through the definition itself: it is
    conv(da, c', a') with c' = [k0[0], k1[0], k1[1], ...] and a' = [k0[1], k0[2], ...] (zero-filled to c's length)."""
    c = torch.cat([k0[:, :1], k1], -1)
    a = torch.cat([k0[:, 1:], torch.zeros(k0.shape[0], 2, dtype=k0.dtype)], -1)
    return s4conv.two_sided_conv_direct(da, c, a)


@pytest.mark.parametrize("S,L,Lt", [(16, 18, 16), (16, 32, 16), (16, 40, 16), (16, 48, 9), (8, 30, 8), (16, 34, 1)])
def test_segment_scheme_and_its_adjoint_equal_the_definition(S, L, Lt):
    H, B = 3, 2
    g = torch.Generator().manual_seed(S * 1000 + L)
    u, da = (torch.randn(B, H, L, generator=g, dtype=torch.float64) for _ in range(2))
    k0, k1 = (torch.randn(H, Lt, generator=g, dtype=torch.float64) for _ in range(2))
    y = s4conv.two_sided_conv_direct(u, k0, k1)
    assert float((anyl.segmented_conv(u, k0, k1, S) - y).abs().max()) < 1e-12
    assert float((s4conv.two_sided_conv_fft(u, k0, k1) - y).abs().max()) < 1e-12
    du = anyl.segmented_adjoint(da, k0, k1, S)
    assert float((du - _definition_adjoint(da, k0, k1)).abs().max()) < 1e-12
    assert abs(float((y * da).sum() - (u * du).sum())) < 1e-10
    # the two mistakes are visible here already (one tap per direction at lag 0 only: nothing crosses a segment)
    for kw in (dict(swap=False), dict(conj=False)):
        moved = float((anyl.segmented_adjoint(da, k0, k1, S, **kw) - du).abs().max())
        assert moved > 1e-2 or (Lt == 1 and "swap" in kw), (kw, moved)


def _host(case):
    H, B, l_max, L, seed = case
    cfg, net, audio, steps, cots, minima = anyl.prepare_case(*case)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    assert s4conv.tail_is_transparent(sd, H) and int(sd[s4conv.KERNEL + "L"]) == l_max
    taps = s4conv.oracle_taps(sd, l_max)
    return cfg, sd, audio, steps, cots, minima, taps


@pytest.mark.parametrize("case", anyl.ALL_CASES, ids=lambda c: "H%d-B%d-lmax%d-L%d-seed%d" % c)
def test_case_conditions_hold_on_the_reference(case):
    H, B, l_max, L, seed = case
    cfg, sd, audio, steps, cots, minima, taps = _host(case)
    assert min(minima) >= 0.25, minima
    refs = s4conv.host_references(sd, cfg, audio, steps, cots, taps)
    assert s4conv.taps_from_engine(taps, L)[0].shape == (H, min(L, l_max))
    worst = dict(audio=0.0, off=0.0, share=1e30, off_on=1e30)
    for name in s4conv.COTANGENTS:
        da = refs["ref"][name][0]
        off = s4conv.off_support(name, L)
        share = refs["branch"][name].abs()[:, 0].amax(-1) / da.abs()[:, 0].amax(-1)
        worst["share"] = min(worst["share"], float(share.min()))
        if name == "head":
            ratio = da.abs()[:, 0, off].amax(-1) / s4conv.on_support_max(da, name)
            worst["off_on"] = float(ratio.min())
        every, offs = s4conv.audio_errors(refs["oracle32"][name][0], da, refs["branch"][name], off)
        worst["audio"] = max(worst["audio"], every[0])
        worst["off"] = max(worst["off"], offs[0] if offs else 0.0)
    print(f"S4ADJ-ANY-REF H={H} B={B} l_max={l_max} L={L} seed {seed}: ReLU minima {minima[0]:.3f} {minima[1]:.3f}, branch share "
          f">= {worst['share']:.2f}, head off/on >= {worst['off_on']:.1e} | fp32 oracle: audio {worst['audio']:.2e}, off support "
          f"{worst['off']:.2e}")
    assert worst["audio"] <= s4conv.AUDIO_BOUND / 4 and worst["off"] <= s4conv.AUDIO_BOUND / 4
    assert worst["off_on"] >= 1.25e-2
    assert worst["share"] >= 0.125


@pytest.mark.parametrize("case", anyl.SEGMENTED_CASES, ids=lambda c: "H%d-B%d-lmax%d-L%d-seed%d" % c)
def test_the_measures_catch_a_wrong_segment_adjoint(case):
    H, B, l_max, L, seed = case
    cfg, sd, audio, steps, cots, minima, taps = _host(case)
    k0, k1 = s4conv.taps_from_engine(taps, L)
    ref = s4conv.adjoint_reference(sd, cfg, audio, steps, cots, taps=(k0, k1))
    branch = s4conv.branch_part(sd, cfg, audio, steps, cots, ref)

    def measures(**kw):
        wrong = s4conv.adjoint_reference(sd, cfg, audio, steps, cots, taps=(k0, k1), conv=anyl.conv_with_adjoint(
            lambda da, a, b: anyl.segmented_adjoint(da, a, b, anyl.SEGMENT, **kw)))
        out = {}
        for name in s4conv.COTANGENTS:
            every, offs = s4conv.audio_errors(wrong[name][0], ref[name][0], branch[name], s4conv.off_support(name, L))
            out[name] = (every[0], offs[0] if offs else None)
        return out

    right = measures()
    assert all(v < 1e-10 for pair in right.values() for v in pair if v is not None), right
    for what, kw in (("causal' / anti-causal' not swapped", dict(swap=False)), ("spectra not conjugated", dict(conj=False))):
        m = measures(**kw)
        print(f"H={H} B={B} l_max={l_max} L={L}: {what}: " + "; ".join(
            f"{n}: audio {v[0]:.1e}" + ("" if v[1] is None else f", off support {v[1]:.1e}") for n, v in m.items()))
        assert all(v > s4conv.AUDIO_BOUND for pair in m.values() for v in pair if v is not None), (what, m)

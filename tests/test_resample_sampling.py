"""CPU: the host side of RePaint's resampling (`dws_sampler_run_program`): `repaint_program` against the rules of its
schedule, `jump_coefficients` against an independent float64 evaluation, the Philox stream assignment, the argument
errors that are raised before any GPU work, and the two `generate.*` keys."""
import math

import numpy as np
import pytest
import torch

from tests.test_edit_sampling import _calls


def _check_walk(prog, S, j, r, start_step=None):
    """The rules of the schedule, written out independently of the generator.  Returns the network evaluations."""
    K = S if start_step is None else start_step + 1
    points = [k for k in range(0, K, j) if k + j <= K - 1]
    used = {k: 0 for k in points}
    pos, evals = K, 0
    prog = [int(a) for a in prog]
    for i, a in enumerate(prog):
        if a >= 0:
            assert a == pos - 1, (i, a, pos)                   # a reverse visit is one below the position reached
            pos, evals = a, evals + 1
            jumps_next = i + 1 < len(prog) and prog[i + 1] < 0
            assert jumps_next == (pos in used and used[pos] < r - 1), (i, pos)   # a jump point with counter above zero
        else:
            assert a == -j and i > 0 and prog[i - 1] >= 0, (i, a)
            used[pos] += 1
            pos += j
            assert pos <= K - 1
    assert pos == 0 and prog[-1] == 0                          # ends in reverse step 0
    assert all(n == r - 1 for n in used.values()), used        # every jump point used exactly r - 1 times
    assert evals == K + (r - 1) * j * len(points)              # the evaluation count of the issue
    return evals


def test_worked_example_and_the_trivial_program():
    from diffwave_sashimi_amd.sampling import program_evaluations, repaint_program
    p = repaint_program(6, 2, 2)
    assert p.dtype == np.int32 and p.tolist() == [5, 4, 3, 2, -2, 3, 2, 1, 0, -2, 1, 0]
    assert program_evaluations(6, 2, 2) == 10
    for S in (1, 2, 6, 50):
        for j in (1, 2, S + 3):
            assert repaint_program(S, j, 1).tolist() == list(range(S - 1, -1, -1))
    assert repaint_program(8, 3, 1, start_step=4).tolist() == [4, 3, 2, 1, 0]
    assert repaint_program(6, 2, 2, start_step=3).tolist() == [3, 2, 1, 0, -2, 1, 0]   # K = 4: 2 + 2 > K - 1, so 0 is the only jump point


def test_programs_are_walks_over_a_grid():
    from diffwave_sashimi_amd.sampling import program_evaluations, repaint_program
    n = 0
    for S in range(2, 51):
        for j in range(1, S):
            for r in range(1, 5):
                p = repaint_program(S, j, r)
                assert _check_walk(p, S, j, r) == program_evaluations(S, j, r) == int((p >= 0).sum())
                n += 1
    assert n == sum(S - 1 for S in range(2, 51)) * 4


def test_programs_with_a_partial_start_stay_below_it():
    from diffwave_sashimi_amd.sampling import program_evaluations, repaint_program
    for S in (6, 17, 50):
        for s0 in range(1, S):
            for j in range(1, s0 + 1):                         # K - 1 = s0
                for r in (1, 2, 4):
                    p = repaint_program(S, j, r, start_step=s0)
                    assert p[0] == s0 and int(p.max()) == s0   # nothing above position s0 + 1 is visited
                    assert _check_walk(p, S, j, r, start_step=s0) == program_evaluations(S, j, r, s0)


def _all_jumps_program(S, j):
    """One walk that jumps from every k with k + j <= S - 1 up to k + j: down to k, up, down again, one further."""
    k0 = S - 1 - j
    prog = list(range(S - 1, k0 - 1, -1))
    for k in range(k0, -1, -1):
        prog += [-j] + list(range(k + j - 1, k - 1, -1))
        if k > 0:
            prog.append(k - 1)
    return prog


def _levels(which):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, ddim_steps
    if which == "ddpm50":
        return calc_diffusion_hyperparams(50, 1e-4, 0.05)["Alpha_bar"]
    ab = calc_diffusion_hyperparams(200, 1e-4, 0.02)["Alpha_bar"]
    return ab if which == "ddpm200" else ab[ddim_steps(200, 50)]


@pytest.mark.parametrize("which", ["ddpm50", "ddpm200", "ddim50of200"])
def test_jump_coefficients_match_a_float64_evaluation(which):
    """Bit-equal to sqrt(P[k+j] / P[k]) and sqrt(1 - P[k+j] / P[k]) in float64 from the float32 levels, rounded once; the
    known region stays a q-sample of y: q1[k+j] within 2 ulps of float32(q1[k] * ja) (q1[k] and ja carry half an ulp
    each, the product adds half an ulp); ja^2 + jb^2 = 1 within 2^-22."""
    from diffwave_sashimi_amd.sampling import edit_coefficients, jump_coefficients
    lv32 = _levels(which)
    q1 = edit_coefficients(lv32)[0]
    lv = [float(v) for v in lv32.numpy()]                      # the float32 levels, exactly, as Python doubles
    S = len(lv)
    P = [1.0] + lv
    worst_ulp, worst_unit, pairs = 0, 0.0, 0
    for j in range(1, S):
        prog = _all_jumps_program(S, j)
        jc = jump_coefficients(lv32, prog)
        V = len(prog)
        assert jc.dtype == np.float32 and jc.shape == (2, V)
        pos = S
        for i, a in enumerate(prog):
            v = V - 1 - i
            if a >= 0:
                pos = a
                assert jc[0, v] == 0.0 and jc[1, v] == 0.0     # zero on reverse visits
                continue
            k = pos
            pos = k + j
            ratio = P[k + j] / P[k]
            want = (np.float32(math.sqrt(ratio)), np.float32(math.sqrt(1.0 - ratio)))
            assert (jc[0, v], jc[1, v]) == want, (k, j)
            assert 0.0 < jc[0, v] < 1.0 and 0.0 < jc[1, v] < 1.0
            prod = np.float32(q1[k]) * np.float32(jc[0, v])    # one float32 product
            assert prod.dtype == np.float32
            ulp = abs(int(np.float32(q1[k + j]).view(np.uint32)) - int(prod.view(np.uint32)))
            unit = abs(float(jc[0, v]) ** 2 + float(jc[1, v]) ** 2 - 1.0)
            worst_ulp, worst_unit, pairs = max(worst_ulp, ulp), max(worst_unit, unit), pairs + 1
            assert ulp <= 2, (k, j, ulp)
            assert unit <= 2.0 ** -22, (k, j, unit)
    assert pairs == sum(S - 1 - j + 1 for j in range(1, S))    # every k >= 0, j >= 1 with k + j <= S - 1
    print(f"{which}: {pairs} jumps, worst |q1[k+j] - q1[k] ja| = {worst_ulp} ulp, worst |ja^2 + jb^2 - 1| = {worst_unit:.2e}")


def test_jump_coefficients_follow_the_program_and_reject_a_non_walk():
    from diffwave_sashimi_amd.sampling import jump_coefficients, repaint_program
    lv = _levels("ddpm50")[:6]
    P = [1.0] + [float(v) for v in lv.numpy()]
    jc = jump_coefficients(lv, repaint_program(6, 2, 2))       # [5,4,3,2,-2,3,2,1,0,-2,1,0]: jumps at v = 7 and v = 2
    assert np.flatnonzero(jc[0]).tolist() == [2, 7]
    assert jc[0, 7] == np.float32(math.sqrt(P[4] / P[2])) and jc[0, 2] == np.float32(math.sqrt(P[2] / P[0]))
    jc = jump_coefficients(lv, repaint_program(6, 2, 2, start_step=3), start_step=3)
    assert jc.shape == (2, 7) and np.flatnonzero(jc[0]).tolist() == [2]       # [3, 2, 1, 0, -2, 1, 0]
    for bad in ([5, 4, 2, 1, 0], [4, 3, 2, 1, 0], [5, 4, 3, 2, 1], [5, 4, 3, -4, 5, 4, 3, 2, 1, 0], [5, 4, 3, 2, 1, 0, -2], []):
        with pytest.raises(ValueError):
            jump_coefficients(lv, bad)


def _stream_ids(prog):
    from diffwave_sashimi_amd.sampling import program_streams
    st = program_streams(prog)
    ids = [int(v) for v in st["visit"]] + [int(v) for v in st["known"] if v >= 0] + [int(st["x_T"]), int(st["start"])]
    return st, ids


def test_no_philox_stream_is_used_twice():
    from diffwave_sashimi_amd.sampling import repaint_program
    for S in range(2, 51):
        for j in range(1, S):
            for r in range(1, 5):
                prog = repaint_program(S, j, r)
                st, ids = _stream_ids(prog)
                V = len(prog)
                assert len(set(ids)) == len(ids) and min(ids) == 0, (S, j, r)
                assert len(st["visit"]) == V and int((st["known"] >= 0).sum()) == int((prog >= 0).sum())
                for i, a in enumerate(prog):                   # the documented ids, by visit number
                    v = V - 1 - i
                    assert st["visit"][v] == v and st["known"][v] == (V + 1 + v if a >= 0 else -1)
                assert st["x_T"] == V and st["start"] == 2 * V + 1
                if r == 1:                                     # dws_sampler_run_edit's: s, S + 1 + s, S, 2S + 1
                    assert [int(v) for v in st["visit"]] == list(range(S))
                    assert [int(v) for v in st["known"]] == [S + 1 + s for s in range(S)]
                    assert st["x_T"] == S and st["start"] == 2 * S + 1


def test_argument_errors_are_value_errors_before_any_gpu_work():
    size, calls = _calls()                                     # S = 6 steps each, size (2, 1, 16), a stub network
    B, C, L = size
    y, x = torch.zeros(size), torch.zeros(size)
    m = torch.zeros(size, dtype=torch.bool)
    km = dict(known=y, mask=m)
    bad = [
        dict(resample=(2, 2)),                                      # resampling without known / mask
        dict(resample=(2, 2), x_start=x, start_step=3),
        dict(resample=(2, 2), known=y),
        dict(km, resample=(1.5, 2)),                                # non-integer values
        dict(km, resample=(2, 2.5)),
        dict(km, resample=("2", 2)),
        dict(km, resample=(True, 2)),
        dict(km, resample=(0, 2)),                                  # jump < 1
        dict(km, resample=(-1, 2)),
        dict(km, resample=(2, 0)),                                  # resamples < 1
        dict(km, resample=2),                                       # not a pair
        dict(km, resample=(2,)),
        dict(km, resample=(6, 2)),                                  # jump > K - 1 = 5 with resamples > 1
        dict(km, resample=(3, 2), x_start=x, start_step=2),         # K = 3: jump > 2
        dict(km, resample=(2, 2), noise=torch.zeros(6, B, C, L)),   # V = 12 visits, not S = 6 rows
        dict(km, resample=(2, 2), known_noise=torch.zeros(6, B, C, L)),
        dict(km, resample=(2, 2), noise=torch.zeros(12, B, C, L + 1)),
        dict(km, resample=(2, 2), x_start=x, start_step=3, known_noise=torch.zeros(12, B, C, L)),   # K = 4: V = 7
    ]
    good = [
        dict(km, resample=(2, 2)),
        dict(km, resample=(6, 1)),                                  # no jump point needed when nothing is resampled
        dict(km, resample=(2, 2), noise=torch.zeros(12, B, C, L), known_noise=torch.zeros(12, B, C, L)),
        dict(km, resample=(2.0, 2), x_start=x, start_step=3, known_noise=torch.zeros(7, B, C, L)),
    ]
    for name, call in calls:
        for use_graph in (True, False):
            for kw in bad:
                with pytest.raises(ValueError):
                    call(use_graph=use_graph, **kw)
            for kw in good:                                        # past the checks: the stub network is reached
                with pytest.raises(AssertionError, match="touched net"):
                    call(use_graph=use_graph, **kw)


def test_generate_keys_compose_and_are_checked(tmp_path):
    from diffwave_sashimi_amd.generate import generate, load_config
    from tests.test_generate_cli import _tree
    d = _tree(tmp_path)
    cfg = load_config(d)
    for k in ("resample_jump", "resample_n"):
        assert k not in cfg["generate"]                            # absent = today's behaviour
    cfg = load_config(d, ["generate.known_name=clip", "generate.keep=[[0,8000]]", "generate.resample_jump=2",
                          "generate.resample_n=3", "generate.sampler=ddim", "generate.steps=8"])
    g = cfg["generate"]
    assert g["resample_jump"] == 2 and g["resample_n"] == 3 and g["known_name"] == "clip" and g["sampler"] == "ddim"
    # refused before a model is built or a GPU is touched
    diff = dict(T=6, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="sc09", segment_length=640, sampling_rate=16000, data_path=str(tmp_path))
    model = dict(cfg["model"])
    kw = dict(ckpt_iter="init", exp_root=str(tmp_path / "exp"))
    known = dict(known_name="clip", keep=[[0, 10]])
    with pytest.raises(ValueError, match="resample_n"):
        generate(0, diff, model, ds, resample_jump=2, **known, **kw)
    with pytest.raises(ValueError, match="resample_jump"):
        generate(0, diff, model, ds, resample_n=2, **known, **kw)
    with pytest.raises(ValueError, match="known_name"):
        generate(0, diff, model, ds, resample_jump=2, resample_n=2, **kw)
    with pytest.raises(ValueError, match="known_name"):
        generate(0, diff, model, ds, resample_jump=2, resample_n=2, start_name="clip", start_step=3, **kw)
    for sampler, extra in (("ddpm", {}), ("ddim", dict(steps=6)),
                           ("aligned", dict(diffusion_cfg=dict(diff, T=50, beta=[1e-4, 1e-3, 1e-2, 0.05, 0.2, 0.5])))):
        dcfg = extra.pop("diffusion_cfg", diff)                    # six steps with every sampler: K - 1 = 5
        with pytest.raises(ValueError, match="jump"):
            generate(0, dcfg, model, ds, sampler=sampler, resample_jump=6, resample_n=2, **known, **extra, **kw)
        with pytest.raises(ValueError, match="jump"):
            generate(0, dcfg, model, ds, sampler=sampler, resample_jump=1.5, resample_n=2, **known, **extra, **kw)
        with pytest.raises(ValueError, match="resamples"):
            generate(0, dcfg, model, ds, sampler=sampler, resample_jump=2, resample_n=0, **known, **extra, **kw)
        with pytest.raises(ValueError, match="jump"):             # K = 3 with the partial start
            generate(0, dcfg, model, ds, sampler=sampler, resample_jump=3, resample_n=2, start_name="clip", start_step=2,
                     **known, **extra, **kw)

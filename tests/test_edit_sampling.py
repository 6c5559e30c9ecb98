"""CPU: the host side of the sampler's editing modes (inpainting / continuation by known-region replacement, partial
start): `edit_coefficients` against an independent float64 evaluation, `spans_to_mask`, the argument errors that are
raised before any GPU work, and the new `generate.*` keys."""
import numpy as np
import pytest
import torch

SIX = [1e-4, 1e-3, 1e-2, 0.05, 0.2, 0.5]


class _StubNet:
    """Stands where the engine module goes: any use of it means argument checking came too late."""

    def __getattr__(self, name):
        raise AssertionError(f"the sampler touched net.{name} before rejecting its arguments")


@pytest.mark.parametrize("T,beta_T", [(50, 0.05), (200, 0.02)])
def test_edit_coefficients_match_a_float64_evaluation(T, beta_T):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, edit_coefficients
    ab = calc_diffusion_hyperparams(T, 1e-4, beta_T)["Alpha_bar"]
    q = edit_coefficients(ab)
    assert q.dtype == np.float32 and q.shape == (4, T)
    lv = [float(v) for v in ab.numpy()]                # the float32 levels, exactly, as Python doubles
    for s in range(T):
        p = 1.0 if s == 0 else lv[s - 1]
        want = [np.float32(np.sqrt(np.float64(p))), np.float32(np.sqrt(np.float64(1.0) - p)),
                np.float32(np.sqrt(np.float64(lv[s]))), np.float32(np.sqrt(np.float64(1.0) - lv[s]))]
        assert [q[r, s] for r in range(4)] == want, s
    assert q[0, 0] == 1.0 and q[1, 0] == 0.0
    assert np.all(np.diff(q[0]) < 0) and np.all(np.diff(q[2]) < 0)     # the state gets noisier with s


def test_edit_q1_row_is_ddim_k3_row():
    from diffwave_sashimi_amd.sampling import (calc_diffusion_hyperparams, ddim_coefficients, ddim_steps,
                                               edit_coefficients)
    ab = calc_diffusion_hyperparams(200, 1e-4, 0.02)["Alpha_bar"]
    tau = ddim_steps(200, 50)
    k = ddim_coefficients(ab, tau, 0.0)
    q = edit_coefficients(ab[tau])
    assert q.shape == (4, 50)
    assert np.array_equal(q[0].view(np.uint32), k[2].view(np.uint32))
    assert np.array_equal(q[2].view(np.uint32), k[1].view(np.uint32))   # n1 = sqrt(level) is DDIM's k2


def test_spans_to_mask():
    from diffwave_sashimi_amd.sampling import spans_to_mask
    m = spans_to_mask((3, 1, 20), [[2, 5], [4, 9], [19, 20]])         # overlapping spans unite
    assert m.dtype == torch.bool and m.shape[-1] == 20
    assert torch.broadcast_shapes(tuple(m.shape), (3, 1, 20)) == (3, 1, 20)
    want = torch.zeros(20, dtype=torch.bool)
    want[2:9] = True
    want[19] = True
    assert torch.equal(m.reshape(-1), want)
    assert not spans_to_mask((3, 1, 20), []).any()
    assert spans_to_mask((1, 1, 8), [[0, 8]]).all()
    for bad in ([[0, 21]], [[-1, 3]], [[5, 4]], [[1, 2, 3]], [[0.5, 3]]):
        with pytest.raises(ValueError):
            spans_to_mask((3, 1, 20), bad)


def _calls():
    """(name, call(**kw)) of the three entry points on a stub network: S = 6 steps each, size (2, 1, 16)."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling, sampling_aligned, sampling_ddim
    size = (2, 1, 16)
    net = _StubNet()
    dh6 = calc_diffusion_hyperparams(6, 1e-4, 0.05)
    dh50 = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    cfg = dict(T=50, beta_0=1e-4, beta_T=0.05, beta=SIX)
    return size, [("sampling", lambda **kw: sampling(net, size, dh6, **kw)),
                  ("aligned", lambda **kw: sampling_aligned(net, size, cfg, **kw)),
                  ("ddim", lambda **kw: sampling_ddim(net, size, dh50, 6, 0.0, **kw))]


def test_argument_errors_are_value_errors_before_any_gpu_work():
    size, calls = _calls()
    B, C, L = size
    y, x = torch.zeros(size), torch.zeros(size)
    m = torch.zeros(size, dtype=torch.bool)
    bad = [
        dict(known=y),                                              # known without mask
        dict(mask=m),                                               # mask without known
        dict(known=torch.zeros(B, C, L + 1), mask=m),               # shapes
        dict(known=y, mask=torch.zeros(B, C, L - 1, dtype=torch.bool)),
        dict(known=y, mask=torch.full(size, 2)),                    # neither bool nor 0 / 1
        dict(known=y, mask=torch.full(size, 0.5)),
        dict(known=y, mask=m, known_noise=torch.zeros(5, B, C, L)), # not [S, B, C, L]
        dict(known_noise=torch.zeros(6, B, C, L)),                  # known_noise without known
        dict(x_start=x, x_T=x),                                     # two initial states
        dict(start_step=2),                                         # start_step without x_start
        dict(start_noise=False),                                    # start_noise without x_start
        dict(x_start=x, start_step=6),                              # out of range (S = 6)
        dict(x_start=x, start_step=-1),
        dict(x_start=x, start_step=1.5),
        dict(x_start=torch.zeros(B, C, L + 1), start_step=2),       # shapes
        dict(x_start=x, start_step=2, start_noise=torch.zeros(B, C, L + 1)),
    ]
    for name, call in calls:
        for kw in bad:
            for use_graph in (True, False):
                with pytest.raises(ValueError):
                    call(use_graph=use_graph, **kw)


def test_generate_keys_compose_and_are_checked(tmp_path):
    from diffwave_sashimi_amd.generate import generate, load_config
    from tests.test_generate_cli import _tree
    d = _tree(tmp_path)
    cfg = load_config(d)
    for k in ("known_name", "keep", "start_name", "start_step", "start_noise"):
        assert k not in cfg["generate"]                            # absent = today's behaviour
    cfg = load_config(d, ["generate.known_name=clip", "generate.keep=[[0,8000],[12000,12100]]",
                          "generate.sampler=ddim", "generate.steps=8"])
    assert cfg["generate"]["known_name"] == "clip" and cfg["generate"]["keep"] == [[0, 8000], [12000, 12100]]
    assert cfg["generate"]["sampler"] == "ddim" and cfg["generate"]["n_samples"] == 16
    cfg = load_config(d, ["generate.start_name=noisy", "generate.start_step=3", "generate.start_noise=false"])
    g = cfg["generate"]
    assert g["start_name"] == "noisy" and g["start_step"] == 3 and g["start_noise"] is False
    # refused before a model is built or a GPU is touched
    diff = dict(T=6, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="sc09", segment_length=640, sampling_rate=16000, data_path=str(tmp_path))
    model = dict(cfg["model"])
    root = str(tmp_path / "exp")
    with pytest.raises(ValueError, match="keep"):
        generate(0, diff, model, ds, ckpt_iter="init", exp_root=root, known_name="clip")
    with pytest.raises(ValueError, match="keep"):
        generate(0, diff, model, ds, ckpt_iter="init", exp_root=root, known_name="clip", keep=[])
    with pytest.raises(ValueError, match="known_name"):
        generate(0, diff, model, ds, ckpt_iter="init", exp_root=root, keep=[[0, 10]])
    with pytest.raises(ValueError, match="start_step"):
        generate(0, diff, model, ds, ckpt_iter="init", exp_root=root, start_name="clip")
    with pytest.raises(ValueError, match="start_name"):
        generate(0, diff, model, ds, ckpt_iter="init", exp_root=root, start_step=2)

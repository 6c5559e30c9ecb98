"""CPU: the host side of the engine optimizer -- ``EngineAdam``'s state-dict compatibility with ``torch.optim.Adam``, its
EMA bookkeeping, the ``train.py`` key validation and ``generate.py``'s choice of weights.  The fused step itself runs on
the GPU only (tests/test_engine_optimizer_gpu.py)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.test_generate_cli import _tree


def _two_groups(seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = [nn.Parameter(torch.randn(5, generator=g)), nn.Parameter(torch.randn(3, 2, generator=g)),
          nn.Parameter(torch.randn(7, generator=g))]
    return ps, [{"params": ps[:2]}, {"params": ps[2:], "lr": 1e-2}]


def _disk(obj):
    """Through torch.save / torch.load, as a checkpoint travels (load_state_dict itself keeps the tensors it is handed)."""
    import io
    f = io.BytesIO()
    torch.save(obj, f)
    f.seek(0)
    return torch.load(f, map_location="cpu")


def _torch_steps(opt, ps, n, seed=1):
    g = torch.Generator().manual_seed(seed)
    for _ in range(n):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()


def test_state_dict_round_trip_torch_to_engine_and_back():
    from diffwave_sashimi_amd.optim import EngineAdam
    ps, groups = _two_groups()
    src = torch.optim.Adam(groups, lr=2e-4)
    _torch_steps(src, ps, 3)
    sd = _disk(src.state_dict())
    ps2, groups2 = _two_groups()
    eng = EngineAdam(groups2, lr=1.0)                     # (every lr comes from the loaded state)
    eng.load_state_dict(sd)
    assert [g["lr"] for g in eng.param_groups] == [2e-4, 1e-2]
    for p_src, p in zip(ps, ps2):
        st = eng.state[p]
        assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 3.0
        assert torch.equal(st["exp_avg"], src.state[p_src]["exp_avg"])
        assert torch.equal(st["exp_avg_sq"], src.state[p_src]["exp_avg_sq"])
    # ... and back: the engine optimizer's state_dict has torch.optim.Adam's layout, key for key
    out = _disk(eng.state_dict())
    assert set(out) == set(sd) and out["param_groups"][0].keys() == sd["param_groups"][0].keys()
    assert [g["params"] for g in out["param_groups"]] == [g["params"] for g in sd["param_groups"]]
    for k in ("lr", "betas", "eps", "weight_decay"):
        assert [g[k] for g in out["param_groups"]] == [g[k] for g in sd["param_groups"]]
    assert out["state"].keys() == sd["state"].keys()
    for i in sd["state"]:
        assert set(out["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert out["state"][i]["step"].dtype == torch.float32 and out["state"][i]["step"].shape == ()
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(out["state"][i][k], sd["state"][i][k])
    # a torch.optim.Adam resumed from the engine optimizer's state continues exactly like the original
    ps3, groups3 = _two_groups()
    for a, b in zip(ps3, ps):
        a.data.copy_(b.data)
    back = torch.optim.Adam(groups3, lr=1.0)
    back.load_state_dict(out)
    _torch_steps(src, ps, 2, seed=5)
    _torch_steps(back, ps3, 2, seed=5)
    for a, b in zip(ps3, ps):
        assert torch.equal(a, b)
    assert float(back.state[ps3[0]]["step"]) == 5.0 and [g["lr"] for g in back.param_groups] == [2e-4, 1e-2]


def test_step_on_cpu_raises_and_bad_parameters_are_refused():
    from diffwave_sashimi_amd.optim import EngineAdam
    ps, groups = _two_groups()
    opt = EngineAdam(groups, lr=2e-4, ema_decay=0.99, max_grad_norm=1.0)
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(RuntimeError, match="GPU only|no CPU fallback"):
        opt.step()
    assert all(torch.equal(a, b) for a, b in zip(before, ps))         # and nothing was half done
    with pytest.raises(TypeError, match="float32"):
        EngineAdam([nn.Parameter(torch.zeros(4, dtype=torch.float64))], lr=1e-3)
    with pytest.raises(ValueError, match="contiguous"):
        EngineAdam([nn.Parameter(torch.zeros(4, 6).t())], lr=1e-3)
    for bad in (dict(ema_decay=0.0), dict(ema_decay=1.0), dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError, match="ema_decay|max_grad_norm"):
            EngineAdam([nn.Parameter(torch.zeros(4))], lr=1e-3, **bad)
    with pytest.raises(TypeError, match="EngineModule"):
        EngineAdam([nn.Parameter(torch.zeros(4))], lr=1e-3, module=nn.Linear(2, 2))


def test_ema_state_dict_replaces_parameters_and_keeps_buffers():
    from diffwave_sashimi_amd.optim import EngineAdam
    net = nn.Sequential(nn.Conv1d(2, 3, 1), nn.BatchNorm1d(3))
    net[0] = nn.utils.weight_norm(net[0])
    opt = EngineAdam(net.parameters(), lr=1e-3, ema_decay=0.9)
    start = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        for p in net.parameters():
            p.add_(1.0)                                                   # the weights move on, the shadows stay
        net[1].running_mean.add_(2.0)
    ema = opt.ema_state_dict(net)
    assert list(ema) == list(net.state_dict())
    names = {n for n, _ in net.named_parameters()}
    assert {"0.weight_g", "0.weight_v"} <= names                      # g and v are separate shadows
    for k, v in ema.items():
        if k in names:
            assert torch.equal(v, start[k]) and not torch.equal(v, net.state_dict()[k])
        else:                                                             # buffers (and int64 counters) as they are now
            assert torch.equal(v, net.state_dict()[k]) and v.dtype == net.state_dict()[k].dtype
    # restore into another optimizer; reset_ema starts over from the weights
    opt2 = EngineAdam(net.parameters(), lr=1e-3, ema_decay=0.9)
    assert all(torch.equal(opt2.ema_state_dict(net)[k], net.state_dict()[k]) for k in names)
    opt2.load_ema_state_dict(ema, net)
    assert all(torch.equal(opt2.ema_state_dict(net)[k], start[k]) for k in names)
    opt2.reset_ema()
    assert all(torch.equal(opt2.ema_state_dict(net)[k], net.state_dict()[k]) for k in names)
    with pytest.raises(KeyError):
        opt2.load_ema_state_dict({}, net)
    with pytest.raises(RuntimeError, match="no EMA"):
        EngineAdam(net.parameters(), lr=1e-3).ema_state_dict(net)


BAD_KEYS = [
    (dict(optimizer="adamw"), "train.optimizer"),
    (dict(ema_decay=0.999), "train.ema_decay"),                               # needs optimizer=engine
    (dict(optimizer="torch", ema_decay=0.999), "train.ema_decay"),
    (dict(clip_grad_norm=1.0), "train.clip_grad_norm"),
    (dict(optimizer="torch", clip_grad_norm=1.0), "train.clip_grad_norm"),
    (dict(optimizer="engine", ema_decay=0.0), "train.ema_decay"),
    (dict(optimizer="engine", ema_decay=1.0), "train.ema_decay"),
    (dict(optimizer="engine", ema_decay=-0.5), "train.ema_decay"),
    (dict(optimizer="engine", ema_decay="fast"), "train.ema_decay"),
    (dict(optimizer="engine", ema_decay=True), "train.ema_decay"),
    (dict(optimizer="engine", clip_grad_norm=0.0), "train.clip_grad_norm"),
    (dict(optimizer="engine", clip_grad_norm=-1.0), "train.clip_grad_norm"),
    (dict(optimizer="engine", clip_grad_norm=float("nan")), "train.clip_grad_norm"),
]


@pytest.fixture
def no_model(monkeypatch):
    """Any attempt to build a model (or to load data) fails the test."""
    import diffwave_sashimi_amd.models as models
    import diffwave_sashimi_amd.train as train_mod

    def boom(*a, **k):
        raise AssertionError("a model / data loader was built before the optimizer keys were checked")
    monkeypatch.setattr(models, "construct_model", boom)
    monkeypatch.setattr(train_mod, "dataloader", boom)


@pytest.mark.parametrize("keys,named", BAD_KEYS, ids=[str(i) for i in range(len(BAD_KEYS))])
def test_train_key_validation_raises_before_any_model_is_built(tmp_path, no_model, keys, named):
    from diffwave_sashimi_amd.train import train
    with pytest.raises(ValueError, match=named.replace(".", r"\.")):
        train(0, 1, diffusion_cfg={"T": 8, "beta_0": 1e-4, "beta_T": 0.05}, model_cfg={"_name_": "wavenet", "unconditional": True},
              dataset_cfg={"_name_": "synthetic"}, generate_cfg={}, ckpt_iter=-1, n_iters=1, iters_per_ckpt=1,
              iters_per_logging=1, learning_rate=2e-4, batch_size_per_gpu=1, exp_root=str(tmp_path / "exp"), **keys)
    assert not (tmp_path / "exp").exists()                                # not even a run directory


def test_train_cli_keys_reach_the_validation(tmp_path, no_model):
    from diffwave_sashimi_amd.train import main, optimizer_options
    d = _tree(tmp_path / "configs")
    common = ["--config-dir", d, "--exp-root", str(tmp_path / "exp"), "model=wavenet", "dataset._name_=synthetic",
              "+train.ckpt_iter=-1", "+train.n_iters=1", "+train.iters_per_ckpt=1", "+train.iters_per_logging=1",
              "+train.learning_rate=2e-4", "+train.batch_size_per_gpu=1"]
    with pytest.raises(ValueError, match=r"train\.ema_decay needs train\.optimizer=engine"):
        main(common + ["+train.ema_decay=0.9"])
    with pytest.raises(ValueError, match=r"train\.clip_grad_norm needs train\.optimizer=engine"):
        main(common + ["+train.optimizer=torch", "+train.clip_grad_norm=1.0"])
    with pytest.raises(ValueError, match=r"train\.ema_decay"):
        main(common + ["+train.optimizer=engine", "+train.ema_decay=1.5"])
    with pytest.raises(AssertionError, match="before the optimizer keys"):   # valid keys get past the check (to the stub)
        main(common + ["+train.optimizer=engine", "+train.ema_decay=0.9", "+train.clip_grad_norm=1.0"])
    assert optimizer_options() == ("torch", None, None)
    assert optimizer_options("engine", 0.9, 2) == ("engine", 0.9, 2.0)
    assert optimizer_options("engine") == ("engine", None, None)


@pytest.mark.parametrize("present", [True, False])
@pytest.mark.parametrize("ema", [None, True, False])
def test_generate_ema_selection(present, ema):
    from diffwave_sashimi_amd.generate import weights_key
    ck = {"model_state_dict": {}, "optimizer_state_dict": {}}
    if present:
        ck["ema_state_dict"] = {}
    if ema is True and not present:
        with pytest.raises(ValueError, match=r"generate\.ema=true.*no ema_state_dict"):
            weights_key(ck, ema)
        return
    want = "ema_state_dict" if (present and ema is not False) else "model_state_dict"
    assert weights_key(ck, ema) == want
    assert weights_key(ck, ema=ema) == weights_key(ck, ema, None)


def test_generate_ema_with_ckpt_smooth_and_bad_values(tmp_path):
    from diffwave_sashimi_amd.generate import generate, weights_key
    ck = {"model_state_dict": {}, "ema_state_dict": {}}
    with pytest.raises(ValueError, match=r"generate\.ema=true does not combine with generate\.ckpt_smooth"):
        weights_key(ck, True, ckpt_smooth=1000)
    assert weights_key(ck, None, ckpt_smooth=1000) == "model_state_dict"        # smoothing averages the raw weights
    assert weights_key(ck, False, ckpt_smooth=1000) == "model_state_dict"
    for bad in ("yes", 1, 0.5):
        with pytest.raises(ValueError, match=r"generate\.ema"):
            weights_key(ck, bad)
    # the driver refuses the combination before it builds a model (there is no GPU here: a model would raise otherwise)
    cfgs = dict(diffusion_cfg={"T": 8, "beta_0": 1e-4, "beta_T": 0.05}, model_cfg={"_name_": "wavenet", "unconditional": True},
                dataset_cfg={"_name_": "synthetic", "segment_length": 64, "sampling_rate": 16000})
    with pytest.raises(ValueError, match=r"generate\.ckpt_smooth"):
        generate(0, ckpt_iter=10, ckpt_smooth=5, ema=True, exp_root=str(tmp_path), **cfgs)
    with pytest.raises(ValueError, match=r"no ema_state_dict"):
        generate(0, ckpt_iter="init", ema=True, exp_root=str(tmp_path), **cfgs)


def test_recipe_baseline_and_its_state_in_engine_adam():
    """A sanity check of the reference the GPU tests use (tests/adam_reference.py), and its Adam state in ``EngineAdam``.
    The fixed recipe of the GPU tests, on the CPU: fp32 ``torch.optim.Adam`` sits ~1e-7 from float64 on it (a few ulp
    of max |p|), so a bound of twice that error is tight, and the float64 reference here agrees with torch's own
    float64 Adam to rounding."""
    from tests.adam_reference import AdamPair, recipe
    sizes, params, grads = recipe(4096)
    pair = AdamPair(params, [2e-4] * len(sizes), ema_decay=0.999)
    tp64 = [nn.Parameter(torch.from_numpy(np.asarray(p, dtype=np.float64).copy())) for p in params]
    opt64 = torch.optim.Adam(tp64, lr=2e-4, foreach=False)
    for gs in grads:
        pair.step(gs)
        for p, g in zip(tp64, gs):
            p.grad = torch.from_numpy(g.astype(np.float64))
        opt64.step()
    assert max(float(np.max(np.abs(a.detach().numpy() - b))) for a, b in zip(tp64, pair.p)) < 1e-14
    _, base_p, ulp_p = pair.errors("p", pair.p)
    _, base_e, _ = pair.errors("ema", pair.ema)
    assert 2e-8 < base_p < 5e-7 and 2e-8 < base_e < 5e-7 and ulp_p < base_p * 2
    # the baseline's state after the 20 steps, as a checkpoint, in EngineAdam: step 20 everywhere, the moments bit for bit,
    # no entry for a parameter that never had a gradient, and the shadows a copy of the parameters
    from diffwave_sashimi_amd.optim import EngineAdam
    extra = nn.Parameter(torch.zeros(3))
    eng = EngineAdam([{"params": pair.tp + [extra], "lr": 2e-4}], lr=1.0, ema_decay=0.999)
    sd = _disk(pair.opt.state_dict())
    sd["param_groups"][0]["params"].append(len(pair.tp))
    eng.load_state_dict(sd)
    eng._pack_steps()
    out = eng.state_dict()
    assert sorted(out["state"]) == list(range(len(pair.tp)))
    for i, p in enumerate(pair.tp):
        assert float(out["state"][i]["step"]) == 20.0
        assert torch.equal(out["state"][i]["exp_avg"], pair.opt.state[p]["exp_avg"])
        assert torch.equal(eng.ema_state_dict(nn.ParameterList(pair.tp))[str(i)], p.detach())

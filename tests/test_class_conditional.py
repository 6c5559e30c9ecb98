"""Class-conditional generation, host side (CPU): the folded-bias reference against a patched-embedding evaluation, the
parameter layout, the RNG contract of ``training_loss``, the SC09 class mapping and every refusal that is raised before a
model or the GPU is touched."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import label_reference as lr


@pytest.mark.parametrize("name", ["wn_tiny", "ss_tiny"])
def test_folded_bias_reference_equals_the_patched_embedding(name):
    """fc_t is linear, so adding table[y] to the embedding equals folding fc_t.weight @ table[y] into fc_t.bias: the
    per-clip loop over the UNCHANGED oracle and the batched oracle with a patched step_embedding_mlp agree in float64."""
    if name.startswith("wn"):
        cfg, _, L, wseed, iseed, _ = cases.WAVENET_CASES[name]
    else:
        cfg, _, wseed, iseed, _ = cases.SASHIMI_CASES[name]
        L = cfg["L"]
    sd = lr.to64(lr.state(lr.build(cfg, wseed)))
    audio, _ = cases.wavenet_inputs(3, L, 1, iseed)
    steps = torch.tensor(lr.STEPS)
    with torch.no_grad():
        a = lr.forward(sd, cfg, audio, steps, lr.LABELS)
        b = lr.patched_forward(sd, cfg, audio, steps, lr.LABELS)
        null = lr.forward(sd, cfg, audio, steps, None)
    err = float((a - b).abs().max() / b.abs().max())
    moved = float((a - null).abs().max() / a.abs().max())
    print(f"{name}: folded vs patched {err:.1e}; labels move the output by {moved:.2f} of its largest magnitude")
    assert err <= 1e-12
    assert moved > 0.05
    assert torch.equal(a[1], null[1])          # clip 1 carries the null class


@pytest.mark.parametrize("name", ["wn_tiny", "ss_tiny"])
def test_batched_reference_equals_the_per_clip_loop(name):
    """The GPU gradient tests evaluate the folded biases for all clips in one oracle call (the S4 kernels are then
    generated once, not per clip): same values and same float64 gradients as the per-clip loop."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from tests import gradcheck
    if name.startswith("wn"):
        cfg, _, L, wseed, _, _ = cases.WAVENET_CASES[name]
    else:
        cfg, _, wseed, _, _ = cases.SASHIMI_CASES[name]
        L = cfg["L"]
    sd = lr.state(lr.build(cfg, wseed))
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    audio = torch.randn(3, 1, L, generator=torch.Generator().manual_seed(9)) * 0.3
    loss_of = gradcheck.mse_training_loss(audio, dh, None, generator=torch.Generator().manual_seed(21))
    la, ga = lr.grads(cfg, sd, loss_of, lr.LABELS, torch.float64)
    lb, gb = lr.grads(cfg, sd, loss_of, lr.LABELS, torch.float64, batched=True)
    assert abs(la - lb) <= 1e-12 * abs(la)
    worst = max(gradcheck.errors(gb, ga).values())
    print(f"{name}: batched vs per-clip float64 gradients {worst:.1e}")
    assert worst <= 1e-10
    tk = lr.table_key(cfg)
    assert float(ga[tk][0].abs().max()) == 0.0 and float(ga[tk][2].abs().max()) == 0.0 and float(ga[tk][1].abs().max()) > 0


@pytest.mark.parametrize("name", ["wn_tiny", "ss_tiny"])
def test_n_classes_adds_exactly_one_parameter(name):
    from diffwave_sashimi_amd.models import construct_model, model_identifier
    cfg = (cases.WAVENET_CASES if name.startswith("wn") else cases.SASHIMI_CASES)[name][0]
    plain = construct_model(dict(cfg))
    assert not any("label_embedding" in k for k in plain.state_dict())
    for none in (None, 0):
        assert list(construct_model(dict(cfg, n_classes=none)).state_dict()) == list(plain.state_dict())
    net = construct_model(dict(cfg, n_classes=3))
    extra = [k for k in net.state_dict() if k not in plain.state_dict()]
    assert extra == [lr.table_key(cfg)]
    assert [k for k in plain.state_dict() if k not in net.state_dict()] == []
    assert tuple(net.state_dict()[extra[0]].shape) == (4, 512)
    assert net.state_dict()[extra[0]].dtype == torch.float32
    assert model_identifier(dict(cfg, n_classes=3)) == model_identifier(cfg) + "_cls3"
    assert model_identifier(dict(cfg, n_classes=None)) == model_identifier(cfg)
    for bad in (-1, 1.5, True, "3"):
        with pytest.raises((ValueError, TypeError)):
            construct_model(dict(cfg, n_classes=bad))


class _StubNet:
    """Records what training_loss hands to the network."""
    n_classes = 3

    def __init__(self):
        self.calls = []

    def __call__(self, inp, mel_spec=None, **kw):
        self.calls.append((inp[0].clone(), inp[1].clone(), kw))
        return inp[0] * 0.5


def test_training_loss_label_dropout_consumes_the_rng_after_the_existing_draws():
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    dh = calc_diffusion_hyperparams(20, 1e-4, 0.05)
    B = 64
    audio = torch.randn(B, 1, 16, generator=torch.Generator().manual_seed(1))
    labels = torch.arange(B) % 3
    loss_fn = torch.nn.MSELoss()

    def run(**kw):
        g = torch.Generator().manual_seed(5)
        net = _StubNet()
        training_loss(net, loss_fn, audio, dh, generator=g, **kw)
        return net.calls[0], g.get_state()

    (x0, t0, kw0), s0 = run()
    assert kw0 == {}                                     # an unlabelled call reaches the network as it always did
    (x1, t1, kw1), s1 = run(labels=None, label_dropout=0.3)
    (x2, t2, kw2), s2 = run(labels=labels, label_dropout=0.0)
    assert torch.equal(s0, s1) and torch.equal(s0, s2)   # no extra draw
    assert torch.equal(x0, x2) and torch.equal(t0, t2) and torch.equal(kw2["labels"], labels)
    p = 0.3
    (x3, t3, kw3), s3 = run(labels=labels, label_dropout=p)
    assert torch.equal(x0, x3) and torch.equal(t0, t3)   # t and z are the unlabelled run's
    assert not torch.equal(s0, s3)
    g = torch.Generator().manual_seed(5)                 # re-draw: steps, noise, then the mask
    torch.randint(20, size=(B, 1, 1), generator=g)
    torch.normal(0, 1, size=audio.shape, generator=g)
    drop = torch.rand(B, generator=g) < p
    assert 0 < int(drop.sum()) < B
    assert torch.equal(kw3["labels"], torch.where(drop, torch.full_like(labels, 3), labels))
    assert torch.equal(g.get_state(), s3)


def _write_wav(path, n=400):
    from scipy.io import wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, 16000, (np.arange(n) % 50).astype(np.int16))


def test_sc09_class_mapping(tmp_path):
    from diffwave_sashimi_amd.train import SpeechCommands, SyntheticClips, dataloader
    for folder, stem in (("two", "a_nohash_0"), ("one", "b_nohash_0"), ("zero", "c_nohash_1"), ("one", "d_nohash_2"),
                         ("_background_noise_", "n_nohash_0")):
        _write_wav(str(tmp_path / folder / f"{stem}.wav"))
    ds = SpeechCommands(str(tmp_path), 400)
    assert ds.classes == ["one", "two", "zero"]
    assert [ds[i][2] for i in range(len(ds))] == ["one", "one", "two", "zero"]      # the default items are unchanged
    di = SpeechCommands(str(tmp_path), 400, label_index=True)
    assert [di[i][2] for i in range(len(di))] == [0, 0, 1, 2]
    cfg = {"_name_": "sc09", "data_path": str(tmp_path), "segment_length": 400}
    batch = next(iter(dataloader(cfg, 4, 1, num_workers=0, n_classes=3)))
    assert batch[2].tolist() == [0, 0, 1, 2] and batch[0].shape == (4, 1, 400)
    with pytest.raises(ValueError, match="class folders"):
        dataloader(cfg, 4, 1, num_workers=0, n_classes=10)
    syn = SyntheticClips(7, 8, n_classes=3)
    assert [syn[i][2] for i in range(7)] == [0, 1, 2, 0, 1, 2, 0]
    assert SyntheticClips(2, 8)[1][2] == "synthetic"
    with pytest.raises(ValueError, match="ljspeech"):
        dataloader({"_name_": "ljspeech", "data_path": str(tmp_path)}, 2, 1, unconditional=False, n_classes=3)


def _gen(tmp_path, model=None, **kw):
    from diffwave_sashimi_amd.generate import generate
    model = dict(cases.WAVENET_CASES["wn_tiny"][0], **(model or {}))
    return generate(0, dict(T=4, beta_0=1e-4, beta_T=0.05), model, dict(segment_length=64, sampling_rate=16000),
                    ckpt_iter="init", n_samples=2, exp_root=str(tmp_path / "exp"), **kw)


def test_generate_refusals_come_before_a_model_is_built(tmp_path):
    cls = {"n_classes": 3}
    with pytest.raises(ValueError, match="n_classes"):
        _gen(tmp_path, label=1)
    with pytest.raises(ValueError, match="generate.label"):
        _gen(tmp_path, cls, cfg_scale=1.0)
    for bad in (4, -1, [0, 7], "some", 1.5, [], True):
        with pytest.raises(ValueError, match="generate.label"):
            _gen(tmp_path, cls, label=bad)
    with pytest.raises(ValueError, match="cfg_scale"):
        _gen(tmp_path, cls, label=1, cfg_scale=float("nan"))
    with pytest.raises(ValueError, match="editing"):
        _gen(tmp_path, cls, label=1, cfg_scale=1.0, known_name="x", keep=[[0, 8]])
    with pytest.raises(ValueError, match="editing"):
        _gen(tmp_path, cls, label=1, cfg_scale=1.0, start_name="x", start_step=1)
    with pytest.raises(ValueError, match="guide_name"):
        _gen(tmp_path, cls, label=1, cfg_scale=1.0, guide_name="x", guide_op="declip", guide_scale=1.0)
    assert not os.path.exists(tmp_path / "exp")          # nothing was created: the checks precede every side effect


def test_train_refusals(tmp_path):
    from diffwave_sashimi_amd.train import train
    cfg = cases.WAVENET_CASES["wn_tiny"][0]
    common = dict(diffusion_cfg=dict(T=4, beta_0=1e-4, beta_T=0.05), generate_cfg={}, ckpt_iter=-1, n_iters=1,
                  iters_per_ckpt=10, iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=2,
                  exp_root=str(tmp_path / "exp"), num_workers=0)
    syn = {"_name_": "synthetic", "n_items": 4, "segment_length": 64}
    with pytest.raises(ValueError, match="label_dropout"):
        train(0, 1, model_cfg=dict(cfg), dataset_cfg=syn, label_dropout=0.2, **common)
    with pytest.raises(ValueError, match="label_dropout"):
        train(0, 1, model_cfg=dict(cfg, n_classes=3), dataset_cfg=syn, label_dropout=1.0, **common)
    with pytest.raises(ValueError, match="ljspeech"):
        train(0, 1, model_cfg=dict(cfg, n_classes=3, unconditional=False),
              dataset_cfg={"_name_": "ljspeech", "data_path": str(tmp_path), "segment_length": 64, "hop_length": 256,
                           "sampling_rate": 22050}, **common)


def test_sampling_refusals_come_before_anything_runs():
    """On CPU modules: every refusal is raised by the argument checks, before the engine is touched."""
    from diffwave_sashimi_amd import sampling as S
    cfg = cases.WAVENET_CASES["wn_tiny"][0]
    plain, net = cases.build_ours(cfg, 1), cases.build_ours(dict(cfg, n_classes=3), 1)
    dh = S.calc_diffusion_hyperparams(6, 1e-4, 0.05)
    size = (2, 1, 64)
    known, mask = torch.zeros(size), torch.ones(size, dtype=torch.bool)
    runs = {
        "sampling": lambda n, **kw: S.sampling(n, size, dh, **kw),
        "ddim": lambda n, **kw: S.sampling_ddim(n, size, dh, 3, **kw),
        "dpmpp": lambda n, **kw: S.sampling_dpmpp(n, size, dh, 3, **kw),
        "aligned": lambda n, **kw: S.sampling_aligned(n, size, dict(T=6, beta_0=1e-4, beta_T=0.05, beta=[1e-4, 1e-2, 0.05]),
                                                      **kw),
    }
    for name, run in runs.items():
        with pytest.raises(ValueError, match="without classes"):
            run(plain, labels=[0, 1])
        with pytest.raises(ValueError, match="needs labels"):
            run(net, cfg_scale=1.0)
        with pytest.raises(ValueError, match="editing"):
            run(net, labels=[0, 1], cfg_scale=1.0, known=known, mask=mask)
        with pytest.raises(ValueError, match="editing"):
            run(net, labels=[0, 1], cfg_scale=1.0, x_start=known, start_step=1)
        with pytest.raises(ValueError, match="resampl"):
            run(net, labels=[0, 1], cfg_scale=1.0, known=known, mask=mask, resample=(1, 2))
        with pytest.raises(ValueError, match="labels must"):
            run(net, labels=[0, 4])
        with pytest.raises(ValueError, match="labels must"):
            run(net, labels=[0, 1, 2])
        with pytest.raises(ValueError, match="labels must"):
            run(net, labels=torch.tensor([0.0, 1.0]))
        with pytest.raises(ValueError, match="cfg_scale"):
            run(net, labels=[0, 1], cfg_scale=float("inf"))
    guided = dict(measurement=torch.zeros(size), operator=lambda x: x, scale=1.0)
    with pytest.raises(ValueError, match="cfg_scale"):
        S.sampling_guided(net, size, dh, labels=[0, 1], cfg_scale=1.0, **guided)
    with pytest.raises(ValueError, match="without classes"):
        S.sampling_guided(plain, size, dh, labels=[0, 1], **guided)
    with pytest.raises(ValueError, match="without classes"):
        plain((torch.zeros(size), torch.zeros(2, 1)), labels=[0, 1])

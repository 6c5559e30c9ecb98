"""CPU: the host side of ragged batches -- the batch plan of ``generate.mel_names`` and the argument checks that need no
device."""
import random

import pytest
import torch

from tests import cases


def test_ragged_plan_covers_every_utterance_once_longest_first():
    from diffwave_sashimi_amd.generate import ragged_plan
    rng = random.Random(7)
    for n, bs in ((1, 1), (5, 2), (16, 16), (17, 4), (40, 7), (9, 100)):
        frames = [rng.randint(1, 12) for _ in range(n)]
        plan = ragged_plan(frames, bs)
        flat = [k for batch in plan for k in batch]
        assert sorted(flat) == list(range(n))                               # every index exactly once
        assert all(1 <= len(batch) <= bs for batch in plan)                 # never more than batch_size
        assert all(len(batch) == bs for batch in plan[:-1])                 # only the last may be short
        lens = [frames[k] for k in flat]
        assert lens == sorted(lens, reverse=True)                           # longest first, across the batches too
        for a, b in zip(flat, flat[1:]):                                    # equal lengths keep their order
            assert frames[a] != frames[b] or a < b
    assert ragged_plan([3, 5, 3, 9, 1], 2) == [[3, 1], [0, 2], [4]]
    assert ragged_plan([], 4) == []


def test_ragged_plan_refuses_bad_arguments():
    from diffwave_sashimi_amd.generate import ragged_plan
    for bs in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            ragged_plan([1, 2], bs)
    for frames in ([0, 1], [1, -2], [1.5], [True]):
        with pytest.raises(ValueError):
            ragged_plan(frames, 2)


def test_mel_names_checks_come_before_a_model_is_built(tmp_path):
    from diffwave_sashimi_amd.generate import generate
    cfg = dict(cases.WAVENET_COND_CASES["wn_cond_tiny"][0])
    diff = dict(T=4, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="ljspeech", data_path=str(tmp_path), segment_length=768, sampling_rate=22050, hop_length=256)
    kw = dict(ckpt_iter="init", exp_root=str(tmp_path / "exp"))
    for bad, match in ((dict(mel_names=["a"], mel_name="a"), "exclude"), (dict(mel_names=[]), "list of wav stems"),
                       (dict(mel_names=["a", "a"]), "twice"), (dict(mel_names=["a", 3]), "list of wav stems"),
                       (dict(mel_names=["a"], clip_seeds=True), "generate.seed"),
                       (dict(mel_names=["a"], known_name="a", keep=[[0, 1]]), "does not combine"),
                       (dict(mel_names=["a"], cfg_scale=1.0), "does not combine"),
                       (dict(mel_names=["a"], clip_seeds=True, seed=1, clips=[0]), "does not combine")):
        with pytest.raises(ValueError, match=match):
            generate(None, diff, cfg, ds, **kw, **bad)
    with pytest.raises(ValueError, match="mel-conditional"):
        generate(None, diff, dict(cases.WAVENET_CASES["wn_tiny"][0]), ds, mel_names=["a"], **kw)


def test_lengths_argument_form_is_checked_without_a_device():
    from diffwave_sashimi_amd.models.engine import EngineModule
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling, sampling_ddim, sampling_guided
    assert EngineModule._length_list(None) == ()
    assert EngineModule._length_list([5, 3]) == (5, 3)
    assert EngineModule._length_list(torch.tensor([7, 1], dtype=torch.int32)) == (7, 1)
    for bad in ([1.0, 2.0], torch.tensor([[1, 2]]), [True, False], [], [2 ** 40]):
        with pytest.raises(ValueError):
            EngineModule._length_list(bad)
    net = cases.build_ours(cases.WAVENET_CASES["wn_tiny"][0], 1)
    dh = calc_diffusion_hyperparams(4, 1e-4, 0.05)
    with pytest.raises(ValueError, match="cfg_scale"):
        sampling(net, (2, 1, 64), dh, lengths=[64, 10], labels=[0, 0], cfg_scale=1.0)
    with pytest.raises(ValueError, match="entries"):
        sampling_ddim(net, (2, 1, 64), dh, 2, lengths=[64, 10, 3])
    with pytest.raises(ValueError, match="lengths"):
        sampling_guided(net, (2, 1, 64), dh, measurement=torch.zeros(2, 1, 64), operator=lambda v: v, scale=1.0,
                        lengths=[64, 10])
    with pytest.raises(ValueError, match="needs lengths"):
        net._set_lengths(None, None, [1, 2])
    # a training call with lengths is refused before the engine is touched (the device check comes first)
    with pytest.raises(RuntimeError, match="GPU only|no CPU fallback"):
        net((torch.zeros(2, 1, 64), torch.zeros(2, 1)), lengths=[64, 10])

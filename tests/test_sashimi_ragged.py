"""CPU: the host side of ragged SaShiMi batches -- the rule that every per-clip length is a multiple of the product of the
pooling factors (module call and samplers: NotImplementedError, the engine's error class, before anything is enqueued) and
the hop check of ``generate.mel_names`` (ValueError before a model is built).  Neither needs a device."""
import pytest
import torch

from tests import cases


def test_a_length_that_does_not_divide_through_the_pooling_stages_is_refused():
    from diffwave_sashimi_amd.models.sashimi import pool_span
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling, sampling_ddim
    assert pool_span([4, 4]) == 16 and pool_span([2]) == 2 and pool_span([]) == 1
    net = cases.build_ours(cases.SASHIMI_CASES["ss_tiny"][0], 1)                   # pool [4, 4]
    assert net._length_multiple == 16
    assert net._lengths_checked(None) == ()
    assert net._lengths_checked([1024, 16]) == (1024, 16)
    assert net._lengths_checked(torch.tensor([512, 0])) == (512, 0)                # the range is the engine's to check
    for bad in ([1024, 100], [1025, 16], [8, 16]):
        with pytest.raises(NotImplementedError, match="multiple of 16"):
            net._lengths_checked(bad)
    with pytest.raises(ValueError):                                                # the form comes first
        net._lengths_checked([1024.0, 16.0])
    knobs = cases.build_ours(cases.SASHIMI_CASES["ss_knobs"][0], 1)                # pool [2]
    assert knobs._lengths_checked([250, 128, 2]) == (250, 128, 2)
    with pytest.raises(NotImplementedError, match="multiple of 2"):
        knobs._lengths_checked([250, 125, 2])
    # WaveNet takes any length
    wn = cases.build_ours(cases.WAVENET_CASES["wn_tiny"][0], 1)
    assert wn._lengths_checked([300, 131, 7]) == (300, 131, 7)
    # the samplers refuse before the engine is touched (no device here: getting past the check would fail otherwise)
    dh = calc_diffusion_hyperparams(4, 1e-4, 0.05)
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        sampling(net, (2, 1, 1024), dh, lengths=[1024, 100])
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        sampling_ddim(net, (2, 1, 1024), dh, 2, lengths=[1000, 16])
    with pytest.raises(ValueError, match="entries"):
        sampling_ddim(net, (2, 1, 1024), dh, 2, lengths=[1024, 16, 16])
    # a module call: the device check comes first, as on WaveNet
    with pytest.raises(RuntimeError, match="GPU only|no CPU fallback"):
        net((torch.zeros(2, 1, 1024), torch.zeros(2, 1)), lengths=[1024, 100])


def test_mel_names_with_sashimi_checks_the_hop_before_a_model_is_built(tmp_path):
    from diffwave_sashimi_amd.generate import _check_ragged_hop, generate
    cfg = dict(cases.SASHIMI_COND_CASES["ss_cond_tiny"][0])                        # pool [4, 4], mel_upsample [16, 16]
    diff = dict(T=4, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="ljspeech", data_path=str(tmp_path), segment_length=512, sampling_rate=22050, hop_length=200)
    kw = dict(ckpt_iter="init", exp_root=str(tmp_path / "exp"))
    with pytest.raises(ValueError, match="hop_length=200 is not a multiple of 16"):
        generate(None, diff, cfg, ds, mel_names=["a", "b"], **kw)
    with pytest.raises(ValueError, match="multiple of 8"):
        generate(None, diff, dict(cfg, pool=[2, 4]), dict(ds, hop_length=260), mel_names=["a"], **kw)
    for hop in (0, -16, 16.0, True):
        with pytest.raises(ValueError, match="multiple of 16"):
            _check_ragged_hop(cfg, dict(ds, hop_length=hop))
    # hops that divide through, and WaveNet with any hop: no objection
    for hop in (16, 256, 320):
        _check_ragged_hop(cfg, dict(ds, hop_length=hop))
    _check_ragged_hop(dict(cases.WAVENET_COND_CASES["wn_cond_tiny"][0]), dict(ds, hop_length=200))
    # the other checks of the key hold for SaShiMi as they do for WaveNet
    with pytest.raises(ValueError, match="mel-conditional"):
        generate(None, diff, dict(cases.SASHIMI_CASES["ss_tiny"][0]), dict(ds, hop_length=256), mel_names=["a"], **kw)
    with pytest.raises(ValueError, match="exclude"):
        generate(None, diff, cfg, dict(ds, hop_length=256), mel_names=["a"], mel_name="a", **kw)

"""CPU: the PQMF filter bank of multi-band runs (``diffwave_sashimi_amd/pqmf.py``): the design against the float64
restatement, the near-perfect reconstruction of the restatement (and that the check tells a wrong cutoff), and every
argument error of the bank, of ``training_loss(pqmf=)`` and of the ``model.subbands`` keys before anything is built."""
import numpy as np
import pytest
import torch

from diffwave_sashimi_amd import pqmf
from diffwave_sashimi_amd.pqmf import PQMF
from tests import pqmf_reference as ref


@pytest.mark.parametrize("K,taps,cutoff,beta", [(4, 62, None, 9.0), (2, 62, None, 9.0), (4, 6, 0.2, 5.0), (2, 254, 0.3, 12.0)])
def test_design_equals_the_restatement(K, taps, cutoff, beta):
    ha, hs = pqmf.design(K, taps, cutoff, beta)
    c = pqmf.DEFAULT_CUTOFF[K] if cutoff is None else cutoff
    ra, rs = ref.design(K, taps, c, beta)
    assert ha.dtype == np.float64 and ha.shape == hs.shape == (K, taps + 1)
    # two float64 evaluations of one formula (vectorised and looped): a few ulps of values below 1
    assert np.abs(ha - ra).max() <= 1e-15 and np.abs(hs - rs).max() <= 1e-15
    h = pqmf.prototype(taps, c, beta)
    assert abs(h.sum() - 1.0) <= 1e-15 and np.array_equal(h, h[::-1])
    # the synthesis filters are the analysis filters reversed in time (cos is even, the phases are opposite)
    assert np.abs(hs - ha[:, ::-1]).max() <= 1e-15


def test_defaults():
    assert pqmf.DEFAULT_CUTOFF == {4: 0.142, 2: 0.267}
    assert PQMF().options() == dict(subbands=4, taps=62, cutoff=0.142, beta=9.0)
    assert PQMF(2).options() == dict(subbands=2, taps=62, cutoff=0.267, beta=9.0)
    assert PQMF(subbands=2, taps=6, cutoff=0.25, beta=4).options() == dict(subbands=2, taps=6, cutoff=0.25, beta=4.0)
    from diffwave_sashimi_amd import _lib
    assert _lib.load().dws_pqmf_tile() == pqmf.TILE


def test_float64_round_trip_and_a_wrong_cutoff():
    e4 = ref.round_trip_error(4, 0.142)
    e2 = ref.round_trip_error(2, 0.267)
    wrong = ref.round_trip_error(4, 0.141)
    print(f"round trip: K=4 {e4:.3e}  K=2 {e2:.3e}  K=4 at cutoff 0.141 {wrong:.3e}")
    assert e4 <= 1e-3 and e2 <= 1e-3
    assert wrong > 5e-3                      # the check tells a mistyped constant


def test_restatement_transposes_are_the_other_bank_with_the_reversed_table():
    rng = np.random.default_rng(5)
    for K in (2, 4):
        ha, hs = pqmf.design(K, 6)
        x, w = rng.standard_normal((2, 8 * K)), rng.standard_normal((2, K, 8))
        assert np.abs(ref.analysis_transpose(w, ha)[0] - ref.synthesis(w, ha[:, ::-1])[0]).max() <= 1e-14
        assert np.abs(ref.synthesis_transpose(x, hs, K, float(K))[0] - ref.analysis(x, hs[:, ::-1], float(K))[0]).max() <= 1e-14


def test_bank_argument_errors_in_their_order():
    for kw in (dict(subbands=3), dict(subbands=8), dict(subbands=1), dict(subbands="4"), dict(subbands=True),
               dict(taps=61), dict(taps=0), dict(taps=256), dict(taps=62.0), dict(cutoff=0.0), dict(cutoff=1.0),
               dict(cutoff="x"), dict(beta=-1.0), dict(beta=float("nan"))):
        with pytest.raises(ValueError, match="subbands|taps|cutoff|beta"):
            PQMF(**kw)
    P = PQMF(4)
    x = torch.zeros(2, 1, 64)
    for bad in (x[0, 0], x.expand(2, 2, 64), x.to(torch.int32), x[..., :62], x[..., :0], "x"):
        with pytest.raises(ValueError, match="PQMF.analysis"):
            P.analysis(bad)
    s = torch.zeros(2, 4, 16)
    for bad in (s[0], s[:, :2], s.to(torch.int64), s[..., :0], PQMF(2).analysis):
        with pytest.raises(ValueError, match="PQMF.synthesis"):
            P.synthesis(bad)
    # good arguments on the CPU: the device error is what is left (there is no CPU path)
    with pytest.raises(RuntimeError, match="GPU only"):
        P.analysis(x)
    with pytest.raises(RuntimeError, match="GPU only"):
        P.analysis(x[:, 0])
    with pytest.raises(RuntimeError, match="GPU only"):
        P.synthesis(s)


class _Never(torch.nn.Module):
    def forward(self, *a, **k):
        raise AssertionError("the network ran before the arguments were checked")


def test_training_loss_argument_errors():
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    mse = torch.nn.MSELoss()
    audio = torch.zeros(2, 1, 256)
    gen = torch.Generator().manual_seed(1)
    state = gen.get_state()
    P = PQMF(4)
    with pytest.raises(ValueError, match="prior_std"):
        training_loss(_Never(), mse, audio, dh, generator=gen, pqmf=P, prior_std=torch.ones(2, 1, 256))
    with pytest.raises(ValueError, match="pqmf"):
        training_loss(_Never(), mse, audio.expand(2, 4, 256), dh, generator=gen, pqmf=P)      # sub-bands handed in
    with pytest.raises(ValueError, match="multiple of subbands"):
        training_loss(_Never(), mse, audio[..., :254], dh, generator=gen, pqmf=P)
    with pytest.raises(ValueError, match="clip 0 has 256 samples"):        # the full-band length counts for the STFT
        training_loss(_Never(), mse, audio, dh, generator=gen, pqmf=P, stft_weight=0.5)
    assert torch.equal(gen.get_state(), state)
    with pytest.raises(RuntimeError, match="GPU only"):
        training_loss(_Never(), mse, audio, dh, generator=gen, pqmf=P)
    assert torch.equal(gen.get_state(), state)          # nothing was drawn


class NeverBuilt(dict):        # a model config that fails the test if anything reads past the checked keys
    def __getitem__(self, k):
        raise AssertionError(f"read model.{k} before the subband keys were checked")


WN = dict(_name_="wavenet", unconditional=False, mel_upsample=[8, 8])
DS = dict(hop_length=256, segment_length=1024)


def test_model_keys():
    assert pqmf.model_options({}) is None
    assert pqmf.model_options(dict(subbands=4)) == dict(subbands=4, taps=62, cutoff=0.142, beta=9.0)
    assert pqmf.model_options(dict(subbands=2, pqmf_taps=30, pqmf_cutoff=0.3, pqmf_beta=8, in_channels=2, out_channels=2)) == \
        dict(subbands=2, taps=30, cutoff=0.3, beta=8.0)
    for bad, key in ((dict(subbands=3), "subbands"), (dict(subbands=0), "subbands"), (dict(pqmf_taps=30), "pqmf_taps"),
                     (dict(subbands=4, pqmf_taps=31), "taps"), (dict(subbands=4, in_channels=1), "in_channels"),
                     (dict(subbands=4, in_channels=4, out_channels=2), "out_channels")):
        with pytest.raises(ValueError, match=key):
            pqmf.model_options(bad)
    cfg = dict(WN, subbands=4, pqmf_taps=30, res_channels=16)
    assert pqmf.network_config(cfg) == dict(WN, res_channels=16, in_channels=4, out_channels=4)
    assert pqmf.network_config(dict(WN, res_channels=16)) == dict(WN, res_channels=16)
    assert pqmf.network_config(dict(_name_="sashimi", L=1024, subbands=4))["L"] == 256
    # the run checks: each names its key
    assert pqmf.check_run(dict(WN), DS) is None
    assert pqmf.check_run(dict(WN, subbands=4), DS)["subbands"] == 4
    for model, data, key in ((dict(WN, subbands=4, mel_upsample=[16, 16]), DS, "mel_upsample"),
                             (dict(WN, subbands=4), dict(DS, segment_length=1022), "segment_length"),
                             (dict(WN, subbands=4, unconditional=True), dict(segment_length=15), "segment_length"),
                             (dict(_name_="sashimi", unconditional=True, subbands=4, pool=[4, 4]), dict(segment_length=1056),
                              "pool"),
                             (dict(_name_="sashimi", unconditional=True, subbands=2, pool=[4, 4], L=1000), {}, "model.L")):
        with pytest.raises(ValueError, match=key):
            pqmf.check_run(model, data)
    assert pqmf.check_run(dict(_name_="sashimi", unconditional=True, subbands=4, pool=[4, 4], L=1024),
                          dict(segment_length=1024))["subbands"] == 4
    # checkpoints: the entry against the keys
    entry = PQMF(4).options()
    assert pqmf.resolve({}, None) is None and pqmf.resolve({}, entry) == entry
    assert pqmf.resolve(dict(subbands=4, pqmf_taps=62), entry) == entry
    for model, e in ((dict(subbands=2), entry), (dict(subbands=4, pqmf_taps=30), entry), (dict(subbands=4), None),
                     (dict(subbands=4, pqmf_cutoff=0.15), entry), ({}, dict(subbands=4))):
        with pytest.raises(ValueError, match="checkpoint"):
            pqmf.resolve(model, e)
    assert pqmf.same_options(None, None) and pqmf.same_options(entry, dict(entry)) and not pqmf.same_options(entry, None)
    assert not pqmf.same_options(entry, dict(entry, taps=30))


def test_the_keys_travel_through_the_config_loader(tmp_path):
    from diffwave_sashimi_amd.generate import load_config
    from tests.test_generate_cli import _tree
    cfg = load_config(_tree(tmp_path), ["experiment=lj", "model=wavenet", "+model.subbands=4", "+model.pqmf_cutoff=0.15",
                                        "model.mel_upsample=[8,8]"])
    assert cfg["model"]["subbands"] == 4 and cfg["model"]["pqmf_cutoff"] == 0.15
    assert pqmf.check_run(cfg["model"], cfg["dataset"]) == dict(subbands=4, taps=62, cutoff=0.15, beta=9.0)
    net_cfg = pqmf.network_config(cfg["model"])
    assert net_cfg["in_channels"] == net_cfg["out_channels"] == 4 and "subbands" not in net_cfg and "pqmf_cutoff" not in net_cfg


def test_train_and_generate_refuse_before_a_model_is_built():
    from diffwave_sashimi_amd.generate import generate
    from diffwave_sashimi_amd.train import train
    tr = dict(diffusion_cfg=dict(T=50, beta_0=1e-4, beta_T=0.05), generate_cfg={}, ckpt_iter=-1, n_iters=1,
              iters_per_ckpt=1, iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=2)
    for model, data, kw, key in ((dict(subbands=3), DS, {}, "subbands"),
                                 (dict(WN, subbands=4, mel_upsample=[16, 16]), DS, {}, "mel_upsample"),
                                 (dict(WN, subbands=4), dict(DS, segment_length=1022), {}, "segment_length"),
                                 (dict(WN, subbands=4, in_channels=1), DS, {}, "in_channels"),
                                 (dict(WN, pqmf_taps=30), DS, {}, "pqmf_taps"),
                                 (dict(WN, subbands=4), DS, dict(prior="energy", prior_energy_max=3.0), "train.prior"),
                                 (dict(WN, in_channels=2), DS, dict(stft_weight=0.1), "in_channels")):
        with pytest.raises(ValueError, match=key):
            train(0, 1, model_cfg=NeverBuilt(model), dataset_cfg=data, **tr, **kw)
    diff = dict(T=4, beta_0=1e-4, beta_T=0.05, beta=None)
    for kw, key in ((dict(known_name="a", keep=[[0, 4]]), "known_name"), (dict(start_name="a", start_step=2), "start_name"),
                    (dict(known_name="a", keep=[[0, 4]], resample_jump=2, resample_n=2), "known_name"),
                    (dict(guide_name="a", guide_op="declip", guide_scale=1.0), "guide_name"),
                    (dict(guide_op="mel", guide_scale=1.0, mel_name="a"), "guide_op"),
                    (dict(prior="energy", prior_energy_max=3.0, mel_name="a"), "prior")):
        with pytest.raises(ValueError, match="generate." + key + " does not combine with model.subbands"):
            generate(0, diff, NeverBuilt(dict(WN, subbands=4)), DS, ckpt_iter="init", **kw)
    with pytest.raises(ValueError, match="mel_upsample"):
        generate(0, diff, NeverBuilt(dict(WN, subbands=2)), DS, ckpt_iter="init")
    with pytest.raises(ValueError, match="subbands"):
        generate(0, diff, NeverBuilt(dict(WN, subbands=5)), DS, ckpt_iter="init")

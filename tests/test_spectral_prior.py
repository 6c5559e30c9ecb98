"""CPU: the filter design of the spectral prior (``mel.minimum_phase_filter``, the pure part of
``TacotronSTFT.spectral_filter``) against its numpy restatement (tests/tvfilter_reference.py), its refusals, and the CLI
keys of ``prior=spectral`` (``prior_settings`` / ``resolve_prior`` / ``same_prior``).

Tolerance of the design: both sides run in float64 and the result is rounded to complex64 once, so the two differ by that
rounding, 2^-24 relative per part, plus float64 noise: 1e-7 relative to |F|."""
import numpy as np
import pytest
import torch

from tests import tvfilter_reference as tvr

ROUNDING = 1e-7


def _magnitudes(B=2, K=33, frames=5, seed=0):
    """Positive magnitudes with a spectral tilt, a few bins below the floor and one exactly 0."""
    rng = np.random.RandomState(seed)
    m = np.exp(rng.standard_normal((B, K, frames)) - 0.08 * np.arange(K)[None, :, None])
    m[0, 3, 1] = 0.0
    m[1, 7:9, 2] = 1e-9
    return m.astype(np.float32)


@pytest.mark.parametrize("K,lifter", [(33, 1), (33, 8), (33, 31), (513, 24)])
def test_design_against_numpy(K, lifter):
    from diffwave_sashimi_amd import mel
    m = _magnitudes(K=K)
    ref = float(m.max())
    F = mel.minimum_phase_filter(torch.from_numpy(m), 6, ref=ref, floor=0.01, lifter=lifter)
    assert F.dtype == torch.complex64 and tuple(F.shape) == (2, K, 6) and F.is_contiguous()
    want = tvr.design64(m, 6, ref, 0.01, lifter)
    assert np.abs(F.numpy() - want).max() <= ROUNDING * np.abs(want).max()
    # |F|^2 is the liftered envelope (frames 0 .. 4; frame 5 repeats frame 4)
    env = tvr.liftered_envelope64(m, ref, 0.01, lifter)
    got = np.abs(F.numpy().astype(np.complex128)[:, :, :5]) ** 2
    assert np.abs(got / env - 1.0).max() <= 4 * ROUNDING
    # exactly real at DC and Nyquist
    assert not bool(F.imag[:, 0].any()) and not bool(F.imag[:, -1].any())
    # the inverse filter is 1 / F, finite by the floor
    inv = 1.0 / F
    assert bool(torch.isfinite(torch.view_as_real(inv)).all())
    assert float((F * inv - 1.0).abs().max()) <= 4 * ROUNDING


def test_gain_one_at_ref_and_floor():
    """A flat spectrum at ``ref`` is the filter 1; one below the floor is the filter ``floor`` (real, flat)."""
    from diffwave_sashimi_amd import mel
    flat = torch.full((1, 33, 3), 0.7)
    F = mel.minimum_phase_filter(flat, ref=0.7, lifter=4)
    assert torch.allclose(F, torch.ones_like(F), atol=1e-6)
    F = mel.minimum_phase_filter(flat * 1e-6, ref=0.7, floor=0.05, lifter=4)
    assert torch.allclose(F, torch.full_like(F, 0.05), atol=1e-7)


def test_frame_repeat_rule():
    """Frame f of the filter comes from frame min(f, frames - 1) of the magnitudes; each frame stands on its own."""
    from diffwave_sashimi_amd import mel
    m = torch.from_numpy(_magnitudes(frames=4))
    F = mel.minimum_phase_filter(m, 7, ref=2.0)
    assert tuple(F.shape) == (2, 33, 7)
    for f in range(4, 7):
        assert torch.equal(F[:, :, f], F[:, :, 3])
    assert torch.equal(mel.minimum_phase_filter(m, ref=2.0), F[:, :, :4])
    assert torch.equal(mel.minimum_phase_filter(m, 2, ref=2.0), F[:, :, :2])
    assert torch.equal(mel.minimum_phase_filter(m[1:, :, 2:3], 1, ref=2.0), F[1:, :, 2:3])


def test_design_refusals():
    from diffwave_sashimi_amd import mel
    m = torch.from_numpy(_magnitudes())            # n_fft = 64: lifter in 1 .. 31
    for lifter in (0, 32, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="lifter"):
            mel.minimum_phase_filter(m, ref=1.0, lifter=lifter)
    for floor in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="floor"):
            mel.minimum_phase_filter(m, ref=1.0, floor=floor)
    for ref in (0.0, -1.0, float("inf"), float("nan"), "loud", None):
        with pytest.raises(ValueError, match="ref"):
            mel.minimum_phase_filter(m, ref=ref)
    with pytest.raises(TypeError):
        mel.minimum_phase_filter(m)                 # ref is required: no default is chosen
    with pytest.raises(ValueError, match="frames"):
        mel.minimum_phase_filter(m, 0, ref=1.0)
    with pytest.raises(ValueError, match="magnitudes"):
        mel.minimum_phase_filter(m[0], ref=1.0)
    # the method's own checks come before the mel is touched
    stft = mel.TacotronSTFT(filter_length=64, hop_length=16, win_length=64, n_mel_channels=8, sampling_rate=8000,
                            mel_fmax=4000.0)
    with pytest.raises(ValueError, match="lifter"):
        stft.spectral_filter(torch.zeros(1, 8, 4), ref=1.0, lifter=32)
    with pytest.raises(TypeError):
        stft.spectral_filter(torch.zeros(1, 8, 4))
    with pytest.raises(ValueError, match="GPU only"):
        stft.spectral_filter(torch.zeros(1, 8, 4), ref=1.0)


def test_training_loss_refusals():
    """The combinations ``training_loss(prior_filter=)`` refuses, before anything is drawn or run."""
    from diffwave_sashimi_amd import mel
    from diffwave_sashimi_amd.training import training_loss
    stft = mel.TacotronSTFT(filter_length=64, hop_length=16, win_length=64, n_mel_channels=8, sampling_rate=8000,
                            mel_fmax=4000.0)
    dh = {"T": 4, "Alpha_bar": torch.linspace(0.9, 0.1, 4)}
    audio, F = torch.zeros(2, 1, 64), torch.ones(2, 33, 5, dtype=torch.complex64)
    state = torch.random.get_rng_state()
    with pytest.raises(ValueError, match="come together"):
        training_loss(None, None, audio, dh, prior_filter=F)
    with pytest.raises(ValueError, match="come together"):
        training_loss(None, None, audio, dh, prior_stft=stft)
    with pytest.raises(ValueError, match="prior_std"):
        training_loss(None, None, audio, dh, prior_filter=F, prior_stft=stft, prior_std=torch.ones(2, 1, 64))
    with pytest.raises(ValueError, match="pqmf"):
        training_loss(None, None, audio, dh, prior_filter=F, prior_stft=stft, pqmf=object())
    with pytest.raises(ValueError, match="one audio channel"):
        training_loss(None, None, torch.zeros(2, 2, 64), dh, prior_filter=F, prior_stft=stft)
    assert torch.equal(torch.random.get_rng_state(), state)


def test_cli_spectral_prior_keys():
    from diffwave_sashimi_amd.generate import (PRIOR_KEYS, SPECTRAL_PRIOR_KEYS, generate, prior_settings, resolve_prior,
                                               same_prior)
    from diffwave_sashimi_amd.train import train
    assert PRIOR_KEYS == ("energy_max", "energy_min", "std_min") and SPECTRAL_PRIOR_KEYS == ("ref", "floor", "lifter")
    full = {"kind": "spectral", "ref": 12.5, "floor": 0.01, "lifter": 24}
    energy = {"kind": "energy", "energy_max": 7.5, "energy_min": 0.0, "std_min": 0.1}
    assert prior_settings("spectral", ref=12.5) == full
    assert prior_settings("spectral", ref=12.5, floor=0.05, lifter=8, n_fft=64) == dict(full, floor=0.05, lifter=8)
    assert prior_settings("energy", 7.5) == energy                       # the energy kind is what it was
    with pytest.raises(ValueError, match="mel-conditional"):
        prior_settings("spectral", unconditional=True, ref=12.5)
    with pytest.raises(ValueError, match="needs generate.prior_ref"):
        prior_settings("spectral")
    with pytest.raises(ValueError, match="needs train.prior=spectral"):
        prior_settings(None, where="train", ref=12.5)
    with pytest.raises(ValueError, match="needs generate.prior=spectral"):
        prior_settings("none", lifter=8)
    with pytest.raises(ValueError, match="needs generate.prior=spectral"):
        prior_settings("energy", 7.5, floor=0.1)
    with pytest.raises(ValueError, match="needs generate.prior=energy"):
        prior_settings("spectral", 7.5, ref=12.5)
    with pytest.raises(ValueError, match="expected energy or none"):
        prior_settings("spectrum", ref=12.5)
    for bad in (dict(ref=0.0), dict(ref=float("nan")), dict(ref=True), dict(ref="1"), dict(ref=1.0, floor=0.0),
                dict(ref=1.0, floor=2.0), dict(ref=1.0, lifter=0), dict(ref=1.0, lifter=1.5),
                dict(ref=1.0, lifter=32, n_fft=64)):
        with pytest.raises(ValueError):
            prior_settings("spectral", **bad)
    # against the checkpoint's entry
    assert resolve_prior(None, full) == full and resolve_prior("none", full) is None
    assert resolve_prior(prior_settings("spectral", ref=12.5), None) == full
    trained = dict(full, lifter=12)
    assert resolve_prior(prior_settings("spectral", ref=12.5), trained, ["ref"]) == trained        # unspoken keys follow it
    with pytest.raises(ValueError, match="contradicts the checkpoint"):
        resolve_prior(prior_settings("spectral", ref=13.0), full, ["ref"])
    with pytest.raises(ValueError, match="contradicts the checkpoint"):
        resolve_prior(prior_settings("spectral", ref=12.5, lifter=24), trained, ["ref", "lifter"])
    with pytest.raises(ValueError, match="contradicts the checkpoint"):
        resolve_prior(prior_settings("energy", 7.5), full, ["energy_max"])       # another kind than the weights'
    with pytest.raises(ValueError, match="contradicts the checkpoint"):
        resolve_prior(prior_settings("spectral", ref=12.5), energy, ["ref"])
    with pytest.raises(ValueError, match="not one this version writes"):
        resolve_prior(None, {"kind": "spectral", "ref": 12.5})
    assert same_prior(full, dict(full)) and same_prior(full, dict(full, lifter=24.0))
    assert not same_prior(full, trained) and not same_prior(full, None) and not same_prior(None, full)
    assert not same_prior(full, energy) and not same_prior(energy, full)
    # an entry that carries both kinds' keys still compares by its own kind
    both = {**energy, **full}
    assert not same_prior(dict(both, kind="energy"), dict(both, kind="spectral"))

    # the entry points themselves, before a model is built (no GPU here: building one would fail otherwise)
    from tests import cases
    uncond = dict(cases.WAVENET_CASES["wn_tiny"][0])
    cond = dict(cases.WAVENET_COND_CASES["wn_cond_tiny"][0])
    diff = dict(T=4, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="ljspeech", data_path="/nonexistent", segment_length=512, sampling_rate=22050, hop_length=256)
    with pytest.raises(ValueError, match="mel-conditional"):
        generate(0, diff, uncond, ds, ckpt_iter="init", prior="spectral", prior_ref=12.5)
    with pytest.raises(ValueError, match="cfg_scale does not combine"):
        generate(0, diff, dict(cond, n_classes=2), ds, ckpt_iter="init", mel_name="a", prior="spectral", prior_ref=12.5,
                 label=0, cfg_scale=1.0)
    with pytest.raises(ValueError, match="mel_name"):
        generate(0, diff, cond, ds, ckpt_iter="init", prior="spectral", prior_ref=12.5)
    with pytest.raises(ValueError, match="mel_upsample"):
        generate(0, diff, cond, dict(ds, hop_length=300), ckpt_iter="init", mel_name="a", prior="spectral", prior_ref=12.5)
    tr = dict(ckpt_iter=-1, n_iters=1, iters_per_ckpt=1, iters_per_logging=1, learning_rate=1e-3, batch_size_per_gpu=1)
    with pytest.raises(ValueError, match="needs train.prior_ref"):
        train(0, 1, diff, cond, ds, {}, prior="spectral", **tr)
    with pytest.raises(ValueError, match="mel-conditional"):
        train(0, 1, diff, uncond, ds, {}, prior="spectral", prior_ref=12.5, **tr)
    with pytest.raises(ValueError, match="model.subbands"):
        train(0, 1, diff, dict(cond, subbands=2), dict(ds, hop_length=512), {}, prior="spectral", prior_ref=12.5, **tr)
    with pytest.raises(ValueError, match="lifter"):
        train(0, 1, diff, cond, dict(ds, filter_length=64), {}, prior="spectral", prior_ref=12.5, prior_lifter=32, **tr)

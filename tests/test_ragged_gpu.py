"""GPU: ragged batches on the WaveNet backbone (``net(..., lengths=...)``, dws_model_set_lengths).

Contract under test: over ``[0, len_b)`` clip b of a padded batch is what the network gives for that clip alone at
``L = len_b`` (the CPU oracle at the clip's own length is the reference), nothing stored in the padding reaches a valid
position, and the returned padding is exactly zero.  The zero-padded, unmasked forward misses the bound on every short
clip by one to two orders of magnitude (asserted too: the shapes can see the defect)."""
import pytest
import torch

from oracle import wavenet as own
from tests import cases
from tests.conftest import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

# case -> (L_max, lengths): the full clip, an odd length on the dword path, exactly one 64-position tile, a clip shorter
# than most dilations
BATCHES = {"wn_c64": (600, [600, 333, 64, 5]), "wn_tiny": (300, [300, 131, 7]), "wn_h256_d36": (600, [600, 333])}

# (case, options, bound): the bound is the one the existing own-length test of that path asserts
PATHS = [
    ("wn_tiny", {}, REL_TOL),                                          # generic kernels
    ("wn_c64", {}, REL_TOL),                                           # the f32 default
    ("wn_c64", {"conv_algo": "winograd"}, REL_TOL / 10),
    ("wn_c64", {"conv_algo": "direct"}, REL_TOL),
    ("wn_c64", {"precision": "bf16x3"}, REL_TOL / 10),
    ("wn_c64", {"precision": "bf16x6"}, REL_TOL / 100),
    ("wn_c64", {"precision": "f16x3"}, REL_TOL / 100),
    ("wn_h256_d36", {"precision": "bf16x6", "bx6_mfma": "32x32x16"}, REL_TOL / 100),
    ("wn_h256_d36", {"precision": "bf16x6", "bx6_mfma": "16x16x32"}, REL_TOL / 100),
]


def _ids(v):
    """Test id of an options dict: its values, or "default"."""
    return ("-".join(v.values()) or "default") if isinstance(v, dict) else None


def _setup(name, gpu):
    """net (weights wseed + 5), inputs random INCLUDING the padding, and the oracle's output per clip at its own length
    (computed once per session, shared by the tests below, never modified)."""
    cfg, _, _, wseed, iseed, _ = cases.WAVENET_CASES[name]
    L, lens = BATCHES[name]
    net = cases.build_ours(cfg, wseed + 5).to(gpu)
    audio, steps = cases.wavenet_inputs(len(lens), L, 1, iseed)

    def make():
        sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        with torch.no_grad():
            return [own.wavenet_forward(sd, cfg, audio[b:b + 1, :, :n], steps[b:b + 1]) for b, n in enumerate(lens)]
    return net, audio, steps, L, lens, cases.cached(("ragged_ref", name), make)


def _options(net, opts):
    for k, v in opts.items():
        net.set_option(k, v)


@pytest.mark.parametrize("name,opts,tol", PATHS, ids=_ids)
def test_clip_of_a_ragged_batch_matches_the_oracle_at_its_own_length(gpu, name, opts, tol):
    net, audio, steps, L, lens, refs = _setup(name, gpu)
    _options(net, opts)
    with torch.no_grad():
        plain = net((audio.to(gpu), steps.to(gpu)))
        got = net((audio.to(gpu), steps.to(gpu)), lengths=lens)
    for b, n in enumerate(lens):
        e_plain, e = rel_err(plain[b:b + 1, :, :n], refs[b]), rel_err(got[b:b + 1, :, :n], refs[b])
        print(f"{name} {opts} clip {b} len {n}: padded unmasked {e_plain:.3e}, with lengths {e:.3e} (bound {tol:.1e})")
        if n < L:       # the defect the feature removes is visible at these shapes
            assert e_plain > REL_TOL, (name, b, n, e_plain)
        assert e < tol, (name, opts, b, n, e)
        assert torch.count_nonzero(got[b, :, n:]) == 0


@pytest.mark.parametrize("name,opts", [("wn_tiny", {}), ("wn_c64", {}), ("wn_c64", {"conv_algo": "direct"}),
                                       ("wn_c64", {"precision": "bf16x3"}), ("wn_c64", {"precision": "bf16x6"})],
                         ids=_ids)
def test_nothing_in_the_padding_reaches_a_valid_position(gpu, name, opts):
    net, audio, steps, L, lens, _ = _setup(name, gpu)
    _options(net, opts)
    zeros, nans = audio.clone(), audio.clone()
    for b, n in enumerate(lens):
        zeros[b, :, n:] = 0.0
        nans[b, :, n:] = float("nan")
    with torch.no_grad():
        a = net((zeros.to(gpu), steps.to(gpu)), lengths=lens)
        c = net((nans.to(gpu), steps.to(gpu)), lengths=lens)
        r = net((audio.to(gpu), steps.to(gpu)), lengths=lens)
    for b, n in enumerate(lens):
        assert torch.equal(a[b, :, :n], c[b, :, :n]) and torch.equal(a[b, :, :n], r[b, :, :n]), (name, b)
    for out in (a, c, r):
        assert not torch.isnan(out).any()
        for b, n in enumerate(lens):
            assert torch.count_nonzero(out[b, :, n:]) == 0


@pytest.mark.parametrize("opts", [{}, {"precision": "bf16x6"}], ids=["f32", "bf16x6"])
def test_clip_does_not_depend_on_the_batch_around_it(gpu, opts):
    """Clip b of the ragged batch is bit-equal to the B = 1 call at the same L_max with lengths=[len_b], also when the
    batch is permuted.  Bit equality with the UNPADDED run at L = len_b is not part of the contract (L selects kernels and
    sets the in-range indicators of the Winograd correction rows): it is measured and printed."""
    net, audio, steps, L, lens, _ = _setup("wn_c64", gpu)
    _options(net, opts)
    perm = [2, 0, 3, 1]
    with torch.no_grad():
        got = net((audio.to(gpu), steps.to(gpu)), lengths=lens)
        gotp = net((audio[perm].to(gpu), steps[perm].to(gpu)), lengths=[lens[p] for p in perm])
        for b, n in enumerate(lens):
            one = net((audio[b:b + 1].to(gpu), steps[b:b + 1].to(gpu)), lengths=[n])
            assert torch.equal(got[b], one[0]), (opts, b)
            assert torch.equal(gotp[perm.index(b)], one[0]), (opts, b)
            own_len = net((audio[b:b + 1, :, :n].contiguous().to(gpu), steps[b:b + 1].to(gpu)))
            print(f"{opts} clip {b} len {n}: bit-equal to the unpadded run at L = len: "
                  f"{torch.equal(own_len[0], one[0, :, :n])} (rel diff {rel_err(one[:, :, :n], own_len):.2e})")


def test_full_lengths_and_no_lengths_are_the_same_bits(gpu):
    net, audio, steps, L, lens, _ = _setup("wn_c64", gpu)
    x, t = audio.to(gpu), steps.to(gpu)
    with torch.no_grad():
        plain = net((x, t))
        full = net((x, t), lengths=[L] * len(lens))
        short = net((x, t), lengths=lens)
        again = net((x, t))
        full_t = net((x, t), lengths=torch.tensor([L] * len(lens), device=gpu))
    assert torch.equal(plain, full) and torch.equal(plain, full_t)
    assert not torch.equal(plain, short)
    assert torch.equal(plain, again)            # removing the lengths restores the old bits


COND = [("wn_cond_tiny", {}, REL_TOL), ("wn_cond_c64", {}, REL_TOL), ("wn_cond_c64", {"precision": "bf16x6"}, REL_TOL / 100)]


@pytest.mark.parametrize("lens", [[768, 512, 256], [768, 500, 130]], ids=["whole-frames", "inside-frames"])
@pytest.mark.parametrize("name,opts,tol", COND, ids=_ids)
def test_conditioner_sees_only_the_clips_own_frames(gpu, name, opts, tol, lens):
    cfg, _, _, _, wseed, iseed, _ = cases.WAVENET_COND_CASES[name]
    Tmel, frames, L = 3, [3, 2, 1], 768
    net = cases.build_ours(cfg, wseed + 5).to(gpu)
    _options(net, opts)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    audio, steps = cases.wavenet_inputs(3, L, 1, iseed)
    mel = cases.mel_inputs(3, Tmel, iseed)                       # random in the padded frames too
    C, NL = cfg["res_channels"], cfg["num_res_layers"]

    def make():
        with torch.no_grad():
            return [own.wavenet_forward(sd, cfg, audio[b:b + 1, :, :n], steps[b:b + 1], mel_spec=mel[b:b + 1, :, :frames[b]])
                    for b, n in enumerate(lens)]
    refs = cases.cached(("ragged_cond_ref", name, tuple(lens)), make)
    mel_nan, audio_nan = mel.clone(), audio.clone()
    for b, n in enumerate(lens):
        mel_nan[b, :, frames[b]:] = float("nan")
        audio_nan[b, :, n:] = float("nan")
    with torch.no_grad():
        plain = net((audio.to(gpu), steps.to(gpu)), mel_spec=mel.to(gpu))
        got = net((audio.to(gpu), steps.to(gpu)), mel_spec=mel.to(gpu), lengths=lens, mel_frames=frames)
        melc = net.read_tap("melc", (NL, 3, 2 * C, L)).cpu()
        dflt = net((audio.to(gpu), steps.to(gpu)), mel_spec=mel.to(gpu), lengths=lens)        # frames = ceil(len / hop)
        sealed = net((audio_nan.to(gpu), steps.to(gpu)), mel_spec=mel_nan.to(gpu), lengths=lens, mel_frames=frames)
    assert torch.equal(got, dflt)
    assert not torch.isnan(sealed).any()
    for b, n in enumerate(lens):
        e_plain, e = rel_err(plain[b:b + 1, :, :n], refs[b]), rel_err(got[b:b + 1, :, :n], refs[b])
        print(f"{name} {opts} clip {b} len {n}, {frames[b]} frames: padded unmasked {e_plain:.3e}, with lengths {e:.3e}")
        if n < L:
            assert e_plain > REL_TOL, (name, b, e_plain)
        assert e < tol, (name, opts, b, n, e)
        assert torch.equal(sealed[b, :, :n], got[b, :, :n]), (name, b)
        assert torch.count_nonzero(got[b, :, n:]) == 0 and torch.count_nonzero(sealed[b, :, n:]) == 0
        # function level: the term every layer adds to its gate pre-activations, against the oracle's conditioner on the
        # clip's own frames
        for layer in range(NL):
            p = f"residual_layer.residual_blocks.{layer}"
            with torch.no_grad():
                want = own.wn_conv1d(sd, p + ".mel_conv.conv", own.mel_upsample(sd, p, mel[b:b + 1, :, :frames[b]], n))
            assert rel_err(melc[layer, b:b + 1, :, :n], want) < REL_TOL, (name, b, layer)


def test_bad_lengths_are_refused(gpu):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling, sampling_guided
    net, audio, steps, L, lens, _ = _setup("wn_c64", gpu)
    x, t = audio.to(gpu), steps.to(gpu)
    with torch.no_grad():
        for bad in ([600, 333, 64, 0], [600, 333, 64, L + 1], [600, 333, 64], [600, 333, 64, 5, 5]):
            with pytest.raises(RuntimeError):
                net((x, t), lengths=bad)
        ok = net((x, t), lengths=lens)                       # a refused table leaves the engine usable
        assert torch.count_nonzero(ok[3, :, 5:]) == 0
    with pytest.raises(ValueError):
        net((x, t), lengths=[600.0, 333.0, 64.0, 5.0])
    # a training call
    net.train()
    with pytest.raises(NotImplementedError):
        net((x, t), lengths=lens)
    net.eval()
    with pytest.raises(NotImplementedError):
        net((x.clone().requires_grad_(True), t), lengths=lens)
    # samplers: classifier-free guidance and guided runs
    dh = calc_diffusion_hyperparams(4, 1e-4, 0.05)
    with pytest.raises(ValueError, match="cfg_scale"):
        sampling(net, (4, 1, L), dh, lengths=lens, labels=[0, 0, 0, 0], cfg_scale=1.0)
    with pytest.raises(ValueError, match="lengths"):
        sampling_guided(net, (4, 1, L), dh, measurement=x, operator=lambda v: v, scale=1.0, lengths=lens)
    # conditional model: frames that do not cover the clip, a shared mel
    cfg, _, _, _, wseed, iseed, _ = cases.WAVENET_COND_CASES["wn_cond_tiny"]
    cnet = cases.build_ours(cfg, wseed).to(gpu)
    a3, s3 = cases.wavenet_inputs(3, 768, 1, iseed)
    mel = cases.mel_inputs(3, 3, iseed).to(gpu)
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            cnet((a3.to(gpu), s3.to(gpu)), mel_spec=mel, lengths=[768, 512, 300], mel_frames=[3, 2, 1])     # 1 * 256 < 300
        with pytest.raises(RuntimeError):
            cnet((a3.to(gpu), s3.to(gpu)), mel_spec=mel, lengths=[768, 512, 256], mel_frames=[4, 2, 1])     # 4 > Tmel
        with pytest.raises(RuntimeError):
            cnet((a3.to(gpu), s3.to(gpu)), mel_spec=mel[:1], lengths=[768, 512, 256])                       # a shared mel
        assert torch.isfinite(cnet((a3.to(gpu), s3.to(gpu)), mel_spec=mel, lengths=[768, 512, 256])).all()
    # SaShiMi
    scfg, sB, swseed, siseed, _ = cases.SASHIMI_CASES["ss_tiny"]
    snet = cases.build_ours(scfg, swseed).to(gpu)
    sa, ss = cases.wavenet_inputs(sB, scfg["L"], 1, siseed)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        snet((sa.to(gpu), ss.to(gpu)), lengths=[scfg["L"], 100])

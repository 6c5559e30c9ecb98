"""GPU: ragged batches on the SaShiMi backbone (``net(..., lengths=...)``, dws_model_set_lengths).

Contract under test, the one ``tests/test_ragged_gpu.py`` states for WaveNet: over ``[0, len_b)`` clip b of a padded batch is
what the network gives for that clip alone at ``L = len_b`` (the CPU oracle, ``oracle/sashimi.py``, run per clip at the
clip's own length on the state dict taken after ``_setup_C()``, is the reference), nothing stored in the padding reaches a
valid position, and the returned padding is exactly zero.  The S4 convolution is global and bidirectional, so the
zero-padded, unmasked forward misses the bound on every short clip by two orders of magnitude (asserted too)."""
import pytest
import torch

from oracle import sashimi as oss
from oracle import wavenet as own
from tests import cases
from tests.conftest import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

# batch -> (case, run length, lengths).  ss_tiny: generic tails; the stage lengths 7 and 1 of the 112 / 16 sample clips are odd
# valid lengths inside even rows.  ss_knobs: its stage of 125 runs on rocFFT.  ss_d64_short: MFMA tails, fused LayerNorm
# epilogues, the pooling GEMM's epilogue.  ss_tiny at 20000: the segmented convolution -- the second segment of clip 1 holds 16
# samples, that of clips 2 and 3 is wholly padding; the stage of 1250 holds an odd valid length (1025) too.
BATCHES = {
    "ss_tiny": ("ss_tiny", 1024, [1024, 512, 112, 16]),
    "ss_snet": ("ss_snet", 256, [256, 128, 48, 16]),
    "ss_knobs": ("ss_knobs", 250, [250, 128, 2]),
    "ss_d64_short": ("ss_d64_short", 1024, [1024, 528, 16]),
    "ss_tiny_20000": ("ss_tiny", 20000, [20000, 16400, 8000, 16]),
}

# (batch, options, bound): REL_TOL, and under bf16x6 the bound of tests/test_sashimi_bf16x6_gpu.py
PATHS = [
    ("ss_tiny", {}, REL_TOL),
    ("ss_snet", {}, REL_TOL),
    ("ss_knobs", {}, REL_TOL),
    ("ss_d64_short", {"precision": "f32"}, REL_TOL),
    ("ss_d64_short", {"precision": "bf16x6"}, REL_TOL / 100),
    ("ss_tiny_20000", {}, REL_TOL),
]


def _ids(v):
    return ("-".join(v.values()) or "default") if isinstance(v, dict) else None


def _cpu_sd(net):
    """The state dict the oracle runs on: after ``_setup_C()`` (the kernels' ``L`` buffers set), as the engine is given it."""
    net._setup_C()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    assert all(int(v) > 0 for k, v in sd.items() if k.endswith(".kernel.kernel.L"))
    return sd


def _setup(batch, gpu):
    """net (weights wseed + 5), inputs random INCLUDING the padding, and the oracle's output per clip at its own length
    (computed once per session, shared by the tests below, never modified)."""
    name, L, lens = BATCHES[batch]
    cfg, _, wseed, iseed, _ = cases.SASHIMI_CASES[name]
    net = cases.build_ours(cfg, wseed + 5).to(gpu)
    audio, steps = cases.wavenet_inputs(len(lens), L, 1, iseed)

    def make():
        sd = _cpu_sd(net)
        with torch.no_grad():
            return [oss.sashimi_forward(sd, cfg, audio[b:b + 1, :, :n], steps[b:b + 1]) for b, n in enumerate(lens)]
    return net, audio, steps, L, lens, cases.cached(("ss_ragged_ref", batch), make)


def _options(net, opts):
    for k, v in opts.items():
        net.set_option(k, v)


@pytest.mark.parametrize("batch,opts,tol", PATHS, ids=_ids)
def test_clip_of_a_ragged_batch_matches_the_oracle_at_its_own_length(gpu, batch, opts, tol):
    net, audio, steps, L, lens, refs = _setup(batch, gpu)
    _options(net, opts)
    with torch.no_grad():
        plain = net((audio.to(gpu), steps.to(gpu)))
        got = net((audio.to(gpu), steps.to(gpu)), lengths=lens)
    worst = 0.0
    for b, n in enumerate(lens):
        e_plain, e = rel_err(plain[b:b + 1, :, :n], refs[b]), rel_err(got[b:b + 1, :, :n], refs[b])
        print(f"{batch} {opts} clip {b} len {n}: padded unmasked {e_plain:.3e}, with lengths {e:.3e} (bound {tol:.1e})")
        worst = max(worst, e)
        if n < L:       # the defect the feature removes is visible at these shapes
            assert e_plain > REL_TOL, (batch, b, n, e_plain)
        assert torch.count_nonzero(got[b, :, n:]) == 0
    assert worst < tol, (batch, opts, worst)


@pytest.mark.parametrize("fill", [float("nan"), 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("batch,opts", [("ss_tiny", {}), ("ss_knobs", {}), ("ss_d64_short", {"precision": "f32"}),
                                        ("ss_d64_short", {"precision": "bf16x6"}), ("ss_tiny_20000", {})], ids=_ids)
def test_nothing_in_the_padding_reaches_a_valid_position(gpu, batch, opts, fill):
    net, audio, steps, L, lens, _ = _setup(batch, gpu)
    _options(net, opts)
    zeros, filled = audio.clone(), audio.clone()
    for b, n in enumerate(lens):
        zeros[b, :, n:] = 0.0
        filled[b, :, n:] = fill
    with torch.no_grad():
        a = net((zeros.to(gpu), steps.to(gpu)), lengths=lens)
        c = net((filled.to(gpu), steps.to(gpu)), lengths=lens)
        r = net((audio.to(gpu), steps.to(gpu)), lengths=lens)
    for b, n in enumerate(lens):
        assert torch.equal(a[b, :, :n], c[b, :, :n]) and torch.equal(a[b, :, :n], r[b, :, :n]), (batch, b)
    for out in (a, c, r):
        assert torch.isfinite(out).all()
        for b, n in enumerate(lens):
            assert torch.count_nonzero(out[b, :, n:]) == 0


@pytest.mark.parametrize("batch,opts", [("ss_tiny", {}), ("ss_knobs", {}), ("ss_d64_short", {"precision": "f32"}),
                                        ("ss_d64_short", {"precision": "bf16x6"})], ids=_ids)
def test_clip_does_not_depend_on_the_batch_around_it(gpu, batch, opts):
    """Clip b of the ragged batch is bit-equal to the B = 1 call at the same L with lengths=[len_b], also when the batch is
    permuted."""
    net, audio, steps, L, lens, _ = _setup(batch, gpu)
    _options(net, opts)
    perm = list(range(len(lens)))[::-1]
    perm = perm[1:] + perm[:1]
    with torch.no_grad():
        got = net((audio.to(gpu), steps.to(gpu)), lengths=lens)
        gotp = net((audio[perm].to(gpu), steps[perm].to(gpu)), lengths=[lens[p] for p in perm])
        for b, n in enumerate(lens):
            one = net((audio[b:b + 1].to(gpu), steps[b:b + 1].to(gpu)), lengths=[n])
            assert torch.equal(got[b], one[0]), (opts, b)
            assert torch.equal(gotp[perm.index(b)], one[0]), (opts, b)


@pytest.mark.parametrize("batch", ["ss_tiny", "ss_knobs", "ss_d64_short", "ss_tiny_20000"])
def test_full_lengths_and_no_lengths_are_the_same_bits(gpu, batch):
    net, audio, steps, L, lens, _ = _setup(batch, gpu)
    x, t = audio.to(gpu), steps.to(gpu)
    taps = lambda: (net.read_tap("split_launches", (2,)).tolist(), int(net.read_tap("sampler_graphs", (1,)).item()))
    with torch.no_grad():
        plain = net((x, t))
        before = taps()
        full = net((x, t), lengths=[L] * len(lens))
        assert taps() == before                 # the same tails, nothing captured
        short = net((x, t), lengths=lens)
        again = net((x, t))
        full_t = net((x, t), lengths=torch.tensor([L] * len(lens), device=gpu))
    assert torch.equal(plain, full) and torch.equal(plain, full_t)
    assert not torch.equal(plain, short)
    assert torch.equal(plain, again)            # removing the lengths restores the old bits


def _blocks(cfg):
    """(prefix, H, configured stage length) of every block, in the state dict's naming."""
    out = []
    for group, layers in zip(("d_layers", "c_layers", "u_layers"), oss.layer_plan(cfg)):
        out += [(f"{group}.{i}", lay[1], lay[2]) for i, lay in enumerate(layers) if lay[0] == "block"]
    return out


COND = [("ss_cond_tiny", 512, [512, 256], [2, 1]), ("ss_cond_d32", 1024, [1024, 768, 256], [4, 3, 1])]


@pytest.mark.parametrize("name,L,lens,frames", COND, ids=[c[0] for c in COND])
def test_conditioner_sees_only_the_clips_own_frames(gpu, name, L, lens, frames):
    cfg, _, Tmel, wseed, iseed, _ = cases.SASHIMI_COND_CASES[name]
    assert cfg["L"] == L and Tmel == frames[0]
    net = cases.build_ours(cfg, wseed + 5).to(gpu)
    sd = _cpu_sd(net)
    B = len(lens)
    audio, steps = cases.wavenet_inputs(B, L, 1, iseed)
    mel = cases.mel_inputs(B, Tmel, iseed)                       # a mel per clip, random in the padded frames too

    def make():
        with torch.no_grad():
            return [oss.sashimi_forward(sd, cfg, audio[b:b + 1, :, :n], steps[b:b + 1], mel_spec=mel[b:b + 1, :, :frames[b]])
                    for b, n in enumerate(lens)]
    refs = cases.cached(("ss_ragged_cond_ref", name), make)
    mel_nan, audio_nan = mel.clone(), audio.clone()
    for b, n in enumerate(lens):
        mel_nan[b, :, frames[b]:] = float("nan")
        audio_nan[b, :, n:] = float("nan")
    blocks = _blocks(cfg)
    with torch.no_grad():
        plain = net((audio.to(gpu), steps.to(gpu)), mel_spec=mel.to(gpu))
        got = net((audio.to(gpu), steps.to(gpu)), mel_spec=mel.to(gpu), lengths=lens, mel_frames=frames)
        melc = {p: net.read_tap("melc:" + p, (B, H, Ls)).cpu() for p, H, Ls in blocks}
        dflt = net((audio.to(gpu), steps.to(gpu)), mel_spec=mel.to(gpu), lengths=lens)        # frames = ceil(len / hop)
        sealed = net((audio_nan.to(gpu), steps.to(gpu)), mel_spec=mel_nan.to(gpu), lengths=lens, mel_frames=frames)
    assert torch.equal(got, dflt)
    assert torch.isfinite(sealed).all()
    for b, n in enumerate(lens):
        e_plain, e = rel_err(plain[b:b + 1, :, :n], refs[b]), rel_err(got[b:b + 1, :, :n], refs[b])
        print(f"{name} clip {b} len {n}, {frames[b]} frames: padded unmasked {e_plain:.3e}, with lengths {e:.3e}")
        if n < L:
            assert e_plain > REL_TOL, (name, b, e_plain)
        assert e < REL_TOL, (name, b, n, e)
        assert torch.equal(sealed[b, :, :n], got[b, :, :n]), (name, b)
        assert torch.count_nonzero(got[b, :, n:]) == 0 and torch.count_nonzero(sealed[b, :, n:]) == 0
        # function level: the term every block adds, over the clip's part of the block's stage, against the oracle's
        # conditioner on the clip's own frames
        for p, H, Ls in blocks:
            ns = n // (L // Ls)
            with torch.no_grad():
                want = own.wn_conv1d(sd, p + ".mel_conv.conv", own.mel_upsample(sd, p, mel[b:b + 1, :, :frames[b]], ns))
            assert rel_err(melc[p][b:b + 1, :, :ns], want) < REL_TOL, (name, b, p)


def test_bad_lengths_are_refused(gpu):
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling, sampling_guided
    net, audio, steps, L, lens, _ = _setup("ss_tiny", gpu)
    x, t = audio.to(gpu), steps.to(gpu)
    with torch.no_grad():
        for bad in ([1024, 512, 112, 100], [1024, 512, 112, L + 1], [8, 512, 112, 16]):       # not multiples of 4 * 4
            with pytest.raises(NotImplementedError, match="multiple of 16"):
                net((x, t), lengths=bad)
        for bad in ([1024, 512, 112, 0], [1024, 512, 112, L + 16], [1024, 512, 112], [1024, 512, 112, 16, 16]):
            with pytest.raises(RuntimeError):
                net((x, t), lengths=bad)
        ok = net((x, t), lengths=lens)                       # a refused table leaves the engine usable
        assert torch.count_nonzero(ok[3, :, 16:]) == 0 and torch.isfinite(ok).all()
    # the engine's own check of the rule (the module's comes first on every Python path)
    from diffwave_sashimi_amd import _lib
    import ctypes
    arr = (ctypes.c_int32 * 4)(1024, 512, 112, 100)
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        _lib.check(_lib.load().dws_model_set_lengths(net._handle, arr, None, 4, _lib.current_stream()))
    # a training call, an input gradient
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
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        sampling(net, (4, 1, L), dh, lengths=[1024, 512, 112, 100])
    # conditional model: frames that do not cover the clip, more frames than the mel holds, a shared mel
    cfg, _, Tmel, wseed, iseed, _ = cases.SASHIMI_COND_CASES["ss_cond_d32"]
    cnet = cases.build_ours(cfg, wseed).to(gpu)
    a3, s3 = cases.wavenet_inputs(3, 1024, 1, iseed)
    mel = cases.mel_inputs(3, Tmel, iseed).to(gpu)
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            cnet((a3.to(gpu), s3.to(gpu)), mel_spec=mel, lengths=[1024, 768, 304], mel_frames=[4, 3, 1])     # 1 * 256 < 304
        with pytest.raises(RuntimeError):
            cnet((a3.to(gpu), s3.to(gpu)), mel_spec=mel, lengths=[1024, 768, 256], mel_frames=[5, 3, 1])     # 5 > Tmel
        with pytest.raises(RuntimeError):
            cnet((a3.to(gpu), s3.to(gpu)), mel_spec=mel[:1], lengths=[1024, 768, 256])                       # a shared mel
        assert torch.isfinite(cnet((a3.to(gpu), s3.to(gpu)), mel_spec=mel, lengths=[1024, 768, 256])).all()

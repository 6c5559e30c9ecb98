"""Function-level GPU parity of the mel conditioner (`models/wavenet.py:98-111` ==
`models/sashimi.py:160-175`; `csrc/conditioner_kernels.hip`) at every kind of stride, read out of the engine through the
taps "mel_u0" / "mel_u1" (the two upsampled mels) and "melc" / "melc:<block>" (the term each layer adds), against the
float64 oracle on the same state dict: the two `conv_transpose2d` + `leaky_relu(0.4)` of `oracle.wavenet.mel_upsample`,
then `wn_conv1d(.., ".mel_conv.conv")`.

Metric: `tests.conftest.rel_err` (max-abs over max-abs: an edge column cannot hide in a norm).  Bound 2e-6 for all three
taps: the fp32 oracle's own distance from float64, measured on the CPU over these stride pairs, Tmel in {1, 2, 7},
`build_ours` weights and `cases.mel_inputs`, is at most 2.3e-7 for the upsampled mel and 4.1e-7 for melc; the kernels run the
same fp32 operation count (6 FMAs per upsampled value, an 80-term dot product), 2e-6 is about 5 x the melc figure, and one
wrong tap costs 1e-2 or more.  Every case also measures the fp32 oracle's distance itself and holds it below 1e-6, so the
reference stays inside the bound on its own.

Strides: [16, 16] control; [2, 2] smallest power of two (pad 1); [4, 8] unequal powers of two; [3, 5] odd (`mel_upsample_kernel`,
the kernel behind every hop that is no power of two); [6, 10] even, no power of two; [12, 20] hop 240; [1, 3] s = 1 (kernel
width 2, pad 0)."""
import faulthandler
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import sashimi as oss
from oracle import wavenet as own
from tests import cases
from tests.conftest import REL_TOL, ROOT, rel_err

pytestmark = pytest.mark.gpu

BOUND = 2e-6            # engine vs float64 (see the module docstring)
ORACLE_BOUND = 1e-6     # fp32 oracle vs float64
STRIDES = [[16, 16], [2, 2], [4, 8], [3, 5], [6, 10], [12, 20], [1, 3]]
TMELS = [1, 2, 7]
MB = 80


def up_len(T, s):
    """Width after one ConvTranspose2d(1, 1, (3, 2s), stride (1, s), padding (1, s // 2))."""
    return (T - 1) * s - 2 * (s // 2) + 2 * s


def lengths(Tmel, strides):
    T0 = up_len(Tmel, strides[0])
    return T0, up_len(T0, strides[1])


class _time_limit:
    """A hung GPU call ends the process with a traceback after `seconds` instead of holding the machine (the watchdog thread
    of `faulthandler` fires even while the main thread sits inside a HIP call)."""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        faulthandler.dump_traceback_later(self.seconds, exit=True, file=sys.__stderr__)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def wn_cond_cfg(strides, C=16, layers=2):
    return cases.wn_cfg(unconditional=False, res_channels=C, skip_channels=C, num_res_layers=layers, dilation_cycle=layers,
                        mel_upsample=list(strides))


def ss_cond_cfg(strides, L, d_model=8):
    return cases.ss_cfg(unconditional=False, d_model=d_model, n_layers=1, L=L, pool=[4, 4], mel_upsample=list(strides),
                        diffusion_step_embed_dim_mid=64)


def wn_prefixes(cfg):
    return [f"residual_layer.residual_blocks.{n}" for n in range(cfg["num_res_layers"])]


def ss_blocks(cfg):
    """[(prefix, H, L_stage)] of every DiffWaveBlock in execution order (`sashimi.py:236-268`)."""
    d, c, u = oss.layer_plan(cfg)
    return [(f"{g}_layers.{i}", k[1], k[2]) for g, layers in (("d", d), ("c", c), ("u", u))
            for i, k in enumerate(layers) if k[0] == "block"]


def oracle_conditioner(sd, prefix, mel, L, dtype):
    """(u0, u1, melc) of one layer in `dtype`: the body of `oracle.wavenet.mel_upsample` with both upsampled mels kept
    whole, then its truncation to the first L frames and the 1x1 `mel_conv`."""
    sdd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefix + ".") and v.is_floating_point()}
    m = mel.to(dtype).unsqueeze(1)
    ups = []
    with torch.no_grad():
        for i in range(2):
            p = f"{prefix}.upsample_conv2d.{i}"
            w = own.weight_norm_weight(sdd, p)
            s = w.shape[-1] // 2
            m = F.leaky_relu(F.conv_transpose2d(m, w, sdd[p + ".bias"], stride=(1, s), padding=(1, s // 2)), 0.4)
            ups.append(m.squeeze(1))
        trunc = own.mel_upsample(sdd, prefix, mel.to(dtype), L)
        assert torch.equal(trunc, ups[1][:, :, :L])            # this restatement IS the oracle's function
        melc = own.wn_conv1d(sdd, prefix + ".mel_conv.conv", trunc)
    return ups[0], ups[1], melc


def _cpu_sd(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


class _Worst:
    """Largest engine-vs-float64 and fp32-oracle-vs-float64 error per tap over one test."""

    def __init__(self):
        self.eng, self.orc = {}, {}

    def add(self, tap, got, ref64, ref32):
        assert tuple(got.shape) == tuple(ref64.shape), (tap, got.shape, ref64.shape)
        assert torch.isfinite(got).all(), tap
        self.eng[tap] = max(self.eng.get(tap, 0.0), rel_err(got, ref64))
        self.orc[tap] = max(self.orc.get(tap, 0.0), rel_err(ref32, ref64))

    def check(self, label):
        print(f"{label}: engine vs float64 " + ", ".join(f"{k} {v:.2e}" for k, v in self.eng.items())
              + " | fp32 oracle vs float64 " + ", ".join(f"{k} {v:.2e}" for k, v in self.orc.items()))
        for k in self.eng:
            assert self.orc[k] < ORACLE_BOUND, (label, k, self.orc[k])
            assert self.eng[k] < BOUND, (label, k, self.eng[k])


def _forward(net, gpu, audio, steps, mel):
    with torch.no_grad():
        return net((audio.to(gpu), steps.to(gpu)), mel_spec=mel.to(gpu)).cpu()


def check_wavenet(gpu, strides, Tmel, L, taps=("mel_u0", "mel_u1", "melc"), B=2, mel_batches=(1, 2), wseed=301, iseed=302):
    """One tiny conditional WaveNet (C = S = 16, two layers: generic layer kernels): a no_grad forward per mel batch, then
    the taps.  EVERY layer's slice of melc is compared; mel_u0 / mel_u1 are those of the last layer (shared scratch)."""
    cfg = wn_cond_cfg(strides)
    C, NL = cfg["res_channels"], cfg["num_res_layers"]
    T0, T1 = lengths(Tmel, strides)
    assert T1 >= L >= 1
    net = cases.build_ours(cfg, wseed).to(gpu)
    sd = _cpu_sd(net)
    audio, steps = cases.wavenet_inputs(B, L, 1, iseed)
    w = _Worst()
    for Bm in mel_batches:
        mel = cases.mel_inputs(Bm, Tmel, iseed + Bm)
        out = _forward(net, gpu, audio, steps, mel)
        assert torch.isfinite(out).all()
        melc = net.read_tap("melc", (NL, Bm, 2 * C, L)).cpu() if "melc" in taps else None
        for n, p in enumerate(wn_prefixes(cfg)):
            last = n == NL - 1
            if not (melc is not None or last):
                continue
            r64, r32 = oracle_conditioner(sd, p, mel, L, torch.float64), oracle_conditioner(sd, p, mel, L, torch.float32)
            if melc is not None:
                w.add("melc", melc[n], r64[2], r32[2])
            if last:
                for i, (name, T) in enumerate((("mel_u0", T0), ("mel_u1", T1))):
                    if name in taps:
                        w.add(name, net.read_tap(name, (Bm, MB, T)).cpu(), r64[i], r32[i])
        if Bm == 1 and B > 1:       # the engine keeps ONE copy and broadcasts it: same output as the mel repeated, bit for bit
            assert torch.equal(out, _forward(net, gpu, audio, steps, mel.repeat(B, 1, 1)))
    w.check(f"wavenet strides {strides} Tmel {Tmel} (T0 {T0}, T1 {T1}) L {L}")
    return net


def check_sashimi(gpu, strides, Tmel, L, B=2, wseed=311, iseed=312):
    """One tiny conditional SaShiMi (d_model 8, pool [4, 4]: stages L, L/4, L/16 with H = 8, 16, 32): EVERY block's
    "melc:<prefix>" against the oracle's FIRST L_stage upsampled frames (`sashimi.py:170-172`: a truncation, no downsampling)."""
    cfg = ss_cond_cfg(strides, L)
    T0, T1 = lengths(Tmel, strides)
    assert T1 >= L and L % 16 == 0
    net = cases.build_ours(cfg, wseed).to(gpu)
    audio, steps = cases.wavenet_inputs(B, L, 1, iseed)
    blocks = ss_blocks(cfg)
    assert len(blocks) == 5 and [b[2] for b in blocks] == [L, L // 4, L // 16, L // 4, L]
    w = _Worst()
    for Bm in (1, B):
        mel = cases.mel_inputs(Bm, Tmel, iseed + Bm)
        out = _forward(net, gpu, audio, steps, mel)
        assert torch.isfinite(out).all()
        sd = _cpu_sd(net)
        for j, (p, H, Ls) in enumerate(blocks):
            r64, r32 = oracle_conditioner(sd, p, mel, Ls, torch.float64), oracle_conditioner(sd, p, mel, Ls, torch.float32)
            w.add("melc", net.read_tap("melc:" + p, (Bm, H, Ls)).cpu(), r64[2], r32[2])
            if j == len(blocks) - 1:        # the scratch holds the upsampled mels of the block processed last
                w.add("mel_u0", net.read_tap("mel_u0", (Bm, MB, T0)).cpu(), r64[0], r32[0])
                w.add("mel_u1", net.read_tap("mel_u1", (Bm, MB, T1)).cpu(), r64[1], r32[1])
        if Bm == 1:
            assert torch.equal(out, _forward(net, gpu, audio, steps, mel.repeat(B, 1, 1)))
    w.check(f"sashimi strides {strides} Tmel {Tmel} (T0 {T0}, T1 {T1}) L {L} / {L // 4} / {L // 16}")
    return net


# ------------------------------------------------------------------------------------------------------------------
# forward: WaveNet, every stride pair x Tmel in {1, 2, 7} x L in {T1 (no truncation), T1 - 3 (ragged, where >= 1)}
# ------------------------------------------------------------------------------------------------------------------
def _wn_cases():
    out = []
    for s in STRIDES:
        for Tmel in TMELS:
            T1 = lengths(Tmel, s)[1]
            out.append((s, Tmel, T1))
            if T1 - 3 >= 1:
                out.append((s, Tmel, T1 - 3))
    return out


@pytest.mark.parametrize("strides,Tmel,L", _wn_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_wavenet_conditioner_matches_the_float64_oracle(gpu, strides, Tmel, L):
    check_wavenet(gpu, strides, Tmel, L)


@pytest.mark.parametrize("strides,Tmel", [([16, 16], 9), ([12, 20], 9)], ids=["16x16", "12x20"])
def test_wavenet_conditioner_beyond_one_tile(gpu, strides, Tmel):
    """T1 = 2304 / 2160 > 2048 with L = T1 - 5 (no multiple of 4): three 1024-position tiles of `conv1x1_trunc_kernel`, the last
    one ragged, and three 1024-output blocks of the power-of-two upsampler."""
    T1 = lengths(Tmel, strides)[1]
    assert T1 > 2048 and (T1 - 5) % 4 != 0
    check_wavenet(gpu, strides, Tmel, T1 - 5)


def test_generic_upsampler_grid_stride_loop(gpu):
    """Strides [12, 20], Tmel = 1100: T1 = 264000 > 1024 blocks x 256 threads, the only case that enters the second pass of
    `mel_upsample_kernel`'s grid-stride loop.  All 80 x 264000 values of mel_u1 (84 MB) against the float64 oracle; L = 300."""
    strides, Tmel = [12, 20], 1100
    T0, T1 = lengths(Tmel, strides)
    assert (T0, T1) == (13200, 264000) and T1 > 1024 * 256
    with _time_limit(240):
        check_wavenet(gpu, strides, Tmel, 300, taps=("mel_u0", "mel_u1"), mel_batches=(1,))


# ------------------------------------------------------------------------------------------------------------------
# forward: SaShiMi.  L is a multiple of 16 (pool [4, 4]) and the pooled stages keep at least 13 samples, so Tmel is chosen
# per stride pair: T1 = L (no truncation at the top stage; the pooled stages always truncate) and T1 > L (ragged).
# ------------------------------------------------------------------------------------------------------------------
SS_CASES = [([16, 16], 1, 256), ([16, 16], 2, 496), ([16, 16], 7, 1792),
            ([2, 2], 64, 256), ([2, 2], 65, 256),
            ([4, 8], 7, 224), ([4, 8], 9, 272),
            ([3, 5], 22, 336), ([3, 5], 17, 256),
            ([6, 10], 4, 240), ([6, 10], 5, 288),
            ([12, 20], 1, 240), ([12, 20], 2, 464),
            ([1, 3], 84, 256), ([1, 3], 86, 256)]


@pytest.mark.parametrize("strides,Tmel,L", SS_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_sashimi_conditioner_matches_the_float64_oracle(gpu, strides, Tmel, L):
    check_sashimi(gpu, strides, Tmel, L)


# ------------------------------------------------------------------------------------------------------------------
# the power-of-two kernel against the generic one, bit for bit
# ------------------------------------------------------------------------------------------------------------------
POW2_STRIDES = [[16, 16], [2, 2], [4, 8]]


def pow2_payload(gpu):
    """mel_u1 and melc of seeded models at the power-of-two stride pairs, whichever upsampler this PROCESS runs
    (`DWS_MEL_UPSAMPLE_GENERIC` is read once per process)."""
    out = {}
    for s in POW2_STRIDES:
        tag = "x".join(map(str, s))
        Tmel = 7
        T0, T1 = lengths(Tmel, s)
        cfg = wn_cond_cfg(s)
        L = T1 - 3
        net = cases.build_ours(cfg, 321).to(gpu)
        audio, steps = cases.wavenet_inputs(2, L, 1, 322)
        mel = cases.mel_inputs(2, Tmel, 323)
        _forward(net, gpu, audio, steps, mel)
        out[f"wn/{tag}/mel_u1"] = net.read_tap("mel_u1", (2, MB, T1)).cpu()
        out[f"wn/{tag}/melc"] = net.read_tap("melc", (cfg["num_res_layers"], 2, 2 * cfg["res_channels"], L)).cpu()
        Tm, Ls = {"16x16": (2, 496), "2x2": (65, 256), "4x8": (9, 272)}[tag]
        T0, T1 = lengths(Tm, s)
        cfg = ss_cond_cfg(s, Ls)
        net = cases.build_ours(cfg, 331).to(gpu)
        audio, steps = cases.wavenet_inputs(2, Ls, 1, 332)
        mel = cases.mel_inputs(2, Tm, 333)
        _forward(net, gpu, audio, steps, mel)
        out[f"ss/{tag}/mel_u1"] = net.read_tap("mel_u1", (2, MB, T1)).cpu()
        for p, H, Lb in ss_blocks(cfg):
            out[f"ss/{tag}/melc:{p}"] = net.read_tap("melc:" + p, (2, H, Lb)).cpu()
    return out


_GENERIC_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["DWS_ROOT"])
assert os.environ.get("DWS_MEL_UPSAMPLE_GENERIC") == "1"
import torch
from tests.test_conditioner_gpu import pow2_payload
torch.save(pow2_payload(torch.device("cuda:0")), sys.argv[1])
'''


def test_power_of_two_upsampler_is_bit_identical_to_the_generic_one(tmp_path, gpu):
    """The comment above `mel_upsample_pow2_kernel` claims bit-identical results (same order of additions).  The generic side
    runs in a fresh child process with `DWS_MEL_UPSAMPLE_GENERIC=1` (the switch is read once per process)."""
    assert "DWS_MEL_UPSAMPLE_GENERIC" not in os.environ       # this process runs the power-of-two kernel
    mine = pow2_payload(gpu)
    script, f = tmp_path / "generic_worker.py", tmp_path / "generic.pt"
    script.write_text(_GENERIC_WORKER)
    env = dict(os.environ, DWS_ROOT=ROOT, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""),
               DWS_MEL_UPSAMPLE_GENERIC="1")
    r = subprocess.run([sys.executable, str(script), str(f)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    theirs = torch.load(f)
    assert set(theirs) == set(mine) and len(mine) == 3 * (2 + 1 + 5)
    diff = [k for k in mine if not torch.equal(mine[k], theirs[k])]
    print(f"power-of-two vs generic upsampler: {len(mine) - len(diff)} of {len(mine)} tensors bit-identical")
    assert not diff, {k: float((mine[k] - theirs[k]).abs().max()) for k in diff}


# ------------------------------------------------------------------------------------------------------------------
# refusals of set_condition, both backbones: the engine's message, and the model still runs afterwards
# ------------------------------------------------------------------------------------------------------------------
def _refusal_setup(backbone, gpu, unconditional=False):
    if backbone == "wavenet":
        cfg, L = wn_cond_cfg([2, 2]), 16
        fwd = own.wavenet_forward
    else:
        cfg, L = ss_cond_cfg([2, 2], 256), 256
        fwd = oss.sashimi_forward
    if unconditional:
        cfg = dict(cfg, unconditional=True)
    net = cases.build_ours(cfg, 341).to(gpu)
    audio, steps = cases.wavenet_inputs(2, L, 1, 342)
    good = None if unconditional else cases.mel_inputs(2, L // 4 + 1, 343)      # T1 = 4 Tmel = L + 4

    def still_runs():
        with torch.no_grad():
            out = net((audio.to(gpu), steps.to(gpu)), mel_spec=None if good is None else good.to(gpu)).cpu()
            ref = fwd(_cpu_sd(net), cfg, audio, steps, mel_spec=good)
        assert rel_err(out, ref) < REL_TOL, rel_err(out, ref)

    return net, audio.to(gpu), steps.to(gpu), L, still_runs


@pytest.mark.parametrize("backbone", ["wavenet", "sashimi"])
def test_upsampled_mel_shorter_than_the_audio_is_refused(gpu, backbone):
    net, audio, steps, L, still_runs = _refusal_setup(backbone, gpu)
    short = cases.mel_inputs(2, L // 4 - 1, 344).to(gpu)                          # T1 = L - 4
    with pytest.raises(RuntimeError, match=r"upsampled mel length %d < L=%d" % (L - 4, L)), torch.no_grad():
        net((audio, steps), mel_spec=short)
    still_runs()


@pytest.mark.parametrize("backbone", ["wavenet", "sashimi"])
def test_mel_batch_that_is_neither_one_nor_the_batch_is_refused(gpu, backbone):
    net, audio, steps, L, still_runs = _refusal_setup(backbone, gpu)
    with pytest.raises(RuntimeError, match=r"mel batch 3 must be 1 or B=2"), torch.no_grad():
        net((audio, steps), mel_spec=cases.mel_inputs(3, L // 4 + 1, 345).to(gpu))
    still_runs()


@pytest.mark.parametrize("backbone", ["wavenet", "sashimi"])
def test_mel_on_an_unconditional_model_is_refused(gpu, backbone):
    net, audio, steps, L, still_runs = _refusal_setup(backbone, gpu, unconditional=True)
    with pytest.raises(RuntimeError, match=r"set_condition on an unconditional model"), torch.no_grad():
        net((audio, steps), mel_spec=cases.mel_inputs(2, L // 4 + 1, 346).to(gpu))
    still_runs()


@pytest.mark.parametrize("backbone", ["wavenet", "sashimi"])
def test_conditioner_taps_need_an_installed_mel(gpu, backbone):
    net, audio, steps, L, still_runs = _refusal_setup(backbone, gpu)
    with torch.no_grad():
        net((audio, steps), mel_spec=None)      # a conditional model runs without a mel (`wavenet.py:99`): nothing installed
    names = ["mel_u0", "mel_u1", "melc" if backbone == "wavenet" else "melc:c_layers.0"]
    for name in names:
        with pytest.raises(RuntimeError, match=r"libdws error -4: tap '%s' before a set_condition with a mel" % name):
            net.read_tap(name, (1 << 20,))
    still_runs()
    with pytest.raises(RuntimeError, match="capacity 1"):      # installed now: a buffer that is too small is refused
        net.read_tap(names[-1], (1,))
    with torch.no_grad():                  # the mel taken away again (an unconditional call): the taps close
        net((audio, steps), mel_spec=None)
    with pytest.raises(RuntimeError, match="libdws error -4"):
        net.read_tap("mel_u1", (1 << 20,))


# ------------------------------------------------------------------------------------------------------------------
# re-conditioning one model: buffer growth (`DevBuf::ensure`) and the module's mel cache (`_mel_key`)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone", ["wavenet", "sashimi"])
def test_reconditioning_equals_a_fresh_model(gpu, backbone):
    """Tmel = 7, then a fresh tensor with Tmel = 2, then the first tensor modified in place (same address and shape, a new
    version counter): after each, melc is bit for bit that of a fresh model given the same mel."""
    if backbone == "wavenet":
        strides, L = [3, 5], 30                      # T1 = 111 and 36
        cfg = wn_cond_cfg(strides)
        read = lambda net, Bm: [net.read_tap("melc", (cfg["num_res_layers"], Bm, 2 * cfg["res_channels"], L)).cpu()]
    else:
        strides, L = [16, 16], 256                   # T1 = 1792 and 512
        cfg = ss_cond_cfg(strides, L)
        read = lambda net, Bm: [net.read_tap("melc:" + p, (Bm, H, Ls)).cpu() for p, H, Ls in ss_blocks(cfg)]
    audio, steps = cases.wavenet_inputs(2, L, 1, 352)
    audio, steps = audio.to(gpu), steps.to(gpu)

    def melc_of(net, mel):
        with torch.no_grad():
            net((audio, steps), mel_spec=mel)
        return read(net, mel.shape[0])

    net = cases.build_ours(cfg, 351).to(gpu)
    mel7 = cases.mel_inputs(2, 7, 353).to(gpu)
    mel2 = cases.mel_inputs(2, 2, 354).to(gpu)
    seen = []
    for step in ("Tmel 7", "Tmel 2", "Tmel 7 modified in place"):
        if step == "Tmel 2":
            mel = mel2
        else:
            mel = mel7
            if step != "Tmel 7":
                ptr = mel7.data_ptr()
                mel7.mul_(0.5).add_(-1.0)
                assert mel7.data_ptr() == ptr
        got = melc_of(net, mel)
        fresh = melc_of(cases.build_ours(cfg, 351).to(gpu), mel.clone())
        assert all(torch.equal(a, b) for a, b in zip(got, fresh)), step
        seen.append(got)
    assert not torch.equal(seen[0][0], seen[2][0])          # the in-place change reached the engine

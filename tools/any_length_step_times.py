"""Device-event times of the data-only pair (dws_model_forward_input + dws_model_backward_input(param_grads=0)) of a SaShiMi
model at a run length other than its kernels' own, on one GPU: the segmented convolution pair against the rocFFT route.

    python tools/any_length_step_times.py [--config unet_d32_n6_T50_cond] [--batch 2] [--length 212992] [--repeats 5]
                                          [--steps 4] [--rounds 2] [--out FILE]

Without `--leg` the script is the driver: it starts one child process per variant -- "segmented" (the default routes) and
"rocfft" (DWS_SASHIMI_ROCFFT=1, read at model setup: every stage on rocFFT) -- alternating `--rounds` times, and writes
every leg's JSON line to `--out`.  A leg, each figure the median [min, max] of `--repeats` after a warm-up, device events:
  forward_input        the training forward of the data-only pair
  backward_data_only   dws_model_backward_input(param_grads=0, daudio)
  pair                 both, back to back
  seg_train / seg_adjoint / long_stage_fwd / long_stage_bwd   launches and summed device time of those kernels in ONE pair
                       (the engine's launch profile; the profile's events serialise nothing, each launch is timed alone)
  guided_step          sampling_guided (DDIM, declip, `--steps` steps, injected noise, one mel for the batch) per step
  plain_step           sampling_ddim over the same steps per step (the captured graph; first call excluded)"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _events(fn, before=None):
    import torch
    if before is not None:
        before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _median(fn, repeats, before=None):
    _events(fn, before)
    v = [_events(fn, before) for _ in range(repeats)]
    return dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), n=len(v))


def leg(args):
    import torch
    from benchlib.configs import CONFIGS, build_model
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, declip_operator, sampling_ddim, sampling_guided
    lib = _lib.load()
    cfg = CONFIGS[args.config]
    dev = torch.device("cuda")
    net = build_model(cfg, dev).eval()
    B, L = args.batch, args.length
    hop = 256
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(B, 1, L, generator=g) * 0.5).to(dev)
    steps = torch.randint(0, cfg["diffusion"]["T"], (B,), generator=g).float().to(dev)
    dout = torch.randn(B, 1, L, generator=g).to(dev)
    out, da = torch.empty_like(x), torch.empty_like(x)
    mel = (torch.rand(B, 80, L // hop, generator=g) * 13.5 - 11.5).to(dev) if "Tmel" in cfg else None
    net._sync_params(L)
    net._prepare(B, L)
    net._set_condition(mel)
    s = _lib.current_stream
    fwd = lambda: _lib.check(lib.dws_model_forward_input(net._handle, x.data_ptr(), steps.data_ptr(), out.data_ptr(), s()))
    bwd = lambda: _lib.check(lib.dws_model_backward_input(net._handle, dout.data_ptr(), da.data_ptr(), 0, s()))
    res = dict(variant="rocfft" if os.environ.get("DWS_SASHIMI_ROCFFT") else "segmented", config=args.config, B=B, L=L,
               kernels_L=cfg["model"]["L"])
    res["forward_input"] = _median(fwd, args.repeats)
    res["backward_data_only"] = _median(bwd, args.repeats, fwd)
    res["pair"] = _median(lambda: (fwd(), bwd()), args.repeats)
    for key, name in (("seg_train", b"fftconv_seg_train"), ("seg_adjoint", b"fftconv_seg_adjoint"),
                      ("long_stage_fwd", b"long_stage_fwd"), ("long_stage_bwd", b"long_stage_bwd")):
        _lib.check(lib.dws_profile_enable(name))
        try:
            fwd(), bwd()
            torch.cuda.synchronize()
            n, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
            _lib.check(lib.dws_profile_query(ctypes.byref(n), ctypes.byref(ms)))
        finally:
            lib.dws_profile_disable()
        res[key] = dict(launches=int(n.value), total_ms=round(ms.value, 3))
    d = cfg["diffusion"]
    dh = calc_diffusion_hyperparams(d["T"], d["beta_0"], d["beta_T"])
    S, size = args.steps, (B, 1, L)
    op = declip_operator(0.2)
    y = op(x * 0.5)
    x_T = torch.randn(size, generator=g).to(dev)
    noise = torch.randn((S,) + size, generator=g).to(dev)
    mel1 = None if mel is None else mel[:1]
    guided = lambda: sampling_guided(net, size, dh, measurement=y, operator=op, scale=0.5, sampler="ddim", steps=S, eta=1.0,
                                     condition=mel1, x_T=x_T, noise=noise)
    plain = lambda: sampling_ddim(net, size, dh, S, 1.0, mel1, x_T=x_T, noise=noise)
    per_step = lambda r: {k: (round(v / S, 3) if k.endswith("_ms") else v) for k, v in r.items()}
    res["guided_step"] = per_step(_median(guided, args.repeats))
    res["plain_step"] = per_step(_median(plain, args.repeats))
    res["guided_over_plain"] = round(res["guided_step"]["median_ms"] / res["plain_step"]["median_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="unet_d32_n6_T50_cond")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--length", type=int, default=212992)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(args)), flush=True)
        return
    rows = []
    argv = [sys.executable, os.path.abspath(__file__), "--leg", "--config", args.config, "--batch", str(args.batch), "--length",
            str(args.length), "--repeats", str(args.repeats), "--steps", str(args.steps)]
    for rnd in range(args.rounds):
        for variant in ("segmented", "rocfft"):
            env = dict(os.environ)
            env.pop("DWS_SASHIMI_ROCFFT", None)
            if variant == "rocfft":
                env["DWS_SASHIMI_ROCFFT"] = "1"
            r = subprocess.run(argv, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:       # (nothing more is started on the card after a leg that did not end well)
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(r.returncode if r.returncode > 0 else 1)
            row = json.loads(r.stdout.strip().splitlines()[-1])
            row["round"] = rnd
            print(json.dumps(row), flush=True)
            rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

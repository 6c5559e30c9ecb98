"""Device-event times of the two backward modes and of a guided (DPS) sampler step, on one GPU.

    python tools/guided_step_times.py [--configs unet_d64_n6_T200,wnet_h256_d36_T200] [--precisions f32,bf16x6]
                                      [--repeats 5] [--steps 4] [--batch B] [--out FILE] [--backward-only]

Per (config, precision), each the median of `--repeats` after a warm-up, timed with device events on the stream:
  forward_train        dws_model_forward_train
  backward             dws_model_backward (every parameter gradient; what a training step runs)
  backward_with_input  dws_model_backward_input(param_grads=1, daudio): the same plus the input gradient
  backward_data_only   dws_model_backward_input(param_grads=0, daudio): the input gradient alone
  guided_step          sampling_guided (DDIM, declip, `--steps` steps, injected noise) per step: a training forward, a
                       data-only backward and the torch autograd of the operator, eager
  plain_step           sampling_ddim over the same steps per step (the captured graph; first call excluded)
`--backward-only` times forward_train / backward alone; with DWS_LIB naming an older libdws.so (one without
dws_model_backward_input) this gives the number to set the new entry's param_grads=1 mode against, in the same session."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _events(fn, before=None):
    """Device time of fn() in ms (before(): enqueued ahead of the first event, not timed)."""
    if before is not None:
        before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _median(fn, repeats, before=None):
    _events(fn, before)      # warm-up: code objects, buffers of this mode
    v = [_events(fn, before) for _ in range(repeats)]
    return dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), n=len(v))


def leg(cfg_name, precision, args):
    from benchlib.configs import CONFIGS, build_model
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, declip_operator, sampling_ddim, sampling_guided
    lib = _lib.load()
    cfg = CONFIGS[cfg_name]
    dev = torch.device("cuda")
    net = build_model(cfg, dev)
    net.set_option("precision", precision)
    B, L = args.batch or cfg["B"], cfg["L"]
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(B, 1, L, generator=g) * 0.5).to(dev)
    steps = torch.randint(0, cfg["diffusion"]["T"], (B,), generator=g).float().to(dev)
    dout = torch.randn(B, 1, L, generator=g).to(dev)
    out, da = torch.empty_like(x), torch.empty_like(x)
    mel = None
    if "Tmel" in cfg:
        mel = (torch.rand(B, 80, cfg["Tmel"], generator=g) * 13.5 - 11.5).to(dev)
    net._sync_params(L)
    net._prepare(B, L)
    net._set_condition(mel)
    s = _lib.current_stream
    fwd = lambda: _lib.check(lib.dws_model_forward_train(net._handle, x.data_ptr(), steps.data_ptr(), out.data_ptr(), s()))
    res = dict(config=cfg_name, precision=precision, B=B, L=L)
    res["forward_train"] = _median(fwd, args.repeats)
    res["backward"] = _median(lambda: _lib.check(lib.dws_model_backward(net._handle, dout.data_ptr(), s())), args.repeats, fwd)
    if args.backward_only:
        return res
    bwd_in = lambda pg: _lib.check(lib.dws_model_backward_input(net._handle, dout.data_ptr(), da.data_ptr(), pg, s()))
    res["backward_with_input"] = _median(lambda: bwd_in(1), args.repeats, fwd)
    res["backward_data_only"] = _median(lambda: bwd_in(0), args.repeats, fwd)
    # a guided step next to the plain sampler's
    d = cfg["diffusion"]
    dh = calc_diffusion_hyperparams(d["T"], d["beta_0"], d["beta_T"])
    S = args.steps
    size = (B, 1, L)
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
    ap.add_argument("--configs", default="unet_d64_n6_T200,wnet_h256_d36_T200")
    ap.add_argument("--precisions", default="f32,bf16x6")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--backward-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.backward_only:      # an older library has no input-gradient entry to bind
        from diffwave_sashimi_amd import _lib
        _lib._SIGS.pop("dws_model_backward_input", None)
    rows = []
    for c in args.configs.split(","):
        for p in args.precisions.split(","):
            r = leg(c, p, args)
            print(json.dumps(r), flush=True)
            rows.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

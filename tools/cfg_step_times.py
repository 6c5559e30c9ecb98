"""Device-event times of class-conditional sampling and training, on one GPU.

    python tools/cfg_step_times.py [--configs wnet_h256_d36_T200,unet_d64_n6_T200] [--precisions f32,bf16x6]
                                   [--bc 16] [--classes 10] [--steps 8] [--repeats 5] [--legs cfg,table,train]
                                   [--unlabelled-only] [--out FILE]

Per (config, precision), each the median (with min / max) of `--repeats` runs after a warm-up run, timed with device
events on the stream; sampler figures are per step of a `--steps`-step DDIM run through the captured graph:
  unlabelled_step   a model WITHOUT classes at B = bc: the path this feature must not touch.  `--unlabelled-only` times
                    this alone and binds none of the new entry points, so that DWS_LIB may name the parent commit's
                    libdws.so: alternate the two libraries in one session and compare.
  plain_step_2bc    the labelled model (n_classes = `--classes`) at B = 2 bc, labels installed: the captured plain step
  cfg_step          classifier-free guidance at Bc = bc (the network at 2 bc, the guided eps, the update over bc clips,
                    the mirror copy); cfg_minus_plain_ms is what the two small kernels and the halved update cost
  table (leg)       the labelled step table at T = 200, B = 2 bc: rewrite_ms = a one-step run that follows a new label
                    assignment minus the same run with the assignment unchanged (every per-(step, clip) row rebuilt: the
                    label rows, every block's fc_t rows, WaveNet's correction fragments); resident bytes by the formula and
                    as the drop of free device memory over the first build
  train (leg)       one training step (forward_train + backward + get_grads through autograd) of the config-5 network
                    (unet_d128_n6) at its per-GPU batch, labelled against unlabelled
Audio quality is not measured here or anywhere: no trained class-conditional weights exist."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _median(fn, repeats, scale=1.0):
    _events(fn)      # warm-up: code objects, buffers, step table, graph capture
    v = [_events(fn) * scale for _ in range(repeats)]
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), n=len(v))


def _model(cfg, dev, precision, classes=0):
    from benchlib.configs import build_model
    c = dict(cfg, model=dict(cfg["model"], **({"n_classes": classes} if classes else {})))
    net = build_model(c, dev)
    net.set_option("precision", precision)
    return net


def sampler_leg(cfg_name, precision, args):
    from benchlib.configs import CONFIGS
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling_ddim
    cfg = CONFIGS[cfg_name]
    dev = torch.device("cuda")
    d = cfg["diffusion"]
    dh = calc_diffusion_hyperparams(d["T"], d["beta_0"], d["beta_T"])
    S, bc, L = args.steps, args.bc, cfg["L"]
    g = torch.Generator().manual_seed(3)
    res = dict(config=cfg_name, precision=precision, bc=bc, L=L, steps=S, lib=os.environ.get("DWS_LIB", "in-tree"))

    def ddim(net, B, **kw):
        x_T = torch.randn(B, 1, L, generator=g).to(dev)
        noise = torch.randn(S, B, 1, L, generator=g).to(dev)
        return lambda: sampling_ddim(net, (B, 1, L), dh, S, 1.0, x_T=x_T, noise=noise, **kw)

    net = _model(cfg, dev, precision)
    res["unlabelled_step"] = _median(ddim(net, bc), args.repeats, 1.0 / S)
    del net
    torch.cuda.empty_cache()
    if args.unlabelled_only:
        return res
    net = _model(cfg, dev, precision, args.classes)
    lab = [i % args.classes for i in range(2 * bc)]
    res["plain_step_2bc"] = _median(ddim(net, 2 * bc, labels=lab), args.repeats, 1.0 / S)
    res["cfg_step"] = _median(ddim(net, bc, labels=lab[:bc], cfg_scale=1.5), args.repeats, 1.0 / S)
    res["cfg_minus_plain_ms"] = round(res["cfg_step"]["median_ms"] - res["plain_step_2bc"]["median_ms"], 4)
    return res


def table_leg(cfg_name, precision, args):
    from benchlib.configs import CONFIGS
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling_ddim
    cfg = CONFIGS[cfg_name]
    dev = torch.device("cuda")
    T, B, L = 200, 2 * args.bc, cfg["L"]
    dh = calc_diffusion_hyperparams(T, 1e-4, 0.02)
    net = _model(cfg, dev, precision, args.classes)
    x = torch.randn(B, 1, L, generator=torch.Generator().manual_seed(4)).to(dev)
    # all T steps in the table, ONE of them run (a partial start at step 0 with the state as given)
    one = lambda lab: sampling_ddim(net, (B, 1, L), dh, T, 0.0, x_start=x, start_step=0, start_noise=False, labels=lab)
    labs = [[(i + k) % args.classes for i in range(B)] for k in range(2 * args.repeats + 2)]
    one(None)                                   # buffers, graph, the unlabelled (per-step) table
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    first = _events(lambda: one(labs[0]))       # the first labelled build (allocates the per-(step, clip) rows)
    torch.cuda.synchronize()
    grown = free0 - torch.cuda.mem_get_info()[0]
    same, new = [], []
    for k in range(1, args.repeats + 1):
        new.append(_events(lambda: one(labs[k])))
        same.append(_events(lambda: one(labs[k])))
    m = net
    E = m.embed_dims[2]
    if cfg["model"]["_name_"] == "wavenet":
        C, NL = m.res_channels, m.num_res_layers
        rows = NL * C + NL * 4 * 2 * C + E          # fc_t rows + correction fragments (Winograd layout) + summed embedding
    else:
        rows = sum(b.H for b in m._blocks()) + E
    diff = [a - b for a, b in zip(new, same)]
    return dict(config=cfg_name, precision=precision, T=T, B=B, leg="table",
                first_build_and_step_ms=round(first, 3),
                rewrite_ms=dict(median_ms=round(statistics.median(diff), 3), min_ms=round(min(diff), 3),
                                max_ms=round(max(diff), 3), n=len(diff)),
                one_step_ms=round(statistics.median(same), 3),
                table_bytes_formula=T * B * rows * 4, device_memory_grown_bytes=int(grown))


def train_leg(precision, args):
    from benchlib.configs import CONFIGS
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    cfg = CONFIGS["unet_d128_n6_T200"]
    dev = torch.device("cuda")
    B, L = 32, cfg["L"]
    dh = calc_diffusion_hyperparams(200, 1e-4, 0.02)
    audio = ((torch.rand(B, 1, L, generator=torch.Generator().manual_seed(5)) * 2 - 1) * 0.3).to(dev)
    res = dict(config="unet_d128_n6_T200 training", precision=precision, B=B, L=L, leg="train")
    for name, classes in (("unlabelled_step", 0), ("labelled_step", args.classes)):
        net = _model(cfg, dev, precision, classes).train()
        labels = torch.arange(B) % args.classes if classes else None
        loss_fn = torch.nn.MSELoss()

        def step():
            for p in net.parameters():
                p.grad = None
            kw = dict(labels=labels, label_dropout=0.1) if classes else {}
            training_loss(net, loss_fn, audio, dh, **kw).backward()

        res[name] = _median(step, args.repeats)
        del net
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="wnet_h256_d36_T200,unet_d64_n6_T200")
    ap.add_argument("--precisions", default="f32,bf16x6")
    ap.add_argument("--bc", type=int, default=16)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", default="cfg,table,train")
    ap.add_argument("--unlabelled-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.unlabelled_only:      # the parent commit's library has none of the new entry points to bind
        from diffwave_sashimi_amd import _lib
        for k in ("dws_model_set_classes", "dws_model_set_labels", "dws_sampler_set_cfg"):
            _lib._SIGS.pop(k, None)
        args.legs = "cfg"
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    legs = args.legs.split(",")
    for c in args.configs.split(","):
        for p in args.precisions.split(","):
            if "cfg" in legs:
                emit(sampler_leg(c, p, args))
            if "table" in legs:
                emit(table_leg(c, p, args))
    if "train" in legs:
        for p in args.precisions.split(","):
            emit(train_leg(p, args))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

"""Cost of the adaptive prior in the schedule sampler's step ("Adaptive prior"): the headline
configuration's DDPM step with a prior table installed against the step without one, in one process, the legs
alternating.

    python tools/prior_step_times.py [--config wnet_h256_d36_T200] [--steps 40] [--rounds 3]

Two figures per leg:
  ms_per_step   a whole captured run of --steps steps (`sampling(..., net_steps=0..T-1)`, use_graph=True) between two
                events, divided by the steps -- the replayed step as a user runs it (the run's x_T draw and copies included);
  update_us     the update kernel alone, per launch: the engine's per-launch events (dws_profile_enable("smp_update"))
                around the update of uncaptured steps (launches inside a capture are not timed), first launch dropped.
The prior adds one read of the [B, C L] table per noise site: here the update kernel's, once per step.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="wnet_h256_d36_T200")
    ap.add_argument("--precision", default="bf16x6")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from benchlib.configs import CONFIGS, build_model
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling
    cfg = CONFIGS[args.config]
    net = build_model(cfg, torch.device("cuda"))
    if args.precision != "f32":
        net.set_option("precision", args.precision)
    B, L, d = cfg["B"], cfg["L"], cfg["diffusion"]
    T = args.steps
    dh = calc_diffusion_hyperparams(T, d["beta_0"], d["beta_T"])
    steps = np.arange(T, dtype=np.float32)
    sigma = (torch.rand(B, 1, L, generator=torch.Generator().manual_seed(1)) * 0.9 + 0.1).cuda()
    lib = _lib.load()
    legs = {"off": {}, "on": {"prior_std": sigma}}
    run = lambda leg, graph: sampling(net, (B, 1, L), dh, seed=1, use_graph=graph, net_steps=steps, **legs[leg])
    for leg in legs:            # warm-up: code objects, buffers, step table, both captures
        run(leg, True)
        run(leg, False)
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for leg in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(leg, True)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / T
            _lib.check(lib.dws_profile_enable(b"smp_update"))
            try:
                run(leg, False)
                torch.cuda.synchronize()
                n = ctypes.c_int64()
                buf = (ctypes.c_double * 1024)()
                _lib.check(lib.dws_profile_query_each(buf, 1024, ctypes.byref(n)))
            finally:
                lib.dws_profile_disable()
            us = [buf[i] * 1e3 for i in range(min(n.value, 1024))][1:]
            print(json.dumps(dict(round=r, prior=leg, config=args.config, precision=args.precision, B=B, L=L, steps=T,
                                  ms_per_step=round(ms, 4), update_launches=len(us),
                                  update_us_median=round(statistics.median(us), 3), update_us_min=round(min(us), 3),
                                  update_us_max=round(max(us), 3))), flush=True)


if __name__ == "__main__":
    main()

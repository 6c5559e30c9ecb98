"""Time of the DDPM update kernel of the schedule sampler per launch, with the scalar seed or with per-clip seeds
(DESIGN.md section 4).  Measured with the engine's per-launch events (dws_profile_enable("smp_update") /
dws_profile_query_each) around the update kernel of uncaptured steps (use_graph=False: launches inside a capture are not
timed); one run of --steps steps after a warm-up run, the first launch (t = T-1) dropped.

    python tools/clip_seed_update_times.py --seeds scalar|clips [--root TREE] [--config wnet_h256_d36_T200]

--root: the checkout whose package and library are measured (default: this one), so that one script times two builds
back to back; only the scalar form exists in a tree without dws_sampler_set_clip_seeds.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seeds", choices=["scalar", "clips"], default="scalar")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--config", default="wnet_h256_d36_T200")
    ap.add_argument("--precision", default="bf16x6")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
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
    seed = 1 if args.seeds == "scalar" else list(range(1, B + 1))
    lib = _lib.load()
    run = lambda: sampling(net, (B, 1, L), dh, seed=seed, use_graph=False, net_steps=np.arange(T, dtype=np.float32))
    run()                                                    # warm-up: code objects, buffers, step table
    torch.cuda.synchronize()
    _lib.check(lib.dws_profile_enable(b"smp_update"))
    try:
        run()
        torch.cuda.synchronize()
        n = ctypes.c_int64()
        buf = (ctypes.c_double * 1024)()
        _lib.check(lib.dws_profile_query_each(buf, 1024, ctypes.byref(n)))
    finally:
        lib.dws_profile_disable()
    us = [buf[i] * 1e3 for i in range(min(n.value, 1024))][1:]
    print(json.dumps(dict(tag=args.tag, seeds=args.seeds, config=args.config, precision=args.precision, B=B, L=L,
                          launches=len(us), median_us=round(statistics.median(us), 3), min_us=round(min(us), 3),
                          max_us=round(max(us), 3), lib=os.path.relpath(_lib.LIB_PATH, os.path.abspath(args.root)))),
          flush=True)


if __name__ == "__main__":
    main()

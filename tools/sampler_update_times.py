"""Time of the few-step samplers' update kernel per step, by kind: DDIM against DPM-Solver++(2M),
whose step also reads and writes the [B, C, L] history buffer.  Measured with the engine's per-launch events
(dws_profile_enable("smp_update") / dws_profile_query_each) around the update kernel of uncaptured steps
(use_graph=False: launches inside a capture are not timed); one run of S = 6 steps per kind after a warm-up run.

    python tools/sampler_update_times.py [--config wnet_h256_d36_T200] [--steps 6]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="wnet_h256_d36_T200")
    ap.add_argument("--steps", type=int, default=6)
    args = ap.parse_args()
    from benchlib.configs import CONFIGS, build_model
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling_ddim, sampling_dpmpp
    cfg = CONFIGS[args.config]
    net = build_model(cfg, torch.device("cuda"))
    B, L, d = cfg["B"], cfg["L"], cfg["diffusion"]
    dh = calc_diffusion_hyperparams(d["T"], d["beta_0"], d["beta_T"])
    lib = _lib.load()
    runs = {"ddim": lambda: sampling_ddim(net, (B, 1, L), dh, args.steps, 0.0, seed=1, use_graph=False),
            "dpmpp2m": lambda: sampling_dpmpp(net, (B, 1, L), dh, args.steps, seed=1, use_graph=False)}
    for name, run in runs.items():
        run()                                                    # warm-up: code objects, buffers, step table
        torch.cuda.synchronize()
        _lib.check(lib.dws_profile_enable(b"smp_update"))
        try:
            run()
            torch.cuda.synchronize()
            n = ctypes.c_int64()
            buf = (ctypes.c_double * 64)()
            _lib.check(lib.dws_profile_query_each(buf, 64, ctypes.byref(n)))
        finally:
            lib.dws_profile_disable()
        us = [round(buf[i] * 1e3, 2) for i in range(min(n.value, 64))]
        print(json.dumps(dict(sampler=name, config=args.config, B=B, L=L, launches=n.value, us_per_step=us,
                              mean_us=round(sum(us) / max(len(us), 1), 2))), flush=True)


if __name__ == "__main__":
    main()

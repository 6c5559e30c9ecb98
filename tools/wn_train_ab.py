"""Same-box A/B of the WaveNet training step: precision f32 against bf16x6, in one process.

    python tools/wn_train_ab.py [--config wnet_h256_d36_T200] [--batch 4] [--steps 20] [--warmup 3] [--rounds 2] [--legs f32,bf16x6]

Each round runs benchlib.train.train_bench once per leg, alternating f32 and bf16x6 (a fresh model per leg, the same
synthetic batch and seed), so that clock or thermal drift over the run reaches both legs alike.  Prints one line per leg and
round, then one JSON line with every ms_per_step and final loss and the per-leg medians.  bench.py is not involved: its
--mode train keeps timing WaveNet training in f32."""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="wnet_h256_d36_T200")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per leg and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--legs", default="f32,bf16x6", help="comma-separated precisions (one alone: e.g. for a kernel trace per leg)")
    args = ap.parse_args()

    import torch
    from benchlib.configs import CONFIGS
    from benchlib.train import train_bench
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd import dist as ddist

    _lib.load()
    cfg = dict(CONFIGS[args.config])
    assert cfg["model"]["_name_"] == "wavenet", "a WaveNet config"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    legs = tuple(args.legs.split(","))
    runs = {p: [] for p in legs}
    for r in range(args.rounds):
        for prec in legs:
            a = types.SimpleNamespace(config=args.config, batch=args.batch, steps=args.steps, warmup=args.warmup,
                                      precision=prec, full=False, no_roofline=True, cpu_train_baseline=False)
            line = train_bench(a, cfg, 1, 0, dev, ddist, emit=False)
            runs[prec].append({"ms_per_step": line["ms_per_step"], "final_loss": line["final_loss"]})
            print(f"round {r} {prec:7s} {line['ms_per_step']:8.2f} ms/step  final loss {line['final_loss']:.6f}", flush=True)
    med = {p: statistics.median(x["ms_per_step"] for x in runs[p]) for p in legs}
    print(json.dumps({"config": args.config, "batch": args.batch, "L": cfg["L"], "steps_per_leg_and_round": args.steps,
                      "warmup": args.warmup, "rounds": args.rounds, "legs": runs, "median_ms_per_step": med,
                      **({"bf16x6_over_f32": med["bf16x6"] / med["f32"]} if set(legs) >= {"f32", "bf16x6"} else {}),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()

"""One training step of `experiment=ljspeech_harder` through the HIP engine: SaShiMi unet d_model 128, n_layers 6,
pool [4, 4], expand 2, ff 2, L = 44000 (the top stage's twelve blocks on the rocFFT convolution), B = 2, mel conditioning at
hop 2048 (mel_upsample [32, 64]); seeded random weights, audio and mel.  Adam as `train.py` runs it.

Per precision: warm-up steps, then >= 20 steps timed with device events (ms per step), then one profiled step per name of
the long stage (ProfileScope event pairs: the whole rocFFT-stage convolution forward / backward, and each new kernel with the
bytes its shapes move).  Prints one JSON line per precision.

    python tools/long_stage_train_step.py [--precision f32,bf16x6] [--steps 20] [--warmup 3] [--no-profile]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TBS = 8.0       # MI355X HBM3E peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f32,bf16x6")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()

    import torch
    import torch.nn as nn
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from diffwave_sashimi_amd.training import training_loss
    from tests import cases

    dev = torch.device("cuda:0")
    B, L, H, Tmel = 2, 44000, 128, 22
    cfg = cases.ss_cfg(d_model=H, n_layers=6, L=L, pool=[4, 4], expand=2, ff=2, unconditional=False, mel_upsample=[32, 64])
    dh = calc_diffusion_hyperparams(50, 1e-4, 0.05)
    g = torch.Generator().manual_seed(99)
    audio = ((torch.rand(B, 1, L, generator=g) * 2 - 1) * 0.3).to(dev)
    mel = cases.mel_inputs(B, Tmel, 5).to(dev)
    lib = _lib.load()
    Lf = L + 1
    f = 4
    # bytes each new kernel moves, from its shapes (one launch at the top stage: B H rows of L, 2L-padded rows, L+1 bins)
    kernel_bytes = {
        "pad_rows": B * H * L * f + B * H * 2 * L * f,
        "s4_post_train": 2 * B * H * L * f + 2 * B * H * L * f,
        "conv_adjoint_spec": (3 * B * H * Lf + 2 * H * Lf) * 2 * f,
        "conv_adjoint_epi": 3 * B * H * L * f,
        "s4_twosided_bwd": 4 * H * L * f,
    }

    for prec in args.precision.split(","):
        net = cases.build_ours(cfg, 15).to(dev).train()
        net.set_option("precision", prec)
        opt = torch.optim.Adam(net.parameters(), lr=2e-4)
        loss_fn = nn.MSELoss()

        def step():
            opt.zero_grad(set_to_none=True)
            loss = training_loss(net, loss_fn, audio, dh, mel_spec=mel, generator=g)
            loss.backward()
            opt.step()
            return loss

        for _ in range(max(args.warmup, 1)):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            loss = step()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.steps
        res = {"config": "ljspeech_harder", "precision": prec, "B": B, "L": L, "d_model": H, "n_layers": 6,
               "ms_per_step": round(ms, 3), "loss": float(loss.detach()), "steps": args.steps}
        if not args.no_profile:
            prof = {}
            for name in ("long_stage_fwd", "long_stage_bwd", *kernel_bytes):
                _lib.check(lib.dws_profile_enable(name.encode()))
                step()
                torch.cuda.synchronize()
                n, tot = ctypes.c_int64(), ctypes.c_double()
                _lib.check(lib.dws_profile_query(ctypes.byref(n), ctypes.byref(tot)))
                lib.dws_profile_disable()
                per = tot.value / max(n.value, 1)
                row = {"launches": n.value, "ms_total": round(tot.value, 4), "us_per_launch": round(per * 1e3, 2)}
                if name in kernel_bytes:
                    gbs = kernel_bytes[name] / (per * 1e-3) / 1e9
                    row.update({"mbytes_per_launch": round(kernel_bytes[name] / 1e6, 2), "GB_s": round(gbs, 1),
                                "frac_of_8TBs": round(gbs / (HBM_TBS * 1e3), 3)})
                prof[name] = row
            long_ms = prof["long_stage_fwd"]["ms_total"] + prof["long_stage_bwd"]["ms_total"]
            res["long_stage_ms"] = round(long_ms, 3)
            res["long_stage_share"] = round(long_ms / ms, 3)
            res["profile"] = prof
        print(json.dumps(res), flush=True)
        del net, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

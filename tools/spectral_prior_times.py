"""Cost of the spectral prior ("Spectral prior"), in one process, the legs alternating.

    python tools/spectral_prior_times.py [--config wnet_h256_d36_T200] [--precision bf16x6] [--rounds 3]

Three measurements, each between two device events after a warm-up of every shape:
  kernel   ``dws_tv_filter`` forwards and as the adjoint (``mel.tv_filter``: two launches and the workspace's allocation
           from torch's cache) at B = 32, T = 16128 = 63 hops (the kernel's T is a multiple of the hop: the 16000 of the
           benchmark's clips rounded up), n_fft 1024, hop 256; ms per call over --calls calls.
  step     a training step of --config at B = 4, L = 16128 (``training_loss`` + ``backward``; no optimizer) without the
           prior -- the step as it was before the prior existed: not one operation of it changed -- and with it (the
           filter handed in), and the filter's design (``TacotronSTFT.spectral_filter``, float64 torch) on its own,
           which a training loop pays once per batch on top.
  shaping  the one-off noise shaping ahead of a T = 200, B = 16 DDPM run: 200 Philox draws and filter calls, and the
           [200, 16, 1, 16128] tensor they fill.
"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="wnet_h256_d36_T200")
    ap.add_argument("--precision", default="bf16x6")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from benchlib.configs import CONFIGS, build_model
    from diffwave_sashimi_amd import mel as melmod
    from diffwave_sashimi_amd import sampling as smp
    from diffwave_sashimi_amd.training import training_loss
    dev = torch.device("cuda")
    hop, n_fft, L = 256, 1024, 63 * 256
    stft = melmod.TacotronSTFT(filter_length=n_fft, hop_length=hop, win_length=n_fft)
    window = stft._tables(dev)[0]
    g = torch.Generator().manual_seed(1)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def log_mel(B):     # the log-mel range of the reference's front-end, U(-11.5, 2)
        return (torch.rand(B, 80, L // hop, generator=g) * 13.5 - 11.5).to(dev)

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    # ---- kernel
    B = 32
    x = torch.randn(B, L, generator=g).to(dev)
    F = stft.spectral_filter(log_mel(B), L, ref=30.0)
    legs = {"forward": lambda: melmod.tv_filter(x, F, window=window, hop_length=hop),
            "adjoint": lambda: melmod.tv_filter(x, F, window=window, hop_length=hop, adjoint=True)}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for leg, fn in legs.items():
            emit(what="kernel", round=r, leg=leg, B=B, T=L, n_fft=n_fft, hop=hop, calls=args.calls,
                 ms_per_call=round(timed(fn, args.calls), 4))

    # ---- training step
    cfg = CONFIGS[args.config]
    net = build_model(cfg, dev).train()
    if args.precision != "f32":
        net.set_option("precision", args.precision)
    B = 4
    d = cfg["diffusion"]
    dh = smp.calc_diffusion_hyperparams(d["T"], d["beta_0"], d["beta_T"])
    audio = (torch.rand(B, 1, L, generator=g) * 0.6 - 0.3).to(dev)
    mel = log_mel(B)
    F4 = stft.spectral_filter(mel, L, ref=30.0)
    loss_fn = torch.nn.MSELoss()

    def step(**kw):
        net.zero_grad(set_to_none=True)
        training_loss(net, loss_fn, audio, dh, **kw).backward()

    legs = {"off": lambda: step(), "on": lambda: step(prior_filter=F4, prior_stft=stft),
            "design": lambda: stft.spectral_filter(mel, L, ref=30.0)}
    for fn in legs.values():
        fn()
        fn()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for leg, fn in legs.items():
            emit(what="step", round=r, leg=leg, config=args.config, precision=args.precision, B=B, L=L, steps=args.steps,
                 ms_per_step=round(timed(fn, args.steps), 4))

    # ---- the noise shaping of a whole run
    B, S = 16, 200
    F16 = stft.spectral_filter(log_mel(B), L, ref=30.0)
    shape = lambda: smp.spectral_prior_noise((B, 1, L), S, F16, stft, seed=1)
    shape()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        emit(what="shaping", round=r, B=B, L=L, steps=S, noise_gb=round(S * B * L * 4 / 1e9, 3), ms=round(timed(shape, 1), 3))


if __name__ == "__main__":
    main()

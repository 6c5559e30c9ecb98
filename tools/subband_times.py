"""Times of multi-band runs ("Multi-band runs"): the two PQMF kernels, the network evaluation on K
sub-bands against the full band, and a training step with and without sub-bands.

    python tools/subband_times.py [--batch 16] [--samples 16000] [--repeats 20] [--train-batch 4] [--only kernels|steps|train]

Every figure is the median (and the smallest) over --repeats of the time between two events around the call, after a
warm-up call; everything runs in one process on one GPU on seeded random weights.  One JSON line per measurement:

* ``kernel``: ``PQMF.analysis`` / ``PQMF.synthesis`` (one launch each, output allocation included) at [B, T] for K = 2 and
  K = 4, beside a device copy of the same B x T floats -- the 2 x 4 x B x T bytes both kernels move -- at the measured
  copy rate.
* ``step``: one network evaluation (``net((x, t))``, eval, no grad) of ``wnet_h256_d36`` under bf16x6 and of
  ``unet_d64_n6`` at B = --batch: one channel at L = --samples against ``in_channels = out_channels = 4`` at L / 4 (the
  SaShiMi built with ``L = samples / 4``, so that its kernels are generated at the length they run at), as samples of
  audio per second, and the kernels that ran (launch counts of the engine's profile scopes in one evaluation).
* ``train``: one ``training_loss`` + ``backward`` of ``wnet_h256_d36`` under bf16x6 at B = --train-batch, full band and on
  4 sub-bands, each without and with ``stft_weight`` (the default three resolutions).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

SCOPES = ("wn_layer_bx6", "wn_layer_wino_mfma", "wn_layer_mfma", "wn_layer_generic", "init_conv", "wn_final", "fftconv_seg",
          "fftconv", "rocfft_r2c", "long_stage_fwd", "s4_tail_mfma_chain", "s4_tail_mfma", "spec_mul", "pw_glu_res")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--train-batch", type=int, default=4)
    ap.add_argument("--only", choices=("kernels", "steps", "train"), default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from benchlib.configs import CONFIGS, build_model
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.pqmf import PQMF
    dev = torch.device("cuda")
    lib = _lib.load()
    B, T = args.batch, args.samples

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    if args.only in (None, "kernels"):
        x = torch.randn(B, T, generator=torch.Generator().manual_seed(1)).to(dev)
        dst = torch.empty_like(x)
        c_med, c_min, c_max = timed(lambda: dst.copy_(x))
        emit(kernel="copy", B=B, T=T, bytes=2 * 4 * B * T, ms_median=c_med, ms_min=c_min, ms_max=c_max,
             gb_per_s=round(2 * 4 * B * T / (c_med * 1e-3) / 1e9, 1))
        for K in (2, 4):
            P = PQMF(K)
            s = P.analysis(x)
            a = timed(lambda: P.analysis(x))
            y = timed(lambda: P.synthesis(s))
            emit(kernel="pqmf", K=K, B=B, T=T, taps=P.taps, analysis_ms_median=a[0], analysis_ms_min=a[1], analysis_ms_max=a[2],
                 synthesis_ms_median=y[0], synthesis_ms_min=y[1], synthesis_ms_max=y[2], copy_ms_median=c_med)

    def scopes_of(call):
        """Launch counts of the engine's profile scopes over one ``call()`` (one run per scope name)."""
        ran = {}
        for name in SCOPES:
            _lib.check(lib.dws_profile_enable(name.encode()))
            call()
            torch.cuda.synchronize()
            n, ms = ctypes.c_int64(), ctypes.c_double()
            _lib.check(lib.dws_profile_query(ctypes.byref(n), ctypes.byref(ms)))
            lib.dws_profile_disable()
            if n.value:
                ran[name] = n.value
        return ran

    def model(name, channels, L, precision):
        cfg = dict(CONFIGS[name])
        cfg["model"] = dict(cfg["model"], in_channels=channels, out_channels=channels)
        if cfg["model"]["_name_"] == "sashimi":
            cfg["model"]["L"] = L
        net = build_model(cfg, dev)
        if precision != "f32":
            net.set_option("precision", precision)
        return net

    if args.only in (None, "steps"):
        for name, precision in (("wnet_h256_d36_T200", "bf16x6"), ("unet_d64_n6_T200", "f32")):
            rates = {}
            for K in (1, 4):
                net = model(name, K, T // K, precision)
                x = torch.randn(B, K, T // K, generator=torch.Generator().manual_seed(2)).to(dev)
                t = torch.full((B, 1), 17.0, device=dev)
                with torch.no_grad():
                    med, lo, hi = timed(lambda: net((x, t)))
                    ran = scopes_of(lambda: net((x, t)))
                rates[K] = B * T / (med * 1e-3)
                emit(step=name, precision=precision, channels=K, B=B, positions=T // K, audio_samples=T, ms_median=med, ms_min=lo,
                     ms_max=hi, audio_samples_per_s=round(rates[K]), scopes=ran)
                del net
            emit(step=name, precision=precision, subband_over_full_band=round(rates[4] / rates[1], 3))

    if args.only in (None, "train"):
        from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
        from diffwave_sashimi_amd.training import training_loss
        name, Bt = "wnet_h256_d36_T200", args.train_batch
        dh = calc_diffusion_hyperparams(200, 1e-4, 0.02)
        mse = torch.nn.MSELoss()
        audio = (torch.rand(Bt, 1, T, generator=torch.Generator().manual_seed(3)) * 0.6 - 0.3).to(dev)
        for K in (1, 4):
            net = model(name, K, T // K, "bf16x6").train()
            band = {} if K == 1 else {"pqmf": PQMF(K)}
            for stft in (None, 0.1):
                def step():
                    net.zero_grad(set_to_none=True)
                    training_loss(net, mse, audio, dh, generator=torch.Generator().manual_seed(4), stft_weight=stft,
                                  **band).backward()
                med, lo, hi = timed(step)
                emit(train=name, precision="bf16x6", channels=K, B=Bt, audio_samples=T, stft_weight=stft, ms_median=med,
                     ms_min=lo, ms_max=hi)
            del net


if __name__ == "__main__":
    main()

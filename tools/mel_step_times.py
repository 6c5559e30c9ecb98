"""Device-event times of the mel front-end's two kernels and of a mel-guided sampler step, on one GPU.

    python tools/mel_step_times.py [--repeats 7] [--steps 4] [--batch 16] [--configs test_sashimi_cond,unet_d32_n6_T50_cond]
                                   [--out FILE]

  mel_forward / mel_backward   dws_mel_spectrogram / dws_mel_spectrogram_backward at LJ's transform (filter 1024, hop 256,
                               80 bands, 22050 Hz), B = 16, T = 16000: `--calls` calls per event pair, ms per call, median /
                               min / max of `--repeats` after a warm-up.  The backward is both of its kernels (the per-frame
                               adjoint and the gather); the workspace is allocated once, outside the timing.
  guided step                  sampling_guided (DDIM, `--steps` steps, eta 1, injected noise, eager) per step with
                               mel_operator (LJ's transform; the measurement is the model's conditioning-sized mel of a
                               random clip) and with lowpass_operator(2), alternating mel / lowpass / mel / lowpass ... in
                               one process: `test_sashimi_cond` is the conditional SaShiMi of tests/test_guided_sampling_gpu.py
                               (d32, 1 layer, L = 1024, B = 2), the other names are benchlib configs at `--batch` clips."""
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


def _stats(v, per=1):
    v = [x / per for x in v]
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), n=len(v))


def kernel_times(args):
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.mel import MEL_CLIP, TacotronSTFT
    lib = _lib.load()
    dev = torch.device("cuda")
    st = TacotronSTFT(sampling_rate=22050)
    B, T, N, hop, M = 16, 16000, st.filter_length, st.hop_length, st.n_mel_channels
    F = T // hop + 1
    g = torch.Generator().manual_seed(3)
    x = ((torch.rand(B, T, generator=g) * 2 - 1) * 0.8).to(dev)
    dout = torch.randn(B, M, F, generator=g).to(dev)
    win, basis = st.window.to(dev), st.mel_basis.to(dev)
    out, dx, ws = torch.empty(B, M, F, device=dev), torch.empty(B, T, device=dev), torch.empty(B, F, N, device=dev)
    s = _lib.current_stream

    def fwd():
        for _ in range(args.calls):
            _lib.check(lib.dws_mel_spectrogram(x.data_ptr(), B, T, win.data_ptr(), basis.data_ptr(), N, hop, M, MEL_CLIP,
                                               out.data_ptr(), s()))

    def bwd():
        for _ in range(args.calls):
            _lib.check(lib.dws_mel_spectrogram_backward(x.data_ptr(), B, T, win.data_ptr(), basis.data_ptr(), N, hop, M,
                                                        MEL_CLIP, dout.data_ptr(), dx.data_ptr(), ws.data_ptr(), s()))
    res = dict(what="kernels", filter_length=N, hop_length=hop, bands=M, B=B, T=T, frames=F, calls_per_window=args.calls)
    for name, fn in (("mel_forward", fwd), ("mel_backward", bwd)):
        _events(fn)
        res[name] = _stats([_events(fn) for _ in range(args.repeats)], args.calls)
    res["backward_over_forward"] = round(res["mel_backward"]["median_ms"] / res["mel_forward"]["median_ms"], 2)
    return res


def guided_times(name, args):
    from diffwave_sashimi_amd.mel import TacotronSTFT
    from diffwave_sashimi_amd.sampling import (calc_diffusion_hyperparams, lowpass_operator, mel_operator, sampling_guided)
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    if name == "test_sashimi_cond":
        from tests import cases
        cfg = cases.ss_cfg(unconditional=False, d_model=32, n_layers=1, L=1024, mel_upsample=[16, 16],
                           diffusion_step_embed_dim_mid=64)
        net = cases.build_ours(cfg, 35).to(dev).eval()
        B, L, Tmel, d = 2, 1024, 4, dict(T=50, beta_0=1e-4, beta_T=0.05)
    else:
        from benchlib.configs import CONFIGS, build_model
        cfg = CONFIGS[name]
        net = build_model(cfg, dev)
        B, L, Tmel, d = args.batch, cfg["L"], cfg.get("Tmel"), cfg["diffusion"]
    dh = calc_diffusion_hyperparams(d["T"], d["beta_0"], d["beta_T"])
    S, size = args.steps, (B, 1, L)
    cond = None if Tmel is None else (torch.rand(1, 80, Tmel, generator=g) * 13.5 - 11.5).to(dev)
    clean = (torch.randn(size, generator=g) * 0.3).to(dev)
    x_T = torch.randn(size, generator=g).to(dev)
    noise = torch.randn((S,) + size, generator=g).to(dev)
    ops = {"mel": mel_operator(TacotronSTFT(sampling_rate=22050)), "lowpass": lowpass_operator(2)}
    runs = {}
    for k, op in ops.items():
        y = op(clean)
        runs[k] = lambda op=op, y=y: sampling_guided(net, size, dh, measurement=y, operator=op, scale=0.1, sampler="ddim",
                                                     steps=S, eta=1.0, condition=cond, x_T=x_T, noise=noise)
    times = {k: [] for k in runs}
    for k, fn in runs.items():
        _events(fn)                    # warm-up of every shape the timed window uses
    for _ in range(args.repeats):      # alternating, so a drift of the box hits both alike
        for k, fn in runs.items():
            times[k].append(_events(fn))
    res = dict(what="guided_step", config=name, B=B, L=L, steps=S, precision="f32")
    for k in runs:
        res[k + "_step"] = _stats(times[k], S)
    res["mel_over_lowpass"] = round(res["mel_step"]["median_ms"] / res["lowpass_step"]["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="test_sashimi_cond,unet_d32_n6_T50_cond")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mel_step_times: no GPU (there is nothing to time without one)")
    rows = [kernel_times(args)]
    print(json.dumps(rows[-1]), flush=True)
    for c in [c for c in args.configs.split(",") if c]:
        try:
            rows.append(guided_times(c, args))
        except NotImplementedError as e:       # a model the guided path is not built for: recorded, not timed
            rows.append(dict(what="guided_step", config=c, not_run=str(e)))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

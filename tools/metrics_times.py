"""Time of the objective-metrics kernel per STFT resolution ("Objective metrics"), and beside it
the float32 ``torch.stft`` restatement of the same sums (tests/spectral_reference.py: ``sums(..., dtype=float32)``) on
the same inputs on the same GPU.

    python tools/metrics_times.py [--batch 16] [--samples 160000] [--repeats 20]

One JSON line per pass (Parallel WaveGAN's three resolutions and the mel pass of ``TacotronSTFT()``): the median over
--repeats of one ``dws_spectral_distance`` call between two events (tables cached, workspace allocation included, no
copy to the host), the same for the restatement, and the largest relative difference of the two results.  A last line
times the pitch pass (``dws_pitch_distance`` at the defaults of ``metrics.pitch_metrics``, DESIGN.md section 4, "Pitch
metrics") at the same shape; it has no torch restatement beside it.

    python tools/metrics_times.py --loss [--batch 32] [--samples 16000] [--repeats 20]

times the spectral training loss instead ("Spectral loss"): ``metrics.mr_stft_loss`` forward, and
forward + backward, at the training shape and the three default resolutions, beside the float32 ``torch.stft`` autograd
restatement of the same loss.  One JSON line.  On an MI355X (B = 32, T = 16000): forward 2.77 ms, forward + backward
7.79 ms; the restatement 2.10 ms forward + backward (an FFT against the direct DFT); the gradients differ by 3.6e-4
relative L2.
"""
import argparse
import json
import os
import statistics
import sys


def loss_times(args, timed):
    """``mr_stft_loss(x, y).sum().backward()`` at the three default resolutions (``dws_spectral_distance`` +
    ``dws_spectral_loss_backward`` per resolution, workspaces included) beside the float32 ``torch.stft`` autograd
    restatement of the same loss on the same inputs."""
    import torch
    from diffwave_sashimi_amd import metrics
    from tests import spectral_reference as ref
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(1)
    y = (torch.randn(args.batch, args.samples, generator=gen) * 0.1).to(dev)
    x = (y + (torch.randn(args.batch, args.samples, generator=gen) * 0.02).to(dev)).requires_grad_(True)
    res = metrics.MR_STFT_RESOLUTIONS

    def kernel(backward=True):
        x.grad = None
        out = metrics.mr_stft_loss(x, y).sum()
        if backward:
            out.backward()
        return x.grad

    def restated():
        x.grad = None
        total = 0.0
        for n_fft, hop, win in res:
            px, py = ref.power(x, n_fft, hop, win, torch.float32), ref.power(y, n_fft, hop, win, torch.float32)
            mx, my = torch.sqrt(px.clamp_min(ref.FLOOR)), torch.sqrt(py.clamp_min(ref.FLOOR))
            sc = torch.sqrt(((my - mx) ** 2).sum(dim=(-2, -1)) / (my ** 2).sum(dim=(-2, -1)))
            total = total + sc + (torch.log(my) - torch.log(mx)).abs().mean(dim=(-2, -1))
        (total / len(res)).sum().backward()
        return x.grad

    f_ms, f_min, _ = timed(lambda: kernel(False))
    k_ms, k_min, k_grad = timed(kernel)
    k_grad = k_grad.clone()
    t_ms, t_min, t_grad = timed(restated)
    rel = float(torch.linalg.vector_norm((k_grad - t_grad).double()) / torch.linalg.vector_norm(t_grad.double()))
    print(json.dumps(dict(loss=True, B=args.batch, T=args.samples, resolutions=[list(r) for r in res],
                          kernel_forward_ms_median=round(f_ms, 3), kernel_forward_ms_min=round(f_min, 3),
                          kernel_forward_backward_ms_median=round(k_ms, 3), kernel_forward_backward_ms_min=round(k_min, 3),
                          torch_stft_f32_forward_backward_ms_median=round(t_ms, 3),
                          torch_stft_f32_forward_backward_ms_min=round(t_min, 3), gradient_rel_l2_diff=rel)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--loss", action="store_true", help="time metrics.mr_stft_loss forward + backward instead "
                    "(defaults then: --batch 32 --samples 16000)")
    args = ap.parse_args()
    if args.loss:
        args.batch = 32 if "--batch" not in sys.argv else args.batch
        args.samples = 16000 if "--samples" not in sys.argv else args.samples
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from diffwave_sashimi_amd import metrics
    from tests import spectral_reference as ref
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(1)
    y = (torch.randn(args.batch, args.samples, generator=gen) * 0.1).to(dev)
    x = y + (torch.randn(args.batch, args.samples, generator=gen) * 0.02).to(dev)
    stft = metrics.default_stft()
    basis = stft._tables(dev)[1]
    passes = [(r, None, 0) for r in metrics.MR_STFT_RESOLUTIONS] + \
             [((stft.filter_length, stft.hop_length, stft.win_length), basis, 13)]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), out

    if args.loss:
        loss_times(args, timed)
        return
    total_k = total_t = 0.0
    for (n_fft, hop, win), b, n_cep in passes:
        cep = metrics._cep(dev, n_cep, b.shape[0]) if n_cep else None
        k_ms, k_min, k_out = timed(lambda: metrics._run(x, y, None, n_fft, hop, win, b, cep))
        t_ms, t_min, t_out = timed(lambda: ref.sums(x, y, n_fft, hop, win, basis=b, n_cep=n_cep, dtype=torch.float32))
        cols = 6 if n_cep else 4
        rel = float(((k_out[:, :cols] - t_out[:, :cols].double()).abs() / t_out[:, :cols].double().abs()).max())
        total_k, total_t = total_k + k_ms, total_t + t_ms
        print(json.dumps(dict(n_fft=n_fft, hop=hop, win=win, mel=b is not None, B=args.batch, T=args.samples,
                              kernel_ms_median=round(k_ms, 3), kernel_ms_min=round(k_min, 3),
                              torch_stft_f32_ms_median=round(t_ms, 3), torch_stft_f32_ms_min=round(t_min, 3),
                              max_rel_diff=rel)), flush=True)
    print(json.dumps(dict(all_passes=True, kernel_ms=round(total_k, 3), torch_stft_f32_ms=round(total_t, 3),
                          audio_seconds_at_22050=round(args.batch * args.samples / 22050.0, 2))), flush=True)
    # the pitch pass ("Pitch metrics"): one dws_pitch_distance call at the defaults -- the YIN
    # tracks of x and y and the eight sums.  The same noise is unvoiced throughout; a tracker's time does not depend on
    # the decision (every lag of every frame is computed either way), so a second input with voiced frames is timed
    # only to show that.
    pd = metrics.PITCH_DEFAULTS
    lo, hi = metrics.pitch_lags(pd["sampling_rate"], pd["fmin"], pd["fmax"])
    run = lambda a, b: metrics._pitch_run(a, b, None, pd["sampling_rate"], pd["hop"], pd["win"], lo, hi, pd["threshold"])
    p_ms, p_min, p_out = timed(lambda: run(x, y))
    t = torch.arange(args.samples, device=dev, dtype=torch.float32) / pd["sampling_rate"]
    tone = 0.3 * torch.sin(2.0 * torch.pi * 140.0 * t).expand(args.batch, -1).contiguous()
    v_ms, v_min, v_out = timed(lambda: run(tone + 0.1 * x, tone))
    print(json.dumps(dict(pitch=True, B=args.batch, T=args.samples, **pd, lags=[lo, hi],
                          kernel_ms_median=round(p_ms, 3), kernel_ms_min=round(p_min, 3),
                          voiced_input_ms_median=round(v_ms, 3), voiced_input_ms_min=round(v_min, 3),
                          voiced_both_noise=float(p_out[:, 0].sum()), voiced_both_tone=float(v_out[:, 0].sum()))),
          flush=True)


if __name__ == "__main__":
    main()

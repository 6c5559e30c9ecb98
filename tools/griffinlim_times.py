"""Times of mel inversion ("Mel inversion"): ``TacotronSTFT.mel_to_audio`` on the engine against a
float32 ``torch.stft`` / ``torch.istft`` Griffin-Lim loop on the same GPU, from the same log-mel.

    python tools/griffinlim_times.py [--batch 16] [--seconds 116] [--iters 32] [--momentum 0] [--repeats 10]

The workload is ``--batch`` clips that hold ``--seconds`` of audio in all at 22050 Hz, 1024 / 256 / 1024, 80 bands.  Every
figure is the median (and the smallest and largest) over --repeats of the time between two events around the call, after a
warm-up call; both sides start from the mel and include the pseudo-inverse product and the draw of the phases.  One JSON
line per measurement, and the spectral convergence both reach (so that the two loops are seen to do the same work).
"""
import argparse
import json
import math
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=116.0)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--momentum", type=float, default=0.0)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from diffwave_sashimi_amd.mel import TacotronSTFT
    dev = torch.device("cuda")
    stft = TacotronSTFT()
    n_fft, hop, sr = stft.filter_length, stft.hop_length, stft.sampling_rate
    B, N, alpha = args.batch, args.iters, args.momentum
    frames = int(round(args.seconds * sr / B / hop)) + 1
    T = (frames - 1) * hop
    y = (torch.rand(B, T, generator=torch.Generator().manual_seed(1)) * 0.6 - 0.3).to(dev)
    mel = stft.mel_spectrogram(y)
    win = stft.window.to(dev)

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
        return round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)

    def torch_loop():
        mag = stft.mel_to_magnitude(mel)
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        phase = (torch.rand(mag.shape, device=dev, generator=g) * 2.0 - 1.0) * math.pi
        x = torch.istft(torch.polar(mag, phase), n_fft, hop_length=hop, window=win, center=True)
        prev = x
        for _ in range(N):
            X = torch.stft(x if alpha == 0.0 else x + alpha * (x - prev), n_fft, hop_length=hop, window=win, center=True,
                           pad_mode="reflect", return_complex=True)
            prev = x
            x = torch.istft(torch.polar(mag, torch.angle(X)), n_fft, hop_length=hop, window=win, center=True)
        return x

    def convergence(x):
        mag = stft.mel_to_magnitude(mel).double()
        X = torch.stft(x.double(), n_fft, hop_length=hop, window=win.double(), center=True, pad_mode="reflect",
                       return_complex=True).abs()
        return float(torch.linalg.norm(X - mag) / torch.linalg.norm(mag))

    shape = dict(B=B, frames=frames, samples=T, seconds=round(B * T / sr, 2), n_fft=n_fft, hop=hop, n_iters=N, momentum=alpha)
    ours = timed(lambda: stft.mel_to_audio(mel, n_iters=N, momentum=alpha))
    print(json.dumps(dict(run="engine mel_to_audio", ms_median=ours[0], ms_min=ours[1], ms_max=ours[2],
                          convergence=round(convergence(stft.mel_to_audio(mel, n_iters=N, momentum=alpha)), 5), **shape)),
          flush=True)
    theirs = timed(torch_loop)
    print(json.dumps(dict(run="torch.stft / torch.istft loop", ms_median=theirs[0], ms_min=theirs[1], ms_max=theirs[2],
                          convergence=round(convergence(torch_loop()), 5), **shape)), flush=True)
    print(json.dumps(dict(run="engine over torch", time_ratio=round(ours[0] / theirs[0], 3))), flush=True)


if __name__ == "__main__":
    main()

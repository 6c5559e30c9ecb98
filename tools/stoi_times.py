"""Times of the intelligibility metrics ("Intelligibility metrics"): the sample-rate converter, the
STOI / ESTOI kernels at 10 kHz, and the whole ``metrics.stoi`` pass.

    python tools/stoi_times.py [--batch 16] [--samples 160000] [--sampling-rate 22050] [--repeats 20]

Every figure is the median (and the smallest and largest) over --repeats of the time between two events around the call,
after a warm-up call; everything runs in one process on one GPU on seeded noise (stationary: no frame is silent, so every
frame is transformed -- the most work a clip of that length can be).  One JSON line per measurement:

* ``copy``: a device copy of the B x T floats, the least a pass over the input can take.
* ``resample``: ``audio.resample`` (one ``dws_resample`` launch, table cached, output allocation included) from
  --sampling-rate to 10 kHz, and for the table-layout notes 16000 -> 10000 (5/8, 161 taps) and 16000 -> 22050 (441/320,
  8821 taps) at the same B x T.
* ``stoi_kernels``: one ``dws_stoi`` call on the converted batch (five launches, workspace allocation included, no copy to
  the host).
* ``stoi``: the whole ``metrics.stoi(x, y)`` -- two conversions, ``dws_stoi``, the copy of [B, 4] doubles to the host and
  the divisions there.
"""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--sampling-rate", type=int, default=22050)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from diffwave_sashimi_amd import audio, metrics
    dev = torch.device("cuda")
    B, T, sr = args.batch, args.samples, args.sampling_rate
    gen = torch.Generator().manual_seed(1)
    y = (torch.randn(B, T, generator=gen) * 0.1).to(dev)
    x = y + (torch.randn(B, T, generator=gen) * 0.02).to(dev)

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
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4)), out

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    dst = torch.empty_like(x)
    t, _ = timed(lambda: dst.copy_(x))
    emit(kernel="copy", B=B, T=T, bytes=2 * 4 * B * T, **t)
    for a, b in ((sr, 10000), (16000, 10000), (16000, 22050)):
        U, D, h = audio.resample_filter(a, b)
        t, (out, _) = timed(lambda: audio.resample(x, a, b))
        emit(kernel="resample", sr_in=a, sr_out=b, U=U, D=D, taps=len(h), B=B, T=T, T_out=int(out.shape[1]),
             products_per_output=round(len(h) / U, 1), **t)
    x10, _ = audio.resample(x, sr, 10000)
    y10, _ = audio.resample(y, sr, 10000)
    t, out = timed(lambda: metrics._stoi_run(x10, y10, None))
    emit(kernel="stoi_kernels", B=B, T=int(x10.shape[1]), frames_kept=out[:, 3].tolist()[:2], segments=out[:, 2].tolist()[:2], **t)
    t, out = timed(lambda: metrics.stoi(x, y, sampling_rate=sr))
    emit(call="metrics.stoi", B=B, T=T, sampling_rate=sr, audio_seconds=round(B * T / sr, 2),
         stoi=round(float(out["stoi"][0]), 6), estoi=round(float(out["estoi"][0]), 6), **t)


if __name__ == "__main__":
    main()

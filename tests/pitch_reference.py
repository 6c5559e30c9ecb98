"""float64 numpy restatement of the pitch tracker (``dws_pitch_track`` / ``dws_pitch_distance``, include/dws.h) and the
signals its tests run on.  Nothing here touches the engine.

Definitions (sr, hop, W = win, theta = threshold as the float32 it travels as; tau_lo = floor(sr / fmax),
tau_hi = ceil(sr / fmin), M = tau_hi + 1, S = W + M; rho the reflect map about the clip's own ends):

    u_f[i] = s[rho(f hop - S // 2 + i)]                       i = 0 .. S - 1,  f = 0 .. len // hop
    d(tau)  = sum_{j < W} (u_f[j] - u_f[j + tau])^2           tau = 1 .. M,  d(0) = 0
    d'(tau) = d(tau) tau / sum_{t = 1 .. tau} d(t)            (1 where the sum is 0; d'(0) = 1)

the smallest tau in [tau_lo, tau_hi] with d'(tau) < theta, then tau <- tau + 1 while tau + 1 <= tau_hi and
d'(tau + 1) < d'(tau); voiced: f0 = sr / (tau* + delta) with the parabola through d'(tau* - 1 .. tau* + 1)
(delta = 0 unless a - 2b + c > 0 and |delta| <= 1), p = clamp(1 - d'(tau*), 0, 1); unvoiced: f0 = 0,
p = clamp(1 - min d', 0, 1).
"""
import math

import numpy as np

# the three parameter sets of tests/test_pitch_gpu.py: (A) more lags than one 256-thread pass, (B) W no multiple of 64 and
# M no multiple of 4, (C) the largest window and more than 512 lags
PARAMS = {
    "A": dict(sampling_rate=22050, hop=256, win=1024, fmin=50.0, fmax=550.0, threshold=0.15),
    "B": dict(sampling_rate=8000, hop=80, win=200, fmin=80.0, fmax=800.0, threshold=0.15),
    "C": dict(sampling_rate=22050, hop=256, win=2048, fmin=40.0, fmax=550.0, threshold=0.15),
}
SAMPLES = {"A": 16640, "B": 6400, "C": 20480}      # 66, 81 and 81 frames
SEEDS = {"A": 1, "B": 2, "C": 3}
MARGIN = 1e-5               # frames whose decision margin is below this are left out of frame-wise comparisons
LEFT_OUT_CAP = 0.05         # at most this share of a case's frames


def lags(sampling_rate, fmin, fmax):
    return int(math.floor(sampling_rate / fmax)), int(math.ceil(sampling_rate / fmin))


def frame_size(sampling_rate=22050, hop=256, win=1024, fmin=50.0, fmax=550.0, threshold=0.15):
    """S = W + M."""
    return win + lags(sampling_rate, fmin, fmax)[1] + 1


def min_samples(**params):
    """(S + 1) // 2 + 1: the shortest clip reflect padding admits."""
    return (frame_size(**params) + 1) // 2 + 1


def track(s, sampling_rate=22050, hop=256, win=1024, fmin=50.0, fmax=550.0, threshold=0.15):
    """Per frame ``(f0, p, voiced, margin)`` of the 1-D signal ``s`` (its own length is the clip's), float64.  ``margin``
    is the smallest |difference| over every comparison made for the frame: ``d'(tau) < theta`` from tau_lo to the first
    crossing (the whole range on an unvoiced frame), every ``d'(tau + 1) < d'(tau)`` of the walk and the one that
    stopped it."""
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[0]
    tau_lo, tau_hi = lags(sampling_rate, fmin, fmax)
    M = tau_hi + 1
    S = win + M
    assert n >= (S + 1) // 2 + 1
    theta = float(np.float32(threshold))
    frames = n // hop + 1
    f0, per, voiced, margin = (np.zeros(frames) for _ in range(4))
    taus = np.arange(1, M + 1, dtype=np.float64)
    for f in range(frames):
        j = f * hop - S // 2 + np.arange(S)
        j = np.where(j < 0, -j, j)
        j = np.where(j >= n, 2 * (n - 1) - j, j)
        u = s[j]
        rows = np.lib.stride_tricks.sliding_window_view(u, win)          # rows[tau] = u[tau : tau + W]
        d = ((rows[1:M + 1] - rows[0]) ** 2).sum(axis=1)                 # d(1 .. M)
        cum = np.cumsum(d)
        dp = np.ones(M + 1)
        nz = cum != 0
        dp[1:][nz] = d[nz] * taus[nz] / cum[nz]
        search = dp[tau_lo:tau_hi + 1]
        below = np.nonzero(search < theta)[0]
        if below.size == 0:
            margin[f] = np.abs(search - theta).min()
            per[f] = min(max(1.0 - search.min(), 0.0), 1.0)
            continue
        t = tau_lo + int(below[0])
        m = np.abs(dp[tau_lo:t + 1] - theta).min()
        while t + 1 <= tau_hi:
            m = min(m, abs(dp[t + 1] - dp[t]))
            if not dp[t + 1] < dp[t]:
                break
            t += 1
        a, b, c = dp[t - 1], dp[t], dp[t + 1]
        den = a - 2.0 * b + c
        delta = 0.0
        if den > 0.0:
            delta = 0.5 * (a - c) / den
            if not abs(delta) <= 1.0:
                delta = 0.0
        f0[f] = sampling_rate / (t + delta)
        per[f] = min(max(1.0 - b, 0.0), 1.0)
        voiced[f] = 1.0
        margin[f] = m
    return f0, per, voiced.astype(bool), margin


def sums(f0x, px, f0y, py, frames=None):
    """The eight sums of ``dws_pitch_distance`` from two tracks (their first ``frames`` frames), float64."""
    frames = len(f0x) if frames is None else frames
    f0x, px, f0y, py = (np.asarray(v, dtype=np.float64)[:frames] for v in (f0x, px, f0y, py))
    vx, vy = f0x > 0, f0y > 0
    vv = vx & vy
    out = np.zeros(8)
    for f in range(frames):                 # ascending, as the kernel adds
        if vv[f]:
            out[1] += (f0x[f] - f0y[f]) ** 2
            out[2] += (1200.0 * np.log2(f0x[f] / f0y[f])) ** 2
            out[7] += abs(f0x[f] / f0y[f] - 1.0) > 0.2
        out[6] += (px[f] - py[f]) ** 2
    out[0], out[3], out[4], out[5] = vv.sum(), vy.sum(), vx.sum(), (vx != vy).sum()
    return out


def metrics_from_sums(s, frames):
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"f0_rmse": np.sqrt(s[1] / s[0]), "f0_cents": np.sqrt(s[2] / s[0]), "gpe": s[7] / s[0],
                "vuv_error": s[5] / frames, "vuv_f1": 2.0 * s[0] / (s[3] + s[4]), "periodicity_rmse": np.sqrt(s[6] / frames)}


# ---- signals
def tone(n, f0, sr, rng, vibrato=0.0, phases=None):
    """Six harmonics of ``f0`` (amplitudes 1 / h, random phases), peak about 0.3; ``vibrato``: the relative depth of a
    5 Hz frequency modulation."""
    t = np.arange(n) / sr
    phase = 2.0 * np.pi * f0 * (t - vibrato / (2.0 * np.pi * 5.0) * (np.cos(2.0 * np.pi * 5.0 * t) - 1.0))
    phases = rng.uniform(0.0, 2.0 * np.pi, 6) if phases is None else phases
    out = sum(np.sin(h * phase + phases[h - 1]) / h for h in range(1, 7))
    return 0.12 * out, phases


def tone_f0s(fmin, fmax):
    """Three fundamentals inside [fmin, fmax], at 0.2, 0.4 and 0.6 of the range on a log scale."""
    return [fmin * (fmax / fmin) ** q for q in (0.2, 0.4, 0.6)]


def signal_pair(name, seed=None, samples=None):
    """``(x, y, segments)`` of parameter set ``name``: float32 arrays [samples]; y is six equal segments -- a steady
    tone, white noise, a second tone, digital silence, a vibrato tone (5 Hz, +-3 %), a third tone -- the tones with a
    little noise, and x = 0.9 y + 0.01 noise with the first segment detuned by 2.5 %.  ``segments``: (start, end, kind,
    f0) with kind in tone / noise / silence / vibrato."""
    p = PARAMS[name]
    sr = p["sampling_rate"]
    n = SAMPLES[name] if samples is None else samples
    rng = np.random.default_rng(SEEDS[name] if seed is None else seed)
    fa, fb, fc = tone_f0s(p["fmin"], p["fmax"])
    kinds = [("tone", fa), ("noise", 0.0), ("tone", fb), ("silence", 0.0), ("vibrato", fb), ("tone", fc)]
    edges = [round(k * n / len(kinds)) for k in range(len(kinds) + 1)]
    y = np.zeros(n)
    x_first = None
    segments = []
    for (kind, f0), a, b in zip(kinds, edges[:-1], edges[1:]):
        m = b - a
        if kind in ("tone", "vibrato"):
            seg, phases = tone(m, f0, sr, rng, vibrato=0.03 if kind == "vibrato" else 0.0)
            little = 1e-3 * rng.standard_normal(m)
            if a == 0:
                x_first = tone(m, 1.025 * f0, sr, rng, phases=phases)[0] + little
            seg = seg + little
        elif kind == "noise":
            seg = 0.1 * rng.standard_normal(m)
        else:
            seg = np.zeros(m)
        y[a:b] = seg
        segments.append((a, b, kind, f0))
    x = y.copy()
    x[:edges[1]] = x_first
    x = 0.9 * x + 0.01 * rng.standard_normal(n)
    return x.astype(np.float32), y.astype(np.float32), segments


def frames_inside(segment, hop, S, frames):
    """The frames whose S samples lie wholly inside ``segment`` = (start, end, ...)."""
    a, b = segment[0], segment[1]
    return [f for f in range(frames) if f * hop - S // 2 >= a and f * hop - S // 2 + S <= b]


_cache = {}


def reference_tracks(name):
    """``(x, y, segments, track(x), track(y))`` of set ``name``, computed once and shared; treat as read-only."""
    if name not in _cache:
        x, y, seg = signal_pair(name)
        _cache[name] = (x, y, seg, track(x, **PARAMS[name]), track(y, **PARAMS[name]))
    return _cache[name]

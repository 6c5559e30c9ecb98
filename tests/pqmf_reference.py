"""A numpy float64 restatement of the PQMF filter bank (``diffwave_sashimi_amd/pqmf.py``, ``dws_pqmf_analysis`` /
``dws_pqmf_synthesis`` of include/dws.h) as plain loops over the taps: the three design formulas, the two sums and
their transposes written out from the definitions.  Besides each result the sums return, per output,
``A = sum |filt . input|`` (the sum of the absolute products) and the number of products ``terms``: what the
rounding-error bound of the GPU tests is made of."""
import numpy as np


def prototype(taps=62, cutoff=0.142, beta=9.0):
    """h[n] = c sinc(c (n - taps/2)) kaiser(taps + 1, beta)[n], n = 0 .. taps, normalised to sum 1."""
    w = np.kaiser(taps + 1, beta)
    h = np.array([cutoff * np.sinc(cutoff * (n - taps / 2)) * w[n] for n in range(taps + 1)], dtype=np.float64)
    return h / h.sum()


def design(K=4, taps=62, cutoff=0.142, beta=9.0):
    """(ha, hs) [K, taps + 1]: 2 h[n] cos((2k + 1) pi / (2K) (n - taps/2) +- (-1)^k pi/4)."""
    h = prototype(taps, cutoff, beta)
    ha = np.zeros((K, taps + 1))
    hs = np.zeros((K, taps + 1))
    for k in range(K):
        for n in range(taps + 1):
            arg = (2 * k + 1) * np.pi / (2 * K) * (n - taps / 2)
            ha[k, n] = 2 * h[n] * np.cos(arg + (-1) ** k * np.pi / 4)
            hs[k, n] = 2 * h[n] * np.cos(arg - (-1) ** k * np.pi / 4)
    return ha, hs


def analysis(x, filt, gain=1.0):
    """out[b, k, t] = gain sum_n filt[k, n] x[b, K t + n - taps/2], x zero outside [0, T).  x [B, T] ->
    (out, A, terms), each [B, K, T/K]; a product with a position outside the clip is no term."""
    x = np.asarray(x, dtype=np.float64)
    filt = np.asarray(filt, dtype=np.float64)
    B, T = x.shape
    K, ntap = filt.shape
    half = (ntap - 1) // 2
    Ts = T // K
    out, A, terms = np.zeros((B, K, Ts)), np.zeros((B, K, Ts)), np.zeros((B, K, Ts))
    t = np.arange(Ts)
    for n in range(ntap):                                   # n ascending, every output at once
        p = K * t + n - half
        ok = (p >= 0) & (p < T)
        prod = filt[None, :, n, None] * x[:, None, p[ok]]               # [B, K, #ok]
        out[:, :, ok] += gain * prod
        A[:, :, ok] += abs(gain) * np.abs(prod)
        terms[:, :, ok] += 1
    return out, A, terms


def synthesis(s, filt, gain=1.0):
    """out[b, u] = gain sum_k sum_n filt[k, n] s[b, k, q] over the n with u + n - taps/2 = K q, 0 <= q < Ts.
    s [B, K, Ts] -> (out, A, terms), each [B, K Ts]."""
    s = np.asarray(s, dtype=np.float64)
    filt = np.asarray(filt, dtype=np.float64)
    B, K, Ts = s.shape
    ntap = filt.shape[1]
    half = (ntap - 1) // 2
    T = K * Ts
    out, A, terms = np.zeros((B, T)), np.zeros((B, T)), np.zeros((B, T))
    u = np.arange(T)
    for n in range(ntap):
        p = u + n - half
        ok = (p % K == 0) & (p >= 0) & (p // K < Ts)
        prod = filt[None, :, n, None] * s[:, :, p[ok] // K]             # [B, K, #ok]
        out[:, ok] += gain * prod.sum(1)
        A[:, ok] += abs(gain) * np.abs(prod).sum(1)
        terms[:, ok] += K
    return out, A, terms


def analysis_transpose(w, filt, gain=1.0):
    """The transpose of ``analysis(., filt, gain)`` applied to w [B, K, Ts], written out from the definition:
    dx[b, p] = gain sum_k sum_t filt[k, p - K t + taps/2] w[b, k, t].  -> (dx, A, terms), each [B, K Ts]."""
    w = np.asarray(w, dtype=np.float64)
    filt = np.asarray(filt, dtype=np.float64)
    B, K, Ts = w.shape
    ntap = filt.shape[1]
    half = (ntap - 1) // 2
    T = K * Ts
    dx, A, terms = np.zeros((B, T)), np.zeros((B, T)), np.zeros((B, T))
    t = np.arange(Ts)
    for n in range(ntap):
        p = K * t + n - half                                # (distinct positions: one scatter per n)
        ok = (p >= 0) & (p < T)
        prod = filt[None, :, n, None] * w[:, :, ok]
        dx[:, p[ok]] += gain * prod.sum(1)
        A[:, p[ok]] += abs(gain) * np.abs(prod).sum(1)
        terms[:, p[ok]] += K
    return dx, A, terms


def synthesis_transpose(v, filt, K, gain=1.0):
    """The transpose of ``synthesis(., filt, gain)`` applied to v [B, T]:
    ds[b, k, q] = gain sum_n filt[k, n] v[b, K q - n + taps/2].  -> (ds, A, terms), each [B, K, T/K]."""
    v = np.asarray(v, dtype=np.float64)
    filt = np.asarray(filt, dtype=np.float64)
    B, T = v.shape
    ntap = filt.shape[1]
    half = (ntap - 1) // 2
    Ts = T // K
    ds, A, terms = np.zeros((B, K, Ts)), np.zeros((B, K, Ts)), np.zeros((B, K, Ts))
    q = np.arange(Ts)
    for n in range(ntap):
        u = K * q - n + half
        ok = (u >= 0) & (u < T)
        prod = filt[None, :, n, None] * v[:, None, u[ok]]
        ds[:, :, ok] += gain * prod
        A[:, :, ok] += abs(gain) * np.abs(prod)
        terms[:, :, ok] += 1
    return ds, A, terms


def round_trip_error(K, cutoff, taps=62, beta=9.0, n=1024, seed=0, edge=64):
    """Relative L2 error of synthesis(analysis(x)) against x on the interior [edge : -edge] of n seeded white-noise
    samples, in float64 (the forward synthesis bank has gain K)."""
    x = np.random.default_rng(seed).standard_normal((1, n))
    ha, hs = design(K, taps, cutoff, beta)
    y = synthesis(analysis(x, ha)[0], hs, gain=float(K))[0]
    d = (y - x)[0, edge:-edge]
    return float(np.sqrt((d * d).sum() / (x[0, edge:-edge] ** 2).sum()))

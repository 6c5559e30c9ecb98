"""Float64 Adam / EMA / global-norm clipping written out in numpy, the fp32 CPU baseline (``torch.optim.Adam(foreach=False)``
+ ``lerp_`` + ``clip_grad_norm_``) that prices the error bound, and the fixed recipe of the fused-step tests."""
import numpy as np
import torch

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def recipe_sizes(chunk):
    return [1, 3, 4, 5, 1023, 1025, chunk - 1, chunk, chunk + 1, 3 * chunk + 5]


def recipe(chunk, steps=20, seed=0, zeros_in=6, n_zeros=100):
    """Initial parameters ``0.1 N(0,1)`` and ``steps`` gradient lists ``N(0,1) 10^((k mod 5) - 3)`` (fp32 numpy), with
    ``n_zeros`` exact zeros at fixed positions of tensor ``zeros_in`` in every step."""
    g = torch.Generator().manual_seed(seed)
    sizes = recipe_sizes(chunk)
    params = [(0.1 * torch.randn(n, generator=g)).numpy() for n in sizes]
    grads = []
    for k in range(steps):
        gs = [(torch.randn(n, generator=g) * 10.0 ** ((k % 5) - 3)).numpy() for n in sizes]
        gs[zeros_in][17:17 + n_zeros] = 0.0
        grads.append(gs)
    return sizes, params, grads


class AdamPair:
    """The float64 reference and the fp32 CPU baseline of one run, stepped together on the same fp32 gradients.

    ``lrs`` is the learning rate of every tensor (tensors of one rate form one torch param group).  ``ema_decay`` /
    ``max_norm`` as in ``EngineAdam``.  After the steps, ``check(name, got)`` holds ``got`` (list of fp32 arrays) against
    the float64 values of ``name`` in {p, m, v, ema} with the bound
        max |got - f64| <= 2 max |baseline - f64| + ulp32(max |f64|)."""

    def __init__(self, params, lrs, ema_decay=None, max_norm=None, weight_decay=0.0):
        self.lrs, self.d, self.max_norm, self.wd = list(lrs), ema_decay, max_norm, weight_decay
        self.p = [np.asarray(x, dtype=np.float64).copy() for x in params]
        self.m = [np.zeros_like(x) for x in self.p]
        self.v = [np.zeros_like(x) for x in self.p]
        self.ema = [x.copy() for x in self.p]
        self.t = 0
        self.norms = []          # float64 norm of every step's fp32 gradients
        self.tp = [torch.nn.Parameter(torch.from_numpy(np.asarray(x, dtype=np.float32).copy())) for x in params]
        groups = [{"params": [p for p, l in zip(self.tp, self.lrs) if l == lr], "lr": lr} for lr in sorted(set(self.lrs))]
        self.opt = torch.optim.Adam(groups, lr=1.0, betas=(BETA1, BETA2), eps=EPS, weight_decay=weight_decay, foreach=False)
        self.tema = [p.detach().clone() for p in self.tp]

    def step(self, grads):
        grads = [np.asarray(g, dtype=np.float32) for g in grads]
        self.t += 1
        t = self.t
        norm = float(np.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in grads)))
        self.norms.append(norm)
        coef = 1.0 if self.max_norm is None else min(1.0, self.max_norm / (norm + 1e-6))
        for i, g in enumerate(grads):
            g = g.astype(np.float64) * coef
            if self.wd:
                g = g + self.wd * self.p[i]
            self.m[i] += (g - self.m[i]) * (1.0 - BETA1)
            self.v[i] = BETA2 * self.v[i] + (1.0 - BETA2) * g * g
            step_size = self.lrs[i] / (1.0 - BETA1 ** t)
            self.p[i] -= step_size * self.m[i] / (np.sqrt(self.v[i]) / np.sqrt(1.0 - BETA2 ** t) + EPS)
            if self.d is not None:
                self.ema[i] = self.d * self.ema[i] + (1.0 - self.d) * self.p[i]
        # the fp32 baseline, as a stock training loop would run it
        for p, g in zip(self.tp, grads):
            p.grad = torch.from_numpy(g.copy())
        if self.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(self.tp, self.max_norm, foreach=False)
        self.opt.step()
        if self.d is not None:
            with torch.no_grad():
                for e, p in zip(self.tema, self.tp):
                    e.lerp_(p, 1.0 - self.d)

    def _baseline(self, name):
        if name == "p":
            return [p.detach().numpy() for p in self.tp]
        if name == "ema":
            return [e.numpy() for e in self.tema]
        key = {"m": "exp_avg", "v": "exp_avg_sq"}[name]
        return [self.opt.state[p][key].numpy() for p in self.tp]

    def errors(self, name, got):
        """(error of ``got``, error of the fp32 baseline, one fp32 ulp of the largest magnitude), all max-abs vs float64."""
        ref = getattr(self, name)
        err = max(float(np.max(np.abs(np.asarray(a, dtype=np.float64) - r))) for a, r in zip(got, ref))
        base = max(float(np.max(np.abs(b.astype(np.float64) - r))) for b, r in zip(self._baseline(name), ref))
        ulp = float(np.spacing(np.float32(max(float(np.max(np.abs(r))) for r in ref))))
        return err, base, ulp

    def check(self, name, got, what=""):
        err, base, ulp = self.errors(name, got)
        print(f"{what}{name}: max abs error {err:.3e}, fp32 torch baseline {base:.3e}, ulp {ulp:.3e}")
        assert err <= 2.0 * base + ulp, (what, name, err, base, ulp)

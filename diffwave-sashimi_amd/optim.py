"""``EngineAdam``: Adam on the engine's fused HIP step (``dws_optim_step``, ``csrc/optim_kernels.hip``).

One launch per step does what ``torch.optim.Adam`` does (``amsgrad=False``, ``maximize=False``, L2 ``weight_decay``)
and, in the same pass over the parameters,

* keeps an exponential moving average of the weights (``ema_decay``; ``ema_state_dict`` is what one samples from),
* writes the new parameters into the engine's raw store (``module=``), so the next forward's ``_sync_params`` has
  nothing to re-send (stock optimizers cost one ``dws_model_update_params`` pass over the model per step),
* scales the gradients by ``torch.nn.utils.clip_grad_norm_``'s coefficient (``max_grad_norm``; one more launch for the
  norm, which stays on the device: nothing waits for the GPU).  Unlike torch, ``p.grad`` is NOT rewritten: the scale is
  applied on the fly.

``state_dict()`` has ``torch.optim.Adam``'s layout (per-parameter ``step`` float32 scalar, ``exp_avg``,
``exp_avg_sq``; the same param-group keys), so a checkpoint of either optimizer loads into the other.  Construction and
the state-dict round trip work on CPU tensors; ``step()`` runs on the GPU only -- there is no fallback.
"""
import ctypes

import torch

from . import _lib

# torch.optim.Adam's param-group keys beyond (lr, betas, eps, weight_decay), at the only values the kernel implements
_ADAM_FIXED = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                   decoupled_weight_decay=False)


def _engine_module(module):
    """The ``EngineModule`` behind ``module`` (itself, or ``.module`` of a wrapper)."""
    from .models.engine import EngineModule
    for m in (module, getattr(module, "module", None)):
        if isinstance(m, EngineModule):
            return m
    raise TypeError(f"module= must be an EngineModule (WaveNet / Sashimi), got {type(module).__name__}")


class EngineAdam(torch.optim.Optimizer):
    """``EngineAdam(params_or_groups, lr, betas, eps, weight_decay, ema_decay=None, max_grad_norm=None, module=None)``.

    ``ema_decay`` d in (0, 1): a shadow of every parameter, started as a copy at construction (``reset_ema()`` copies
    again, e.g. after weights were loaded; a parameter that was written between such a copy and this optimizer's first step
    on it -- SaShiMi rewrites its S4 ``C`` at the first forward -- is copied again at that step; a shadow restored by
    ``load_ema_state_dict`` never is), updated every step as
    ``ema += (1 - d) (p_new - ema)``.  ``weight_g`` and
    ``weight_v`` of a weight-normed layer are averaged separately.  A parameter whose ``grad`` is None is skipped
    entirely, shadow included, as torch skips it.
    ``max_grad_norm`` c > 0: global L2-norm clipping over the parameters that have gradients; ``grad_norm`` is the norm
    of the last step as a 0-dim DEVICE tensor (reading it is what synchronises).
    ``module``: the network whose parameters these are; the step then also writes the engine's copy of every parameter
    and bumps the tensors' version counters, recording them in the module so that nothing is sent again.
    Parameters must be float32 and contiguous (checked here); betas and eps must agree across groups (checked in
    ``step``), lr and weight_decay are per group."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, ema_decay=None,
                 max_grad_norm=None, module=None):
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= float(eps):
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= float(betas[0]) < 1.0 and 0.0 <= float(betas[1]) < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= float(weight_decay):
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if ema_decay is not None and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay = {ema_decay!r} (needs 0 < d < 1)")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"max_grad_norm = {max_grad_norm!r} (needs c > 0)")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, **_ADAM_FIXED))
        for group in self.param_groups:
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise TypeError(f"EngineAdam takes float32 parameters, got {p.dtype} of shape {tuple(p.shape)}")
                if not p.is_contiguous():
                    raise ValueError(f"EngineAdam takes contiguous parameters, got strides {p.stride()} for shape "
                                     f"{tuple(p.shape)}")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._module = None if module is None else _engine_module(module)
        self._ema, self._ema_version = {}, {}      # shadows; the parameter's version counter when its shadow was last set
        if self.ema_decay is not None:
            self.reset_ema()
        self._handle = None
        self._grad_norm = None
        self._steps = None         # CPU float32 [n]: every state[p]["step"] is a 0-dim view of it (one add per step)
        self._step_index = {}
        self._table = None         # cached ctypes tables of the last step's tensor list

    # -- EMA -------------------------------------------------------------------
    def _params(self):
        return [p for group in self.param_groups for p in group["params"]]

    @torch.no_grad()
    def reset_ema(self):
        """Start the shadows over as a copy of the current parameters."""
        if self.ema_decay is None:
            raise RuntimeError("this EngineAdam keeps no EMA (ema_decay=None)")
        for p in self._params():
            s = self._ema.get(p)
            if s is None or s.device != p.device or s.shape != p.shape:
                self._ema[p] = p.detach().clone(memory_format=torch.contiguous_format)
            else:
                s.copy_(p.detach())
            self._ema_version[p] = p._version
        self._table = None

    def _module_or(self, module):
        if module is not None:
            return module
        if self._module is None:
            raise ValueError("no module: pass one, or construct EngineAdam with module=")
        return self._module

    @torch.no_grad()
    def ema_state_dict(self, module=None):
        """``module.state_dict()`` with every parameter this optimizer averages replaced by (a copy of) its shadow;
        buffers and everything else as the state_dict has them."""
        if self.ema_decay is None:
            raise RuntimeError("this EngineAdam keeps no EMA (ema_decay=None)")
        module = self._module_or(module)
        sd = module.state_dict()
        for name, p in module.named_parameters():
            s = self._ema.get(p)
            if s is not None and name in sd:
                sd[name] = s.detach().clone()
        return sd

    @torch.no_grad()
    def load_ema_state_dict(self, state_dict, module=None):
        """Restore the shadows from what ``ema_state_dict`` returned (entries that are no shadow are ignored)."""
        if self.ema_decay is None:
            raise RuntimeError("this EngineAdam keeps no EMA (ema_decay=None)")
        module = self._module_or(module)
        for name, p in module.named_parameters():
            s = self._ema.get(p)
            if s is None:
                continue
            if name not in state_dict:
                raise KeyError(f"the EMA state holds no '{name}'")
            src = state_dict[name]
            if tuple(src.shape) != tuple(s.shape):
                raise ValueError(f"EMA state '{name}' has shape {tuple(src.shape)}, the parameter {tuple(s.shape)}")
            s.copy_(src.to(device=s.device, dtype=s.dtype))
            self._ema_version.pop(p, None)       # a restored average is never replaced by a copy of the weights
        self._table = None

    # -- state -----------------------------------------------------------------
    @property
    def grad_norm(self):
        """Global gradient norm of the last clipped step: a 0-dim tensor on the device (None before it / without clipping)."""
        return None if self._grad_norm is None else self._grad_norm[0]

    def state_dict(self):
        sd = super().state_dict()
        # standalone scalars, exactly what torch.optim.Adam saves (new dicts: the packed state holds self.state's own, whose
        # steps must stay views of the one tensor step() advances)
        sd["state"] = {k: (dict(st, step=st["step"].clone()) if torch.is_tensor(st.get("step")) else dict(st))
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._steps, self._step_index, self._table = None, {}, None

    def _pack_steps(self):
        """Gather every per-parameter ``step`` into one CPU tensor and hand the state 0-dim views of it."""
        have = [p for p in self._params() if self.state.get(p)]     # (.get: indexing the defaultdict would insert empty states)
        vals = []
        for p in have:
            st = self.state[p]["step"]
            vals.append(float(st) if torch.is_tensor(st) else float(st))       # (a step on the GPU: read once)
        self._steps = torch.tensor(vals, dtype=torch.float32)
        self._step_index = {}
        for i, p in enumerate(have):
            self.state[p]["step"] = self._steps[i]
            self._step_index[p] = i

    def __del__(self):
        try:
            if getattr(self, "_handle", None) is not None and _lib._lib is not None:
                _lib._lib.dws_optim_destroy(self._handle)
        except Exception:
            pass

    # -- the step ----------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        active, lrs, wds = [], [], []
        hyper = None
        for group in self.param_groups:
            for k in ("amsgrad", "maximize", "decoupled_weight_decay"):     # (a state loaded from such a torch.optim.Adam)
                if group.get(k):
                    raise ValueError(f"EngineAdam does not implement {k}={group[k]!r}")
            h = (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]))
            lr, wd = float(group["lr"]), float(group["weight_decay"])
            for p in group["params"]:
                if p.grad is None:
                    continue
                if hyper is None:
                    hyper = h
                elif h != hyper:
                    raise ValueError(f"EngineAdam needs the same betas and eps in every param group (got {hyper} and {h})")
                active.append(p)
                lrs.append(lr)
                wds.append(wd)
        if not active:
            return loss
        dev = active[0].device
        if dev.type != "cuda":
            raise RuntimeError("EngineAdam.step runs on the GPU only: move the parameters to cuda (there is no CPU fallback)")
        lib = _lib.load()
        n = len(active)
        # The pointer tables of the last step are kept: per step and tensor the host only fetches the gradient's address
        # (a new tensor after every zero_grad) and checks that the parameter still lives where the table says.
        tab = self._table
        if tab is not None and tab["ids"] != [id(p) for p in active]:
            tab = None
        f32 = torch.float32
        for _ in range(2):
            if tab is None:
                tab = self._table = self._prepare(active, dev)
            P, G = tab["P"], tab["G"]
            moved = False
            for i, p in enumerate(active):
                g = p.grad
                if g.dtype is not f32 or g.is_sparse or g.device != dev or not g.is_contiguous():
                    raise RuntimeError(f"EngineAdam.step: gradients must be dense contiguous float32 on {dev} "
                                       f"(got {g.dtype} {tuple(g.shape)} strides {g.stride()} on {g.device})")
                G[i] = g.data_ptr()
                if P[i] != p.data_ptr():
                    moved = True
            if not moved:
                break
            tab = None              # a parameter's storage was replaced (p.data = ...): build the tables again
        steps = self._steps.tolist()        # (advanced only once the step has been enqueued: an error leaves them as they were)
        LR, T, WD = tab["LR"], tab["T"], tab["WD"]
        T[:] = [int(steps[k]) + 1 for k in tab["idx_list"]]
        LR[:] = lrs
        WD[:] = wds
        if self._handle is None:
            h = ctypes.c_void_p()
            _lib.check(lib.dws_optim_create(ctypes.byref(h)))
            self._handle = h
        norm_ptr = None
        if self.max_grad_norm is not None:
            if self._grad_norm is None or self._grad_norm.device != dev:
                self._grad_norm = torch.zeros(1, device=dev, dtype=torch.float32)
            norm_ptr = self._grad_norm.data_ptr()
        mod = self._module
        model = mod._ensure_handle() if (mod is not None and tab["mirrored"]) else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.dws_optim_step(self._handle, n, tab["P"], G, tab["M"], tab["V"], tab["E"], None, tab["N"], LR, T, WD,
                                      hyper[0], hyper[1], hyper[2], self.ema_decay or 0.0, self.max_grad_norm or 0.0,
                                      norm_ptr, model, tab["names"] if model is not None else None, stream))
        if tab["all_steps"]:
            self._steps.add_(1.0)
        else:
            self._steps[tab["idx"]] += 1.0
        if self._ema_version:               # from here on the shadows are averages, no longer copies that may be refreshed
            for p in active:
                self._ema_version.pop(p, None)
        # the kernel wrote the tensors behind autograd's back: bump the version counters (other observers see the write) ...
        torch.autograd.graph.increment_version(active)
        if model is not None:
            # ... and tell the module that the engine already holds exactly these versions: the next _sync_params sends nothing
            vers, sdev = mod._versions, str(dev)
            for p, name, shape in tab["mirror_meta"]:
                vers[name] = (p.data_ptr(), p._version, shape, sdev)
            mod._mel_key = mod._mel_ref = None      # conditioner terms depend on the weights (as _sync_params notes)
        return loss

    def _prepare(self, active, dev):
        """First step of these tensors (or after a load / a change of the set): create missing state, pack the step
        counters, check everything once, build the pointer tables."""
        fresh = False
        for p in active:
            if p.device != dev:
                raise RuntimeError("EngineAdam.step: all parameters and gradients must live on one device")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                fresh = True
            v = self._ema_version.get(p)
            if self.ema_decay is not None and v is not None and v != p._version:
                # written since the shadow was copied from it, and not stepped by this optimizer since (whether or not a
                # loaded Adam state exists): the average starts from what the parameter is now
                s = self._ema.get(p)
                if s is not None and s.device == dev and s.shape == p.shape:
                    s.copy_(p)
                else:
                    self._ema[p] = p.detach().clone(memory_format=torch.contiguous_format)
                self._ema_version[p] = p._version
        if fresh or self._steps is None or any(p not in self._step_index for p in active):
            self._pack_steps()
        return self._build_table(active, dev)

    def _build_table(self, active, dev):
        n = len(active)
        vp = ctypes.c_void_p * n
        tab = {"n": n, "active": list(active), "ids": [id(p) for p in active]}
        tab["P"] = vp(*[p.data_ptr() for p in active])
        tab["G"] = vp()
        tab["M"] = vp(*[self.state[p]["exp_avg"].data_ptr() for p in active])
        tab["V"] = vp(*[self.state[p]["exp_avg_sq"].data_ptr() for p in active])
        for p in active:
            for k in ("exp_avg", "exp_avg_sq"):
                t = self.state[p][k]
                if t.device != dev or t.dtype != torch.float32 or t.shape != p.shape or not t.is_contiguous():
                    raise RuntimeError(f"EngineAdam: state '{k}' must be contiguous float32 of the parameter's shape on {dev} "
                                       f"(got {t.dtype} {tuple(t.shape)} on {t.device})")
        tab["E"] = None
        if self.ema_decay is not None:
            for p in active:
                s = self._ema.get(p)
                if s is None or s.device != dev or s.shape != p.shape:       # the module moved after construction
                    base = p.detach() if s is None or s.shape != p.shape else s
                    self._ema[p] = base.to(device=dev, copy=True).contiguous()
            tab["E"] = vp(*[self._ema[p].data_ptr() for p in active])
        tab["N"] = (ctypes.c_int64 * n)(*[p.numel() for p in active])
        tab["T"] = (ctypes.c_int64 * n)()
        tab["LR"] = (ctypes.c_double * n)()
        tab["WD"] = (ctypes.c_double * n)()
        tab["idx_list"] = [self._step_index[p] for p in active]
        tab["idx"] = torch.tensor(tab["idx_list"], dtype=torch.long)
        tab["all_steps"] = sorted(tab["idx_list"]) == list(range(self._steps.numel()))
        # the engine's copy: parameters of the module the engine has already been handed with this shape
        names, meta = [None] * n, []
        if self._module is not None:
            name_of = {p: k for k, p in self._module.named_parameters()}
            known = self._module._versions
            for i, p in enumerate(active):
                name = name_of.get(p)
                old = known.get(name) if name is not None else None
                if old is not None and tuple(old[2]) == tuple(p.shape):
                    names[i] = name.encode()
                    meta.append((p, name, tuple(p.shape)))
        tab["names"] = (ctypes.c_char_p * n)(*names)
        tab["mirror_meta"] = meta
        tab["mirrored"] = bool(meta)
        # tensors of zero elements take no part
        if any(p.numel() == 0 for p in active):
            raise RuntimeError("EngineAdam: a parameter with zero elements")
        return tab

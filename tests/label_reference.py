"""Independent float64 reference of the class-conditional networks, built on the CPU oracle as it stands.

The label enters as ``e_b = swish(fc_t2(swish(fc_t1(emb(t_b))))) + table[y_b]`` and every block's ``fc_t`` is linear in
``e``.  So clip ``b`` of the labelled network equals the UNLABELLED oracle run on that clip alone with every
``*.fc_t.bias`` replaced by ``bias + fc_t.weight @ table[y_b]``: a per-clip loop, no change under ``oracle/``.  Autograd
through the folded biases gives the reference gradients of every parameter, the table included (``forward_batched``
folds the same biases for all clips in one oracle call, for the gradient tests of the larger cases).  ``cfg_loop`` is a
float64 classifier-free-guidance sampler over that oracle, written from the definition of each update."""
import numpy as np
import torch

from oracle import sashimi as osa
from oracle import wavenet as own
from tests import cases

K = 3                       # classes of the shared setup; row K of the table is the null class
LABELS = [1, 3, 1]          # a repeated class, the null class; classes 0 and 2 are absent
STEPS = [7.0, 120.0, 43.0]  # distinct steps per clip


def table_key(cfg):
    return "residual_layer.label_embedding.weight" if cfg["_name_"] == "wavenet" else "label_embedding.weight"


def class_cfg(cfg, k=K):
    return dict(cfg, n_classes=k)


def build(cfg, wseed, k=K, table_seed=4242):
    """Our module with ``n_classes = k``, seeded like ``cases.build_ours``, and an N(0, 1) table (``nn.Embedding``'s own
    initialisation, drawn from a generator of its own so that the other weights do not depend on it)."""
    net = cases.build_ours(class_cfg(cfg, k), wseed)
    if cfg["_name_"] == "sashimi":
        net._setup_C()      # the state_dict the oracle reads is the post-first-forward one (C~, L = l_max)
    with torch.no_grad():
        t = net.state_dict()[table_key(cfg)]
        t.copy_(torch.randn(t.shape, generator=torch.Generator().manual_seed(table_seed)))
    return net


def state(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def folded(sd, cfg, y):
    """``sd`` with every ``*.fc_t.bias`` replaced by ``bias + fc_t.weight @ table[y]`` (differentiable in all three)."""
    row = sd[table_key(cfg)][int(y)]
    out = dict(sd)
    for k in sd:
        if k.endswith(".fc_t.bias"):
            out[k] = sd[k] + sd[k[:-len("bias")] + "weight"] @ row
    return out


def forward(sd, cfg, audio, steps, labels, mel=None):
    """The labelled network on ``sd`` (any float dtype), clip by clip through the unlabelled oracle.  ``labels`` None =
    the null class for every clip.  ``mel``: [B or 1, 80, Tmel]."""
    fwd = own.wavenet_forward if cfg["_name_"] == "wavenet" else osa.sashimi_forward
    dtype = sd[table_key(cfg)].dtype
    n_null = sd[table_key(cfg)].shape[0] - 1
    B = audio.shape[0]
    labels = [n_null] * B if labels is None else [int(v) for v in labels]
    steps = torch.as_tensor(steps).reshape(B, 1)
    outs = []
    for b in range(B):
        m = None if mel is None else mel[b:b + 1 if mel.shape[0] > 1 else 1].to(dtype)
        outs.append(fwd(folded(sd, cfg, labels[b]), cfg, audio[b:b + 1].to(dtype), steps[b:b + 1], mel_spec=m))
    return torch.cat(outs, dim=0)


def forward_batched(sd, cfg, audio, steps, labels, mel=None):
    """``forward`` in ONE oracle call: every ``*.fc_t.bias`` becomes the [B, C] matrix ``bias + table[y] @ fc_t.weight^T``,
    which ``F.linear`` broadcasts over the clips.  The same folding, B times cheaper where the S4 kernels dominate (they do
    not depend on the clip); tests/test_class_conditional.py holds it to the per-clip loop, values and gradients."""
    fwd = own.wavenet_forward if cfg["_name_"] == "wavenet" else osa.sashimi_forward
    table = sd[table_key(cfg)]
    B = audio.shape[0]
    idx = torch.as_tensor([table.shape[0] - 1] * B if labels is None else [int(v) for v in labels])
    rows = table[idx]
    out = dict(sd)
    for k in sd:
        if k.endswith(".fc_t.bias"):
            out[k] = sd[k] + rows @ sd[k[:-len("bias")] + "weight"].t()
    m = None if mel is None else mel.to(table.dtype)
    return fwd(out, cfg, audio.to(table.dtype), torch.as_tensor(steps).reshape(B, 1), mel_spec=m)


def to64(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def grads(cfg, sd, loss_of, labels, dtype=torch.float64, batched=False):
    """Autograd of ``loss_of(net, dtype)`` (``tests/gradcheck.mse_training_loss``) through ``forward`` (``batched``:
    ``forward_batched``) on ``sd`` in ``dtype``: (loss, gradient of every float tensor as float64).  Classes absent from
    ``labels`` get exact zeros."""
    leaf = {k: (v.detach().clone().to(dtype).requires_grad_(True) if v.is_floating_point() else v.clone())
            for k, v in sd.items()}

    def net(inp, mel_spec=None):
        return (forward_batched if batched else forward)(leaf, cfg, inp[0], inp[1], labels, mel=mel_spec)

    loss = loss_of(net, dtype)
    loss.backward()
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double()
         for k, v in leaf.items() if v.is_floating_point() and v.requires_grad}
    return float(loss.detach()), g


def patched_forward(sd, cfg, audio, steps, labels):
    """The same network evaluated the other way: the whole batch at once through the oracle with its embedding MLP
    patched to add ``table[labels]`` (what the engine does).  Only used to check ``forward`` against."""
    table = sd[table_key(cfg)]
    idx = torch.as_tensor([int(v) for v in labels])
    orig = own.step_embedding_mlp

    def mlp(sd_, prefix, diffusion_steps, dim_in=128):
        return orig(sd_, prefix, diffusion_steps, dim_in) + table[idx]

    fwd = own.wavenet_forward if cfg["_name_"] == "wavenet" else osa.sashimi_forward
    mods = [own, osa]
    saved = [getattr(m, "step_embedding_mlp", None) for m in mods]
    try:
        for m in mods:
            if hasattr(m, "step_embedding_mlp"):
                m.step_embedding_mlp = mlp
        return fwd(sd, cfg, audio.to(table.dtype), torch.as_tensor(steps).reshape(-1, 1))
    finally:
        for m, f in zip(mods, saved):
            if f is not None:
                m.step_embedding_mlp = f


def cfg_loop(sd64, cfg, kind, net_steps, coef, x_T, noise, labels, scale):
    """Classifier-free guidance in float64, from the definitions: per step s = S-1 .. 0 the labelled and the null-class
    network on the same state, ``eps = eps_c + scale (eps_c - eps_u)``, then the update of ``kind`` ("ddpm": coef =
    alpha, alpha_bar, sigma; "ddim": k1 .. k5; "dpmpp2m": m1 .. m5).  ``noise`` [S, B, C, L] or None."""
    c = np.asarray(coef, dtype=np.float64)
    S = len(net_steps)
    x = x_T.double().clone()
    B = x.shape[0]
    hist = None
    with torch.no_grad():
        for s in range(S - 1, -1, -1):
            t = torch.full((B, 1), float(net_steps[s]))
            ec = forward(sd64, cfg, x, t, labels)
            eu = forward(sd64, cfg, x, t, None)
            eps = ec + scale * (ec - eu)
            z = None if noise is None else noise[s].double()
            if kind == "ddpm":
                al, ab, sg = c[0, s], c[1, s], c[2, s]
                x = (x - (1 - al) / np.sqrt(1 - ab) * eps) / np.sqrt(al)
                if s > 0:
                    x = x + sg * z
            elif kind == "ddim":
                u = (x - c[0, s] * eps) / c[1, s]
                x = c[2, s] * u + c[3, s] * eps
                if s > 0 and c[4, s] > 0:
                    x = x + c[4, s] * z
            else:
                x0 = (x - c[0, s] * eps) / c[1, s]
                D = x0
                if hist is not None and c[4, s] != 0:
                    D = x0 + c[4, s] * (x0 - hist)
                x = c[2, s] * x + c[3, s] * D
                hist = x0
    return x

"""GPU: class-conditional networks -- the label row added to the step embedding (forward, training forward, step
tables) and its adjoint, against the folded-bias float64 reference of tests/label_reference.py.

Shared setup: K = 3 classes, B = 3 clips with labels [1, 3, 1] (a repeated class, the null class, classes 0 and 2
absent), distinct steps per clip, an N(0, 1) table."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import cases
from tests import label_reference as lr
from tests.conftest import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

B = 3


def _case(name):
    """(cfg, L, weight seed, audio [B, 1, L], steps [B, 1], mel [B, 80, Tmel] | None)"""
    if name in cases.WAVENET_CASES:
        cfg, _, L, wseed, iseed, _ = cases.WAVENET_CASES[name]
        tmel = None
    elif name in cases.WAVENET_COND_CASES:
        cfg, _, L, tmel, wseed, iseed, _ = cases.WAVENET_COND_CASES[name]
    elif name in cases.SASHIMI_CASES:
        cfg, _, wseed, iseed, _ = cases.SASHIMI_CASES[name]
        L, tmel = cfg["L"], None
    else:
        cfg, _, tmel, wseed, iseed, _ = cases.SASHIMI_COND_CASES[name]
        L = cfg["L"]
    audio, _ = cases.wavenet_inputs(B, L, 1, iseed)
    steps = torch.tensor(lr.STEPS).reshape(B, 1)
    mel = None if tmel is None else cases.mel_inputs(B, tmel, iseed)
    return cfg, L, wseed, audio, steps, mel


def _reference(name):
    """float64 folded-bias forward of the case, computed once per session."""
    def make():
        cfg, L, wseed, audio, steps, mel = _case(name)
        sd = lr.to64(lr.state(lr.build(cfg, wseed)))
        with torch.no_grad():
            return lr.forward(sd, cfg, audio, steps, lr.LABELS, mel=None if mel is None else mel.double())
    return cases.cached(("label_forward64", name), make)


def _run(net, gpu, audio, steps, mel=None, labels=None):
    with torch.no_grad():
        return net((audio.to(gpu), steps.to(gpu)), mel_spec=None if mel is None else mel.to(gpu), labels=labels).cpu()


FORWARD = [("wn_tiny", "f32"), ("wn_c128", "f32"), ("wn_c128", "bf16x6"), ("wn_cond_tiny", "f32"), ("ss_tiny", "f32"),
           ("ss_d64_short", "f32"), ("ss_d64_short", "bf16x6"), ("ss_cond_tiny", "f32")]


@pytest.mark.parametrize("name,precision", FORWARD)
def test_labelled_forward_matches_the_folded_bias_reference(gpu, name, precision):
    cfg, L, wseed, audio, steps, mel = _case(name)
    net = lr.build(cfg, wseed).to(gpu)
    if precision != "f32":
        net.set_option("precision", precision)
    got = _run(net, gpu, audio, steps, mel, torch.tensor(lr.LABELS))
    ref = _reference(name)
    err = rel_err(got, ref)
    null = _run(net, gpu, audio, steps, mel, None)
    moved = rel_err(got, null)
    print(f"{name} {precision}: rel err {err:.3e}; labelled vs null output {moved:.2f}")
    assert err <= REL_TOL
    assert moved > 0.05                         # a label that is silently ignored fails here
    assert torch.equal(got[1], null[1])         # clip 1 carries the null class
    # labels=None is the all-null assignment, and labels hold no state across calls
    assert torch.equal(null, _run(net, gpu, audio, steps, mel, torch.full((B,), lr.K)))
    assert torch.equal(got, _run(net, gpu, audio, steps, mel, lr.LABELS))


@pytest.mark.parametrize("name", ["wn_tiny", "wn_c128", "ss_tiny"])
def test_zero_table_is_the_model_without_classes(gpu, name):
    """Same weights, a table of zeros, any labels: bit-equal to the model built without n_classes, in a forward and in a
    seeded 6-step sampler run."""
    from diffwave_sashimi_amd.models import construct_model
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling
    cfg, L, wseed, audio, steps, _ = _case(name)
    plain = cases.build_ours(cfg, wseed)
    net = construct_model(lr.class_cfg(cfg)).eval()
    missing = net.load_state_dict(plain.state_dict(), strict=False)
    assert missing.missing_keys == [lr.table_key(cfg)] and not missing.unexpected_keys
    with torch.no_grad():
        net.state_dict()[lr.table_key(cfg)].zero_()
    plain, net = plain.to(gpu), net.to(gpu)
    assert torch.equal(_run(plain, gpu, audio, steps), _run(net, gpu, audio, steps, labels=lr.LABELS))
    assert torch.equal(_run(plain, gpu, audio, steps), _run(net, gpu, audio, steps))
    dh = calc_diffusion_hyperparams(6, 1e-4, 0.05)
    a = sampling(plain, (B, 1, L), dh, seed=5)
    assert torch.equal(a, sampling(net, (B, 1, L), dh, seed=5, labels=lr.LABELS))
    assert torch.equal(a, sampling(net, (B, 1, L), dh, seed=5))


@pytest.mark.parametrize("name", ["wn_tiny", "wn_c128", "wn_cond_tiny", "ss_d64_short"])
def test_permuting_the_batch_permutes_the_outputs(gpu, name):
    cfg, L, wseed, audio, steps, mel = _case(name)
    net = lr.build(cfg, wseed).to(gpu)
    labels = torch.tensor(lr.LABELS)
    out = _run(net, gpu, audio, steps, mel, labels)
    for perm in ([2, 0, 1], [1, 2, 0]):
        p = torch.tensor(perm)
        got = _run(net, gpu, audio[p], steps[p], None if mel is None else mel[p], labels[p])
        assert torch.equal(got, out[p])


def _training_batch(cfg, L, T=50):
    """x_t, steps, z of one training step (``train.py:198-222``), drawn once; audio at the 0.3 scale of
    ``gradcheck.smooth_case``."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams
    from tests import gradcheck
    dh = calc_diffusion_hyperparams(T, 1e-4, 0.05)
    audio = torch.randn(B, 1, L, generator=torch.Generator().manual_seed(9)) * 0.3
    return gradcheck.mse_training_loss(audio, dh, None, generator=torch.Generator().manual_seed(21)), dh, audio


GRADS = [("wn_tiny", "f32"), ("wn_c128", "f32"), ("wn_c128", "bf16x6"), ("ss_tiny", "f32"), ("ss_d64_short", "f32")]


@pytest.mark.parametrize("name,precision", GRADS)
def test_gradients_of_every_parameter_and_the_table(gpu, name, precision):
    """The measure and bound of the training tests (tests/gradcheck.py): per tensor 1e-3 of its scale, widened to 3x the
    measured fp32 noise only for the known cancelling families.  The yardsticks are the helper's float64 autograd, its
    float32 autograd and its float64 autograd with the ReLU gates switched at +-2e-6."""
    from diffwave_sashimi_amd.training import training_loss
    from tests import gradcheck
    cfg, L, wseed, _, _, _ = _case(name)
    net = lr.build(cfg, wseed)
    loss_of, dh, audio = _training_batch(cfg, L)
    labels = lr.LABELS

    def yardsticks():       # once per case and session (the precisions share them); all clips in one oracle call
        sd = lr.state(net)
        loss64, truth = lr.grads(cfg, sd, loss_of, labels, torch.float64, batched=True)
        _, o32 = lr.grads(cfg, sd, loss_of, labels, torch.float32, batched=True)
        gmax = max(float(v.abs().max()) for v in truth.values())
        kink = {k: 0.0 for k in truth}
        for thr in (2e-6, -2e-6):
            with gradcheck._shifted_gates(thr):
                _, gp = lr.grads(cfg, sd, loss_of, labels, torch.float64, batched=True)
            for k in kink:
                kink[k] = max(kink[k], float((gp[k] - truth[k]).abs().max()) / gradcheck._scale(truth[k], gmax))
        return loss64, truth, o32, kink

    loss64, truth, o32, kink = cases.cached(("label_grads", name), yardsticks)

    net = net.to(gpu).train()
    if precision != "f32":
        net.set_option("precision", precision)
    x = audio.to(gpu).requires_grad_(True)
    loss = training_loss(net, nn.MSELoss(), x, dh, generator=torch.Generator().manual_seed(21), labels=torch.tensor(labels))
    loss.backward()
    got = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    tk = lr.table_key(cfg)
    assert tk in got and set(got) == set(truth)
    assert abs(float(loss.detach()) - loss64) < 1e-5 * max(1.0, abs(loss64))
    worst, k = gradcheck.compare(got, {k: o32[k] for k in got}, {k: truth[k] for k in got}, label=f"{name} {precision}",
                                 kink=kink)
    terr = gradcheck.errors({tk: got[tk]}, {tk: truth[tk]})[tk]
    print(f"{name} {precision}: worst parameter-gradient rel err {worst:.3e} ({k}); table {terr:.3e}")
    assert terr < REL_TOL
    assert float(truth[tk][1].abs().max()) > 0 and float(truth[tk][3].abs().max()) > 0
    for absent in (0, 2):       # classes absent from the batch: exactly zero, in the reference and in the engine
        assert float(truth[tk][absent].abs().max()) == 0.0
        assert float(got[tk][absent].abs().max()) == 0.0
    # the data-only pass (an eval() module: no parameter takes part) skips the table's kernel and yields the same bits
    full = x.grad.detach().clone()
    net.eval()
    for p in net.parameters():
        p.grad = None
    x2 = audio.to(gpu).requires_grad_(True)
    training_loss(net, nn.MSELoss(), x2, dh, generator=torch.Generator().manual_seed(21), labels=torch.tensor(labels)).backward()
    assert torch.equal(x2.grad, full)
    assert all(p.grad is None for p in net.parameters())


def _graphs(net):
    return int(net.read_tap("sampler_graphs", (1,)).item())


def _sampler_net(kind, gpu):
    if kind == "sashimi":
        cfg, L, wseed = cases.ss_cfg(d_model=32, n_layers=2, L=1024, diffusion_step_embed_dim_mid=64), 1024, 5
    else:       # wn_tiny: the generic layer (part_t strides); wn_c64: the MFMA / Winograd layer (correction-fragment strides)
        cfg, _, L, wseed, _, _ = cases.WAVENET_CASES[kind]
    return lr.build(cfg, wseed).to(gpu), L


@pytest.mark.parametrize("kind", ["wn_tiny", "wn_c64", "sashimi"])
def test_labelled_sampler_equals_the_loop_of_labelled_module_calls(gpu, kind):
    """Rows per (step, clip) of the labelled step table come from the row kernels of the per-clip forward: the trajectory
    equals -- bit for bit -- the loop `generate.py:49-54` written out with labelled module calls; graph equals eager; a
    second label set replays the captured graph."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling
    net, L = _sampler_net(kind, gpu)
    T = 6
    dh = calc_diffusion_hyperparams(T, 1e-4, 0.05)
    g = torch.Generator().manual_seed(77)
    x_T, noise = torch.randn(B, 1, L, generator=g), torch.randn(T, B, 1, L, generator=g)
    al, ab, sg = (dh[k] for k in ("Alpha", "Alpha_bar", "Sigma"))

    def loop(labels):
        # the update in numpy float32 on the host, each operation rounded once (tests/test_sampler_gpu.py)
        x = x_T.numpy().copy()
        with torch.no_grad():
            for t in range(T - 1, -1, -1):
                eps = net((torch.from_numpy(x).to(gpu), torch.full((B, 1), float(t), device=gpu)), labels=labels).cpu().numpy()
                a_t, ab_t = np.float32(al[t]), np.float32(ab[t])
                c1 = (np.float32(1) - a_t) / np.sqrt(np.float32(1) - ab_t)
                x = (x - c1 * eps) / np.sqrt(a_t)
                if t > 0:
                    x = x + np.float32(sg[t]) * noise[t].numpy()
        return torch.from_numpy(x).to(gpu)

    # the plain entry (dws_sampler_run; its graph is keyed on the caller's x, so it captures per call)
    plain = lambda labels, graph: sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise, use_graph=graph, labels=labels)
    assert torch.equal(plain(lr.LABELS, True), loop(lr.LABELS)) and torch.equal(plain(lr.LABELS, False), loop(lr.LABELS))
    # the schedule entry with the identity steps (bit-identical; its graph works on a model-owned state: replays)
    ident = np.arange(T, dtype=np.float32)
    noise_d = noise.to(gpu)      # (the injected noise's address is part of the graph's key: one device tensor for all runs)
    run = lambda labels, graph: sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise_d, use_graph=graph, labels=labels,
                                         net_steps=ident)
    first = run(lr.LABELS, True)
    n_graphs = _graphs(net)
    assert torch.equal(first, loop(lr.LABELS))
    assert torch.equal(first, run(lr.LABELS, False))
    assert torch.equal(first, run(lr.LABELS, True)) and _graphs(net) == n_graphs
    other = [0, 2, 3]
    second = run(other, True)
    assert _graphs(net) == n_graphs                      # the rows were rewritten in place: a replay
    assert torch.equal(second, run(other, False)) and torch.equal(second, loop(other))
    assert not torch.equal(second[0], first[0])          # clip 0 changed its class ...
    assert torch.equal(run(lr.LABELS, True), first) and _graphs(net) == n_graphs
    # the unlabelled run of the same model: the null class everywhere
    assert torch.equal(run(None, True), loop(None))
    # a labelled inpainting run: graph equals eager, the known samples come out bit-equal
    known = torch.randn(B, 1, L, generator=g) * 0.1
    mask = torch.zeros(1, 1, L, dtype=torch.bool)
    mask[..., L // 4: L // 2] = True
    kn = torch.randn(T, B, 1, L, generator=g)
    edit = lambda graph: sampling(net, (B, 1, L), dh, x_T=x_T, noise=noise, use_graph=graph, labels=lr.LABELS, known=known,
                                  mask=mask, known_noise=kn)
    e1, e0 = edit(True), edit(False)
    assert torch.equal(e1, e0)
    m = mask.expand(B, 1, L)
    assert torch.equal(e1.cpu()[m], known[m])
    assert not torch.equal(e1, first)


@pytest.mark.parametrize("kind", ["wn_tiny", "wn_c64", "sashimi"])
def test_labelled_sampler_with_a_single_clip(gpu, kind):
    """B = 1: a labelled table has one row per step, like an unlabelled one -- the label must still be in it (graph and
    eager, both entries), a new label must rewrite it in place, and dropping the labels must bring the null class back."""
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling
    net, L = _sampler_net(kind, gpu)
    T = 6
    dh = calc_diffusion_hyperparams(T, 1e-4, 0.05)
    g = torch.Generator().manual_seed(78)
    x_T, noise = torch.randn(1, 1, L, generator=g), torch.randn(T, 1, 1, L, generator=g)
    al, ab, sg = (dh[k] for k in ("Alpha", "Alpha_bar", "Sigma"))

    def loop(labels):       # the update in numpy float32 on the host, each operation rounded once
        x = x_T.numpy().copy()
        with torch.no_grad():
            for t in range(T - 1, -1, -1):
                eps = net((torch.from_numpy(x).to(gpu), torch.full((1, 1), float(t), device=gpu)), labels=labels).cpu().numpy()
                a_t, ab_t = np.float32(al[t]), np.float32(ab[t])
                x = (x - (np.float32(1) - a_t) / np.sqrt(np.float32(1) - ab_t) * eps) / np.sqrt(a_t)
                if t > 0:
                    x = x + np.float32(sg[t]) * noise[t].numpy()
        return torch.from_numpy(x).to(gpu)

    noise_d = noise.to(gpu)
    ident = np.arange(T, dtype=np.float32)
    run = lambda labels, graph, **kw: sampling(net, (1, 1, L), dh, x_T=x_T, noise=noise_d, use_graph=graph, labels=labels, **kw)
    null, two, zero = loop(None), loop([2]), loop([0])
    assert not torch.equal(two, null) and not torch.equal(two, zero)
    assert torch.equal(run([2], True), two) and torch.equal(run([2], False), two)          # dws_sampler_run
    assert torch.equal(run([2], True, net_steps=ident), two)                               # the schedule entry
    n_graphs = _graphs(net)
    assert torch.equal(run([0], True, net_steps=ident), zero) and _graphs(net) == n_graphs   # rewritten in place: a replay
    assert torch.equal(run([0], False, net_steps=ident), zero)
    assert torch.equal(run(None, True, net_steps=ident), null) and torch.equal(run(None, True), null)
    assert torch.equal(run([lr.K], True, net_steps=ident), null)
    assert torch.equal(run([2], True, net_steps=ident), two)

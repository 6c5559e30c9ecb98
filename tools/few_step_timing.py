"""Whole-call wall clock of the few-step samplers (dws_sampler_run_schedule) next to the full-T sampler and S x one
step, on one GPU: host clock around each call, every call ending in a device synchronise, after warm-up.

    python tools/few_step_timing.py [--repeats 5] [--out FILE]

Legs: config 4 (unet_d32_n6_T50_cond, B = 32, mel [1, 80, 63]) aligned S = 6 under f32 and bf16x6; config 2
(wnet_h256_d36_T200, B = 16) DDIM S = 50 under bf16x6 (the headline arithmetic).  Per leg: the first call (step-table
build + capture + instantiate + S replays), repeat calls with a new seed and a new output tensor (replays only),
the per-step time of the plain sampler's captured step (dws_sampler_steps) and the full-T dws_sampler_run call.
Capture + instantiate alone: `capture_cost`.  `--legs edit_c4,edit_c2` (not in the default list): the unedited schedule
call against the same call with a half-clip continuation mask (dws_sampler_run_edit), alternating in one process.
`--legs resample_c4` (not in the default list either): that edited call against the same call with resample=(2, 2)
(dws_sampler_run_program: 10 network evaluations and 2 jumps for S = 6), alternating in one process.
`--legs ragged_c2` (not in the default list): config 2 under bf16x6, the DDIM step without lengths, with
lengths = [L] * B and with a spread of lengths down to L / 2, alternating in one process (`ragged_leg`).
`--legs ragged_c4` (not in the default list): the same three variants on config 4 (SaShiMi, a mel per clip) under bf16x6,
then at L = 40000, where the top stage runs the segmented convolution (`ragged_sashimi_leg`)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(v):
    return dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), n=len(v))


def _step_ms(net, size, dh, repeats, n_steps=10):
    """Per-step time of the plain sampler's captured step (dws_sampler_steps, the graph replayed n_steps times)."""
    from diffwave_sashimi_amd import _lib
    from diffwave_sashimi_amd.sampling import _host_table, _prepare_run
    lib = _lib.load()
    T = dh["T"]
    with torch.no_grad():
        x, _, _, _ = _prepare_run(net, size, T, getattr(net, "_timing_mel", None), torch.randn(size), None, 1)
    a, pa = _host_table(dh["Alpha"])
    ab, pab = _host_table(dh["Alpha_bar"])
    sg, psg = _host_table(dh["Sigma"])
    run = lambda: _lib.check(lib.dws_sampler_steps(net._handle, x.data_ptr(), pa, pab, psg, T, T - 1, n_steps, 1, 1,
                                                   _lib.current_stream()))
    run()
    return [_clock(run) / n_steps for _ in range(repeats)]


def leg(name, cfg_name, precision, kind, S, repeats):
    from benchlib.configs import CONFIGS, build_model
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling, sampling_aligned, sampling_ddim
    cfg = CONFIGS[cfg_name]
    dev = torch.device("cuda")
    net = build_model(cfg, dev)
    if precision != "f32":
        net.set_option("precision", precision)
    B, L = cfg["B"], cfg["L"]
    size = (B, 1, L)
    mel = None
    if "Tmel" in cfg:
        g = torch.Generator().manual_seed(2)
        mel = (torch.rand(1, 80, cfg["Tmel"], generator=g) * 13.5 - 11.5).to(dev)
    net._timing_mel = mel
    d = cfg["diffusion"]
    dh_train = calc_diffusion_hyperparams(d["T"], d["beta_0"], d["beta_T"])
    if kind == "aligned":
        dcfg = dict(d, beta=[1e-4, 1e-3, 1e-2, 0.05, 0.2, 0.5])
        call = lambda seed: sampling_aligned(net, size, dcfg, mel, seed=seed)
    else:
        call = lambda seed: sampling_ddim(net, size, dh_train, S, 0.0, mel, seed=seed)
    # warm-up: code objects, the plain sampler's graph, allocator (another shape's first call)
    sampling(net, size, calc_diffusion_hyperparams(4, d["beta_0"], d["beta_T"]), mel, seed=0)
    first = _clock(lambda: call(100))
    repeat = [_clock(lambda i=i: call(101 + i)) for i in range(repeats)]
    graphs = int(net.read_tap("sampler_graphs", (1,)).item())
    step = _step_ms(net, size, dh_train, repeats)
    full =[_clock(lambda i=i: sampling(net, size, dh_train, mel, seed=500 + i)) for i in range(max(3, repeats // 2))]
    st = statistics.median(step)
    rec = dict(leg=name, config=cfg_name, precision=precision, sampler=kind, S=S, B=B, L=L,
               first_call=round(first, 3), repeat_call=_stats(repeat), graphs_after_repeats=graphs,
               step=_stats(step), S_x_step_ms=round(S * st, 3),
               repeat_over_S_x_step=round(statistics.median(repeat) / (S * st), 4),
               full_T=dict(T=d["T"], **_stats(full)))
    del net
    torch.cuda.empty_cache()
    return rec


def capture_cost(cfg_name, precision, kind, S, repeats):
    """Capture + instantiate of the schedule graph alone: alternate two schedules of the same S whose step tables
    differ, so that every call rebuilds the table AND recaptures; subtract the same alternation run eagerly
    (table rebuild, no graph) and normalise per call: (graph alternation - eager alternation) - (graph repeat -
    eager repeat) isolates capture + instantiate."""
    from benchlib.configs import CONFIGS, build_model
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling_ddim
    cfg = CONFIGS[cfg_name]
    dev = torch.device("cuda")
    net = build_model(cfg, dev)
    if precision != "f32":
        net.set_option("precision", precision)
    B, L = cfg["B"], cfg["L"]
    size = (B, 1, L)
    mel = None
    if "Tmel" in cfg:
        g = torch.Generator().manual_seed(2)
        mel = (torch.rand(1, 80, cfg["Tmel"], generator=g) * 13.5 - 11.5).to(dev)
    d = cfg["diffusion"]
    dh = calc_diffusion_hyperparams(d["T"], d["beta_0"], d["beta_T"])
    tau_a = list(range(S))
    tau_b = list(range(1, S + 1))
    run = lambda tau, g, seed: sampling_ddim(net, size, dh, tau, 0.0, mel, seed=seed, use_graph=g)
    for g in (True, False):
        run(tau_a, g, 1), run(tau_b, g, 1)
    alt = {True: [], False: []}
    rep = {True: [], False: []}
    for i in range(repeats):
        for g in (True, False):
            run(tau_a, g, 0)
            alt[g].append(_clock(lambda: run(tau_b, g, i)))      # other steps: table rebuild (+ capture)
            run(tau_a, g, 0)
            rep[g].append(_clock(lambda: run(tau_a, g, i)))      # same steps, new seed: replays only
    med = {k: statistics.median(v) for k, v in alt.items()}
    medr = {k: statistics.median(v) for k, v in rep.items()}
    per = [(alt[True][i] - alt[False][i]) - (rep[True][i] - rep[False][i]) for i in range(repeats)]
    rec = dict(config=cfg_name, precision=precision, S=S,
               graph_alternating=_stats(alt[True]), eager_alternating=_stats(alt[False]),
               graph_repeat=_stats(rep[True]), eager_repeat=_stats(rep[False]),
               capture_plus_instantiate_ms=_stats(per),
               capture_plus_instantiate_median_formula_ms=round((med[True] - med[False]) - (medr[True] - medr[False]), 3))
    del net
    torch.cuda.empty_cache()
    return rec


def edit_leg(name, cfg_name, precision, kind, S, repeats):
    """The editing step's cost: in one process and alternating, the unedited schedule call (the yardstick: the same
    code path as without the editing modes) and the same call with a half-clip continuation mask; every call a new
    seed.  The margin for the difference of the medians is the unedited leg's own min-max spread.  Also first call -
    repeat call of the edited graph (capture + instantiate; the step table exists by then)."""
    from benchlib.configs import CONFIGS, build_model
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling_aligned, sampling_ddim, spans_to_mask
    cfg = CONFIGS[cfg_name]
    dev = torch.device("cuda")
    net = build_model(cfg, dev)
    if precision != "f32":
        net.set_option("precision", precision)
    B, L = cfg["B"], cfg["L"]
    size = (B, 1, L)
    mel = None
    if "Tmel" in cfg:
        g = torch.Generator().manual_seed(2)
        mel = (torch.rand(1, 80, cfg["Tmel"], generator=g) * 13.5 - 11.5).to(dev)
    d = cfg["diffusion"]
    dh_train = calc_diffusion_hyperparams(d["T"], d["beta_0"], d["beta_T"])
    g = torch.Generator().manual_seed(3)
    edit = dict(known=(torch.rand(size, generator=g) * 2 - 1).to(dev), mask=spans_to_mask(size, [[0, L // 2]]).to(dev))
    if kind == "aligned":
        dcfg = dict(d, beta=[1e-4, 1e-3, 1e-2, 0.05, 0.2, 0.5])
        call = lambda seed, **kw: sampling_aligned(net, size, dcfg, mel, seed=seed, **kw)
    else:
        call = lambda seed, **kw: sampling_ddim(net, size, dh_train, S, 0.0, mel, seed=seed, **kw)
    call(1), call(2)                                        # warm-up: code objects, step table, the unedited graph
    first = _clock(lambda: call(100, **edit))
    call(101, **edit)
    plain, edited = [], []
    for i in range(repeats):
        plain.append(_clock(lambda: call(200 + i)))
        edited.append(_clock(lambda: call(300 + i, **edit)))
    graphs = int(net.read_tap("sampler_graphs", (1,)).item())
    mp, me = statistics.median(plain), statistics.median(edited)
    rec = dict(leg=name, config=cfg_name, precision=precision, sampler=kind, S=S, B=B, L=L, mask="first half kept",
               unedited_call=_stats(plain), edited_call=_stats(edited),
               edited_minus_unedited_median_ms=round(me - mp, 3),
               unedited_spread_ms=round(max(plain) - min(plain), 3),
               edited_first_call=round(first, 3), edited_first_minus_repeat_ms=round(first - me, 3),
               graphs_after_repeats=graphs)
    del net
    torch.cuda.empty_cache()
    return rec


def resample_leg(name, cfg_name, precision, S, repeats, jump=2, resamples=2):
    """The resampling call's cost per network evaluation beside the edited call's per step: in one process and
    alternating, the aligned call with a half-clip continuation mask (the yardstick) and the same call with
    resample=(jump, resamples); every call a new seed.  The margin for the difference per evaluation is the edited
    leg's own min-max spread per step.  Also first call - repeat call of the resampling graph (capture + instantiate;
    the step table and the other two graphs exist by then)."""
    from benchlib.configs import CONFIGS, build_model
    from diffwave_sashimi_amd.sampling import program_evaluations, repaint_program, sampling_aligned, spans_to_mask
    cfg = CONFIGS[cfg_name]
    dev = torch.device("cuda")
    net = build_model(cfg, dev)
    if precision != "f32":
        net.set_option("precision", precision)
    B, L = cfg["B"], cfg["L"]
    size = (B, 1, L)
    mel = None
    if "Tmel" in cfg:
        g = torch.Generator().manual_seed(2)
        mel = (torch.rand(1, 80, cfg["Tmel"], generator=g) * 13.5 - 11.5).to(dev)
    g = torch.Generator().manual_seed(3)
    edit = dict(known=(torch.rand(size, generator=g) * 2 - 1).to(dev), mask=spans_to_mask(size, [[0, L // 2]]).to(dev))
    dcfg = dict(cfg["diffusion"], beta=[1e-4, 1e-3, 1e-2, 0.05, 0.2, 0.5][:S])
    call = lambda seed, **kw: sampling_aligned(net, size, dcfg, mel, seed=seed, **edit, **kw)
    evals = program_evaluations(S, jump, resamples)
    V = len(repaint_program(S, jump, resamples))
    sampling_aligned(net, size, dcfg, mel, seed=1)          # warm-up: code objects, step table, the unedited graph
    call(2), call(3)                                        # ... and the edited graph
    first = _clock(lambda: call(100, resample=(jump, resamples)))
    call(101, resample=(jump, resamples))
    edited, resampled = [], []
    for i in range(repeats):
        edited.append(_clock(lambda: call(200 + i)))
        resampled.append(_clock(lambda: call(300 + i, resample=(jump, resamples))))
    graphs = int(net.read_tap("sampler_graphs", (1,)).item())
    me, mr = statistics.median(edited), statistics.median(resampled)
    rec = dict(leg=name, config=cfg_name, precision=precision, sampler="aligned", S=S, B=B, L=L, mask="first half kept",
               resample=[jump, resamples], visits=V, evaluations=evals, jumps=V - evals,
               edited_call=_stats(edited), resampled_call=_stats(resampled),
               edited_per_step_ms=round(me / S, 3), resampled_per_evaluation_ms=round(mr / evals, 3),
               per_evaluation_minus_per_step_ms=round(mr / evals - me / S, 3),
               edited_per_step_spread_ms=round((max(edited) - min(edited)) / S, 3),
               resampled_first_call=round(first, 3), resampled_first_minus_repeat_ms=round(first - mr, 3),
               graphs_after_repeats=graphs)
    del net
    torch.cuda.empty_cache()
    return rec


def ragged_leg(name, cfg_name, precision, S, repeats):
    """The cost of per-clip lengths (dws_model_set_lengths) per step: in one process and alternating, the DDIM call
    without lengths (the yardstick: it launches exactly the kernels it launched before the feature), with
    lengths = [L] * B (every sealing launch is in the step and finds an empty range) and with a spread of lengths from L
    down to L / 2 (a quarter of the batch is padding); every call a new seed.  Per step = call / S.  The sealing kernel
    rewrites only the next layer's dilation behind a clip's end; DWS_RAGGED_FULL_TAIL=1 in the environment of the process
    makes it rewrite the whole tail instead (the A/B of the two forms: run the leg once with and once without)."""
    from benchlib.configs import CONFIGS, build_model
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling_ddim
    cfg = CONFIGS[cfg_name]
    dev = torch.device("cuda")
    net = build_model(cfg, dev)
    if precision != "f32":
        net.set_option("precision", precision)
    B, L = cfg["B"], cfg["L"]
    size = (B, 1, L)
    d = cfg["diffusion"]
    dh = calc_diffusion_hyperparams(d["T"], d["beta_0"], d["beta_T"])
    spread = [L - (L // 2) * b // max(B - 1, 1) for b in range(B)]
    variants = {"plain": None, "full_lengths": [L] * B, "spread_lengths": spread}
    call = lambda seed, lens: sampling_ddim(net, size, dh, S, 0.0, None, seed=seed, lengths=lens)
    for lens in variants.values():                          # warm-up: code objects, step table, both graphs
        call(1, lens), call(2, lens)
    times = {k: [] for k in variants}
    for i in range(repeats):
        for k, lens in variants.items():
            times[k].append(_clock(lambda: call(100 + i, lens)) / S)
    med = {k: statistics.median(v) for k, v in times.items()}
    rec = dict(leg=name, config=cfg_name, precision=precision, S=S, B=B, L=L,
               reach="full tail" if os.environ.get("DWS_RAGGED_FULL_TAIL") else "next dilation",
               padded_share_spread=round(1.0 - sum(spread) / float(B * L), 4),
               per_step={k: _stats(v) for k, v in times.items()},
               full_minus_plain_ms=round(med["full_lengths"] - med["plain"], 4),
               spread_minus_plain_ms=round(med["spread_lengths"] - med["plain"], 4),
               spread_over_plain=round(med["spread_lengths"] / med["plain"], 5),
               plain_spread_ms=round(max(times["plain"]) - min(times["plain"]), 4),
               graphs_after_repeats=int(net.read_tap("sampler_graphs", (1,)).item()))
    del net
    torch.cuda.empty_cache()
    return rec


def ragged_sashimi_leg(name, cfg_name, precision, S, repeats, L_long=40000):
    """The cost of per-clip lengths on SaShiMi per step: in one process and alternating, the DDIM call without lengths (the
    yardstick: the kernels it launched before the feature, the length-aware instances are not dispatched), with
    lengths = [L] * B (the length-aware convolutions, every row whole) and with a spread of lengths from L down to L / 2 in
    multiples of 256; every call a new seed, a mel per clip.  Then the plain and the spread call at L = L_long, where the top
    stage runs the segmented convolution, whose workgroups of wholly padded output segments return at once --
    DWS_RAGGED_SEG_NO_SKIP=1 in the environment of the process makes them run (the A/B of the two forms: run the leg once
    with and once without)."""
    from benchlib.configs import CONFIGS, build_model
    from diffwave_sashimi_amd.sampling import calc_diffusion_hyperparams, sampling_ddim
    cfg = CONFIGS[cfg_name]
    dev = torch.device("cuda")
    net = build_model(cfg, dev)
    if precision != "f32":
        net.set_option("precision", precision)
    B = cfg["B"]
    d = cfg["diffusion"]
    dh = calc_diffusion_hyperparams(d["T"], d["beta_0"], d["beta_T"])
    rec = dict(leg=name, config=cfg_name, precision=precision, S=S, B=B,
               padded_segments="run" if os.environ.get("DWS_RAGGED_SEG_NO_SKIP") else "return at once", runs=[])
    for L in (cfg["L"], L_long):
        size = (B, 1, L)
        g = torch.Generator().manual_seed(2)
        mel = (torch.rand(B, 80, (L + 255) // 256, generator=g) * 13.5 - 11.5).to(dev)
        spread = [L if b == 0 else max(L // 2, (L - (L // 2) * b // max(B - 1, 1)) // 256 * 256) for b in range(B)]
        variants = {"plain": None, "full_lengths": [L] * B, "spread_lengths": spread}
        if L == L_long:
            del variants["full_lengths"]
        call = lambda seed, lens: sampling_ddim(net, size, dh, S, 0.0, mel, seed=seed, lengths=lens)
        for lens in variants.values():                      # warm-up: code objects, kernels of this length, step table, graphs
            call(1, lens), call(2, lens)
        times = {k: [] for k in variants}
        for i in range(repeats):
            for k, lens in variants.items():
                times[k].append(_clock(lambda: call(100 + i, lens)) / S)
        med = {k: statistics.median(v) for k, v in times.items()}
        run = dict(L=L, padded_share_spread=round(1.0 - sum(spread) / float(B * L), 4),
                   per_step={k: _stats(v) for k, v in times.items()},
                   spread_minus_plain_ms=round(med["spread_lengths"] - med["plain"], 4),
                   spread_over_plain=round(med["spread_lengths"] / med["plain"], 5),
                   plain_spread_ms=round(max(times["plain"]) - min(times["plain"]), 4),
                   graphs_after_repeats=int(net.read_tap("sampler_graphs", (1,)).item()))
        if "full_lengths" in med:
            run["full_minus_plain_ms"] = round(med["full_lengths"] - med["plain"], 4)
        rec["runs"].append(run)
    del net
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default="c4_f32,c4_bx6,c2_ddim50,capture")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    legs = {
        "c4_f32": lambda: leg("config4 aligned S=6 f32", "unet_d32_n6_T50_cond", "f32", "aligned", 6, args.repeats),
        "c4_bx6": lambda: leg("config4 aligned S=6 bf16x6", "unet_d32_n6_T50_cond", "bf16x6", "aligned", 6, args.repeats),
        "c2_ddim50": lambda: leg("config2 DDIM S=50 bf16x6", "wnet_h256_d36_T200", "bf16x6", "ddim", 50, args.repeats),
        "edit_c4": lambda: edit_leg("config4 aligned S=6 f32, continuation", "unet_d32_n6_T50_cond", "f32", "aligned", 6,
                                    args.repeats),
        "edit_c2": lambda: edit_leg("config2 DDIM S=50 bf16x6, continuation", "wnet_h256_d36_T200", "bf16x6", "ddim", 50,
                                    args.repeats),
        "resample_c4": lambda: resample_leg("config4 aligned S=6 f32, continuation, resample=(2,2)",
                                            "unet_d32_n6_T50_cond", "f32", 6, args.repeats),
        "ragged_c2": lambda: ragged_leg("config2 DDIM S=10 bf16x6, per-clip lengths", "wnet_h256_d36_T200", "bf16x6", 10,
                                        args.repeats),
        "ragged_c4": lambda: ragged_sashimi_leg("config4 DDIM S=6 bf16x6, per-clip lengths", "unet_d32_n6_T50_cond", "bf16x6", 6,
                                                args.repeats),
        "capture": lambda: [capture_cost("unet_d32_n6_T50_cond", "f32", "ddim", 6, args.repeats),
                            capture_cost("wnet_h256_d36_T200", "bf16x6", "ddim", 50, args.repeats)],
    }
    out = []
    for k in args.legs.split(","):
        r = legs[k]()
        for x in (r if isinstance(r, list) else [r]):
            print(json.dumps(x), flush=True)
            out.append(x)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""CPU: the host side of per-clip seeds -- ``sampling.clip_seeds`` (splitmix64 of the run's seed and the global clip
number), the validation of a seed list, ``generate.clip_plan`` (which global clips go in which batch on which rank) and
the two exports in the binding."""
import numpy as np
import pytest
import torch

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def _splitmix64(z):
    """Independent restatement (Vigna's splitmix64.c, one output of the generator whose state is z)."""
    z = (z + 0x9E3779B97F4A7C15) % (1 << 64)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % (1 << 64)
    return z ^ (z >> 31)


def test_splitmix64_restatement_against_the_published_vector():
    """State 0: the first output of splitmix64.c is 0xE220A8397B1DCDAF (the value every xoshiro seeding test pins)."""
    assert _splitmix64(0) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("seed", [0, 5, M64])
@pytest.mark.parametrize("first", [0, 37])
def test_clip_seeds_are_splitmix64_of_seed_and_global_clip(seed, first):
    from diffwave_sashimi_amd.sampling import clip_seeds
    got = clip_seeds(seed, first, 9)
    assert got == [_splitmix64((seed + GOLDEN * (first + j + 1)) % (1 << 64)) for j in range(9)]
    assert all(isinstance(v, int) and 0 <= v <= M64 for v in got)
    # a clip's seed depends on its global number alone, not on where the batch starts
    assert clip_seeds(seed, first + 4, 3) == got[4:7]
    assert clip_seeds(seed, first, 0) == []


def test_clip_seeds_are_distinct_and_neighbouring_runs_do_not_share_streams():
    from diffwave_sashimi_amd.sampling import clip_seeds
    many = clip_seeds(5, 0, 10000)
    assert len(set(many)) == 10000
    assert clip_seeds(5, 1, 1) != clip_seeds(6, 0, 1)          # seed + 1000 r + i would collide like this
    assert not set(clip_seeds(5, 0, 2000)) & set(clip_seeds(6, 0, 2000))
    with pytest.raises(ValueError):
        clip_seeds(5, -1, 2)
    with pytest.raises(ValueError):
        clip_seeds("5", 0, 2)


def test_seed_list_validation_is_host_side():
    from diffwave_sashimi_amd.sampling import seed_list
    assert seed_list(None, 3) is None and seed_list(7, 3) is None and seed_list(np.int64(7), 3) is None
    assert seed_list([11, 11, 2 ** 63 + 5], 3) == [11, 11, 2 ** 63 + 5]
    assert seed_list((0, M64), 2) == [0, M64]
    assert seed_list(torch.tensor([3, 4]), 2) == [3, 4]
    assert seed_list(np.array([3, 2 ** 64 - 1], dtype=np.uint64), 2) == [3, 2 ** 64 - 1]
    for bad, B in (([1, 2], 3), ([1, 2, 3, 4], 3), ([], 1)):                     # wrong length
        with pytest.raises(ValueError, match="clip seeds for a batch"):
            seed_list(bad, B)
    with pytest.raises(ValueError, match="0 .. 2\\^64-1"):
        seed_list([1, -1], 2)
    with pytest.raises(ValueError, match="0 .. 2\\^64-1"):
        seed_list([1, 2 ** 64], 2)
    with pytest.raises(ValueError):
        seed_list([1, 2.0], 2)
    with pytest.raises(ValueError):
        seed_list([1, True], 2)
    with pytest.raises(ValueError):
        seed_list(torch.tensor([[1, 2]]), 2)
    with pytest.raises(ValueError):
        seed_list(torch.tensor([1.0, 2.0]), 2)


def test_samplers_refuse_a_bad_seed_list_before_any_gpu_work():
    """``net`` is never looked at: the check comes first."""
    from diffwave_sashimi_amd import sampling as smp
    dh = smp.calc_diffusion_hyperparams(6, 1e-4, 0.05)
    for call in (lambda s: smp.sampling(None, (3, 1, 64), dh, seed=s),
                 lambda s: smp.sampling_ddim(None, (3, 1, 64), dh, 3, seed=s),
                 lambda s: smp.sampling_dpmpp(None, (3, 1, 64), dh, 3, seed=s),
                 lambda s: smp.sampling_aligned(None, (3, 1, 64), dict(T=6, beta_0=1e-4, beta_T=0.05, beta=[1e-4, 0.05]), seed=s)):
        with pytest.raises(ValueError, match="clip seeds for a batch"):
            call([1, 2])
        with pytest.raises(ValueError, match="0 .. 2\\^64-1"):
            call([1, 2, -3])
        with pytest.raises(ValueError, match="0 .. 2\\^64-1"):
            call([1, 2, 2 ** 64])


def test_guided_fallback_draws_one_generator_per_clip():
    """Another ``net`` (the torch CPU generator path): clip b of a seed-list run is the B = 1 run with seed[b]."""
    from diffwave_sashimi_amd import sampling as smp
    dh = smp.calc_diffusion_hyperparams(4, 1e-4, 0.05)
    net = lambda inp, **kw: 0.1 * inp[0]
    L = 37                                                     # C L % 4 != 0
    y = torch.zeros(1, 1, L)
    op = smp.declip_operator(0.5)
    run = lambda B, seed: smp.sampling_guided(net, (B, 1, L), dh, measurement=y.expand(B, 1, L), operator=op, scale=0.3,
                                              seed=seed)
    seeds = [11, 11, 2 ** 63 + 5]
    out = run(3, seeds)
    for b, k in enumerate(seeds):
        assert torch.equal(out[b:b + 1], run(1, k))
    assert torch.equal(out[0], out[1]) and not torch.equal(out[0], out[2])
    assert torch.equal(run(3, seeds[::-1]), out.flip(0))
    with pytest.raises(ValueError, match="clip seeds for a batch"):
        run(2, seeds)


def test_clip_plan_over_ranks_and_batches():
    from diffwave_sashimi_amd.generate import clip_plan
    kw = dict(clip_seeds=True, seed=5)
    assert clip_plan(8, 4, 0, 1, **kw) == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert clip_plan(8, 4, 0, 2, **kw) == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert clip_plan(8, 4, 1, 2, **kw) == [[8, 9, 10, 11], [12, 13, 14, 15]]
    assert clip_plan(8, 8, 1, 2, **kw) == [[8, 9, 10, 11, 12, 13, 14, 15]]
    assert clip_plan(8, 1, 0, 1, **kw) == [[k] for k in range(8)]
    # named clips: rank r of N takes clips[r::N], batches of up to batch_size
    assert clip_plan(8, 4, 0, 1, clips=[2, 9, 5], **kw) == [[2, 9, 5]]
    assert clip_plan(8, 2, 0, 1, clips=[2, 9, 5], **kw) == [[2, 9], [5]]
    assert clip_plan(8, 4, 0, 2, clips=[2, 9, 5], **kw) == [[2, 5]]
    assert clip_plan(8, 4, 1, 2, clips=[2, 9, 5], **kw) == [[9]]
    assert clip_plan(1, 4, 3, 4, clips=[2, 9, 5], **kw) == []                    # a rank with nothing to do
    # off: nothing is planned, the loop of the reference runs
    assert clip_plan(8, 4, 1, 2) is None and clip_plan(8, 4, 1, 2, clip_seeds=False, seed=5) is None


def test_clip_plan_refusals():
    from diffwave_sashimi_amd.generate import clip_plan
    with pytest.raises(ValueError, match="generate.clips needs generate.clip_seeds"):
        clip_plan(8, 4, clips=[2], seed=5)
    with pytest.raises(ValueError, match="generate.clip_seeds needs generate.seed"):
        clip_plan(8, 4, clip_seeds=True)
    with pytest.raises(ValueError, match="generate.clip_seeds needs generate.seed"):
        clip_plan(8, 4, clip_seeds=True, clips=[2])
    with pytest.raises(ValueError, match="does not divide"):
        clip_plan(8, 3, clip_seeds=True, seed=5)
    for bad in ([], [1, 1], [-1], [1.5], "2"):
        with pytest.raises(ValueError, match="generate.clips"):
            clip_plan(8, 4, clip_seeds=True, seed=5, clips=bad)
    with pytest.raises(ValueError, match="generate.clip_seeds="):
        clip_plan(8, 4, clip_seeds="yes", seed=5)


def test_generate_refuses_the_key_combinations_before_building_a_model():
    from diffwave_sashimi_amd.generate import generate
    from tests import cases
    cfg = cases.WAVENET_CASES["wn_tiny"][0]
    diff = dict(T=6, beta_0=1e-4, beta_T=0.05, beta=None)
    ds = dict(_name_="sc09", segment_length=300, sampling_rate=16000)
    with pytest.raises(ValueError, match="generate.clips needs generate.clip_seeds"):
        generate(0, diff, dict(cfg), ds, ckpt_iter="init", n_samples=4, seed=5, clips=[2])
    with pytest.raises(ValueError, match="generate.clip_seeds needs generate.seed"):
        generate(0, diff, dict(cfg), ds, ckpt_iter="init", n_samples=4, clip_seeds=True)


def test_the_binding_declares_the_two_exports():
    from diffwave_sashimi_amd import _lib
    assert "dws_sampler_set_clip_seeds" in _lib.EXPORTS and "dws_philox_normal_clips" in _lib.EXPORTS

"""The yardstick of tests/test_infer_incep_bf16_gpu.py: with every rounding switched off, the bf16-emulating forward of
make_upscaler_incep_resnet is oracle.generators.upscaler_incep_resnet; with the roundings on, every tensor it stores is the bf16 rounding
of the fp64 function of one launch (layer_plan) applied to the tensors it stored before -- the rounding points sit where the module's
docstring says, and layer_plan is the teacher-forced reference the GPU tests hold the device to."""
import numpy as np
import pytest
import torch

from _incep_bf16_emulation import IncepBf16Net, incep_forward_emulated, layer_plan


def randomised(in_shape, seed, **kw):
    """initial weights with non-trivial statistics, slopes and biases (as tests/test_generators_gpu.py's _randomise)"""
    from oracle import generators as OG, models as M
    w = OG.init_weights(OG.upscaler_incep_resnet, in_shape, seed, **kw)
    rng = np.random.RandomState(seed + 1)
    for name, v in w.items():
        if name.endswith("/gamma"):
            w[name] = rng.uniform(0.7, 1.3, v.shape).astype(np.float32)
        elif name.endswith(("/beta", "/moving_mean", "/bias")):
            w[name] = rng.uniform(-0.2, 0.2, v.shape).astype(np.float32)
        elif name.endswith("/moving_variance"):
            w[name] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif name.endswith("/alpha"):
            w[name] = rng.uniform(0.05, 0.4, v.shape).astype(np.float32)
    return w, M.to_torch(w, torch.float64)


def _frames(n, h, w, seed=0):
    return torch.tensor(np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)) / 127.5 - 1, dtype=torch.float64)


CONFIGS = [dict(a_block_type="3path", a_block_num=1, a_block_kernel=3, b_block_type="2path", b_block_num=1, b_block_kernel=7,
                c_block_type="2path", c_block_num=1, c_block_kernel=3, upscale_factor=2),
           dict(a_block_type="2path", a_block_num=1, a_block_kernel=5, b_block_type="3path", b_block_num=1, b_block_kernel=5,
                c_block_type="2path", c_block_num=0, c_block_kernel=5, upscale_factor=4)]


@pytest.mark.parametrize("kw", CONFIGS)
def test_emulation_without_roundings_is_the_oracle(kw):
    from oracle import generators as OG
    h, w = 10, 14
    _, wd = randomised((h, w, 3), 3, **kw)
    x = _frames(2, h, w)
    f = kw["upscale_factor"]
    with torch.no_grad():
        ref = OG.upscaler_incep_resnet(OG.Net(wd, False), x, **kw)
        got = incep_forward_emulated(wd, x, bf16=False, **kw)
        rounded = incep_forward_emulated(wd, x, bf16=True, **kw)
    assert got.shape == ref.shape == (2, f * h, f * w, 3)
    assert torch.equal(got, ref)
    d = float((rounded - ref).abs().max())          # with the roundings on: a different function, by about what bf16 storage does
    assert 1e-6 < d < 0.2, d


@pytest.mark.parametrize("kw", [dict(a_block_type="3path", a_block_num=1, a_block_kernel=3, b_block_num=0, c_block_num=0, c_block_kernel=3,
                                     upscale_factor=2),
                                dict(a_block_num=0, b_block_type="2path", b_block_num=1, b_block_kernel=7, c_block_num=0, c_block_kernel=5,
                                     upscale_factor=4)])
def test_every_stored_tensor_is_one_launch_of_the_previous_ones(kw):
    h, w = 9, 12
    _, wd = randomised((h, w, 3), 5, **kw)
    x = _frames(1, h, w, 1)
    taps = {}
    with torch.no_grad():
        y = incep_forward_emulated(wd, x, bf16=True, taps=taps, **kw)
        plan = layer_plan(wd, x, **kw)
        # every stored tensor is named (the plan lists them in the engine's launch order: a block's head first; the oracle walks path by path)
        assert sorted(name for name, _ in plan) == sorted(taps) and len(plan) == len(taps)
        for name, fn in plan:
            ref = fn(taps)
            want = ref if name == "final/conv" else ref.to(torch.bfloat16).to(torch.float64)          # final/conv stays unrounded
            assert taps[name].shape == ref.shape, name
            assert float((taps[name] - want).abs().max()) <= 1e-12, name
            if name != "final/conv":          # a stored tensor holds bf16 values
                assert torch.equal(taps[name].to(torch.bfloat16).to(torch.float64), taps[name]), name
    assert torch.equal(taps["final/conv"].permute(0, 2, 3, 1), y)
    n3 = "inc_res_block/A/3p/0"
    if kw["a_block_num"]:
        assert taps[n3 + "/c/3/prelu"].shape[1] == 48 and taps[n3 + "/b/2/prelu"].shape[1] == 32
    else:
        assert taps["inc_res_block/B/2p/0/b/2/prelu"].shape[1] == 19 and taps["inc_res_block/B/2p/0/b/3/prelu"].shape[1] == 25


def test_net_subclass_refuses_duplicate_names_like_the_oracle():
    net = IncepBf16Net({}, True)
    net._name("initial/conv/9x9", "conv2d")
    with pytest.raises(ValueError):
        net._name("initial/conv/9x9", "conv2d")

"""The yardstick of tests/test_infer_cyclegan_bf16_gpu.py: with every rounding switched off, the bf16-emulating forward of
make_generator_cyclegan is oracle.generators.generator_cyclegan."""
import numpy as np
import pytest
import torch

from _cyclegan_bf16_emulation import cyclegan_forward_emulated


def _weights(in_shape, seed, **kw):
    from oracle import generators as OG, models as M
    w = OG.init_weights(OG.generator_cyclegan, in_shape, seed, **kw)
    rng = np.random.RandomState(seed + 1)
    for name, v in w.items():          # non-trivial statistics, slopes and biases
        if name.endswith("/gamma"):
            w[name] = rng.uniform(0.7, 1.3, v.shape).astype(np.float32)
        elif name.endswith(("/beta", "/moving_mean", "/bias")):
            w[name] = rng.uniform(-0.2, 0.2, v.shape).astype(np.float32)
        elif name.endswith("/moving_variance"):
            w[name] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif name.endswith("/alpha"):
            w[name] = rng.uniform(0.0, 0.3, v.shape).astype(np.float32)
    return M.to_torch(w, torch.float64)


@pytest.mark.parametrize("f", [1, 2, 4])
@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_emulation_without_roundings_is_the_oracle(norm, f):
    from oracle import generators as OG
    h, w, nd, res = 16, 24, 2, 1
    kw = dict(filters=64, n_downsample=nd, res_block_num=res, upscale_factor=f, norm=norm, kernel_size=3)
    wd = _weights((h, w, 3), 3, **kw)
    x = torch.tensor(np.random.RandomState(0).randint(0, 256, (1, h, w, 3)) / 127.5 - 1, dtype=torch.float64)
    with torch.no_grad():
        ref = OG.generator_cyclegan(OG.Net(wd, False), x, **kw)
        taps = {}
        got = cyclegan_forward_emulated(wd, x, nd, res, f, norm, bf16=False, taps=taps)
        rounded = cyclegan_forward_emulated(wd, x, nd, res, f, norm, bf16=True)
    assert got.shape == ref.shape == (1, f * h, f * w, 3)
    assert float((got - ref).abs().max()) <= 1e-12
    # every stored tensor is named, in the order of the pass
    names = ["stem/conv", "stem/prelu", "down/0/conv", "down/0/prelu", "down/1/conv", "down/1/prelu", "res_block/0/conv_pre",
             "res_block/0/prelu", "res_block/0/conv_post", "res_block/0/final_add"]
    for i in range(nd + {1: 0, 2: 1, 4: 2}[f]):
        names += ["up/%d/conv_transp" % i, "up/%d/prelu" % i]
    assert list(taps) == names + ["head/conv"]
    assert torch.equal(taps["head/conv"].permute(0, 2, 3, 1), got)
    # ... and with the roundings on it is a different function, by about what bf16 storage does
    d = float((rounded - ref).abs().max())
    assert 1e-6 < d < 0.2, d


def test_emulation_kernel_size_5_one_downsampling():
    from oracle import generators as OG
    h, w = 8, 12
    kw = dict(filters=64, n_downsample=1, res_block_num=2, upscale_factor=2, norm="instance", kernel_size=5)
    wd = _weights((h, w, 3), 5, **kw)
    x = torch.tensor(np.random.RandomState(1).randint(0, 256, (2, h, w, 3)) / 127.5 - 1, dtype=torch.float64)
    with torch.no_grad():
        ref = OG.generator_cyclegan(OG.Net(wd, False), x, **kw)
        got = cyclegan_forward_emulated(wd, x, 1, 2, 2, "instance", bf16=False)
    assert float((got - ref).abs().max()) <= 1e-12

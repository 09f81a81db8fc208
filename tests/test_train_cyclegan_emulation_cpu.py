"""The yardstick of the model test in tests/test_train_cyclegan_bf16_gpu.py, checked without a device: with every rounding switched off the
storage-emulating training forward of make_generator_cyclegan is oracle.generators.generator_cyclegan in training mode, and at the
seeds the model test uses the only gradients the emulation itself leaves below the zero floor are biases in front of a norm."""
import numpy as np
import pytest
import torch

from _cyclegan_bf16_train_emulation import CASES, FLOOR, N, H, W, RES, allowed_zero_gradients, cyclegan_train_forward_emulated, l2, randomized_weights, \
    training_case


@pytest.mark.parametrize("norm,f,down", CASES)
def test_training_emulation_without_roundings_is_the_oracle(norm, f, down):
    from oracle import generators as OG, models as M
    wd = M.to_torch(randomized_weights(norm, f, down), torch.float64)
    x = torch.tensor(np.random.RandomState(0).randint(0, 256, (N, H, W, 3)) / 127.5 - 1, dtype=torch.float64)
    with torch.no_grad():
        net = OG.Net(wd, True)
        ref = OG.generator_cyclegan(net, x, filters=64, n_downsample=down, res_block_num=RES, upscale_factor=f, norm=norm, kernel_size=3)
        got, upd = cyclegan_train_forward_emulated(wd, x, down, RES, f, norm, bf16=False)
        rounded, _ = cyclegan_train_forward_emulated(wd, x, down, RES, f, norm, bf16=True)
    assert got.shape == ref.shape == (N, f * H, f * W, 3)
    assert float((got - ref).abs().max()) <= 1e-12
    assert list(upd) == list(net.upd) and (norm == "batch") == bool(upd)
    for k, v in net.upd.items():
        assert float((upd[k] - v).abs().max()) <= 1e-12, k
    d = float((rounded - ref).abs().max())          # with the roundings on it is a different function, by about what bf16 storage does
    assert 1e-6 < d < 0.2, d


@pytest.mark.parametrize("norm,f,down", CASES)
def test_only_biases_in_front_of_a_norm_fall_below_the_zero_floor(norm, f, down):
    """the model test excludes numerically-zero gradients from its relative comparison; here: which ones those are at its seeds, and that
    the emulation's own fp32-vs-fp64 distance -- the scale of its bound -- is finite for every other tensor"""
    c = training_case(norm, f, down)
    g64, g32 = c["f64"]["grads"], c["f32"]["grads"]
    gmax = max(float(g.abs().max()) for g in g64.values())
    below = {k for k, b in g64.items() if float(b.norm()) < FLOOR * gmax * b.numel() ** 0.5}
    assert below <= allowed_zero_gradients(f, down), sorted(below - allowed_zero_gradients(f, down))
    for k, b in g64.items():
        if k not in below:
            assert np.isfinite(l2(g32[k], b, FLOOR * gmax * b.numel() ** 0.5)), k
    assert np.isfinite(c["f64"]["loss"]) and c["f64"]["loss"] > 1e-3

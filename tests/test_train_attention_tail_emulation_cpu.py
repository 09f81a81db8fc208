"""The yardstick of the model tests in tests/test_train_attention_tail_bf16_gpu.py, checked without a device: with every rounding switched
off the storage-emulating training forward of make_upscaler_attention with the bf16 tail is
oracle.models.upscaler_attention_forward(training=True) -- output, moving statistics and gradients --, and at the seeds the model test uses
the only gradients below the zero floor, in the emulation's fp64 and fp32 pass alike, are biases of convolutions that a BatchNormalization
follows."""
import numpy as np
import pytest
import torch

from _attention_bf16_tail_train_emulation import CASES, FLOOR, N, H, W, RES, SEEDS, allowed_zero_gradients, attention_tail_train_forward_emulated, \
    below_floor, l2, randomized_weights, training_case


@pytest.mark.parametrize("k,f", CASES)
def test_tail_emulation_without_roundings_is_the_oracle(k, f):
    from oracle import models as M
    x = torch.tensor(np.random.RandomState(0).randint(0, 256, (N, H, W, 3)) / 127.5 - 1, dtype=torch.float64)
    t = torch.tensor(np.random.RandomState(3).randint(0, 256, (N, f * H, f * W, 3)) / 127.5 - 1, dtype=torch.float64)
    res = []
    for fn in (lambda w: M.upscaler_attention_forward(w, x, True, RES, f),
               lambda w: attention_tail_train_forward_emulated(w, x, RES, f, True, bf16=False)):
        wd = M.to_torch(randomized_weights(k, f, SEEDS[(k, f)]), torch.float64, requires_grad=True)
        y, upd = fn(wd)
        names = [kk for kk, v in wd.items() if v.requires_grad]
        grads = torch.autograd.grad(((y - t) ** 2).mean(), [wd[kk] for kk in names])
        res.append((y.detach(), upd, dict(zip(names, grads))))
    (ref, rupd, rg), (got, upd, gg) = res
    assert got.shape == ref.shape == (N, f * H, f * W, 3)
    assert float((got - ref).abs().max()) <= 1e-12
    assert list(upd) == list(rupd) and len(upd) == 2 * (2 * RES + 1)
    for kk, v in rupd.items():
        assert float((upd[kk] - v).abs().max()) <= 1e-12, kk
    assert list(gg) == list(rg)
    for kk, v in rg.items():
        assert float((gg[kk] - v).abs().max()) <= 1e-12, kk
    with torch.no_grad():
        wd = M.to_torch(randomized_weights(k, f, SEEDS[(k, f)]), torch.float64)
        rounded, _ = attention_tail_train_forward_emulated(wd, x, RES, f, True, bf16=True)
        ref0, _ = M.upscaler_attention_forward(wd, x, False, RES, f)
        got0, upd0 = attention_tail_train_forward_emulated(wd, x, RES, f, False, bf16=False)
    d = float((rounded - ref).abs().max())          # with the roundings on it is a different function, by about what bf16 storage does
    assert 1e-6 < d < 0.2, d
    assert float((got0 - ref0).abs().max()) <= 1e-12 and not upd0          # learning phase 0: the moving statistics, nothing updated


@pytest.mark.parametrize("k,f", CASES)
def test_tail_only_biases_in_front_of_a_norm_fall_below_the_zero_floor(k, f):
    """a condition on the model test's inputs, not a tolerance: at SEEDS the gradients the model test excludes from its relative comparison
    are allowed_zero_gradients() and nothing else, in the fp64 and in the fp32 pass; every other tensor's fp32-vs-fp64 distance -- the
    scale of its bound -- is finite"""
    c = training_case(k, f)
    for tag in ("f64", "f32"):
        below = set(below_floor(c[tag]))
        assert below <= allowed_zero_gradients(), (tag, sorted(below - allowed_zero_gradients()))
    g64, g32 = c["f64"]["grads"], c["f32"]["grads"]
    gmax = max(float(v.abs().max()) for v in g64.values())
    for kk, b in g64.items():
        assert np.isfinite(l2(g32[kk], b, FLOOR * gmax * b.numel() ** 0.5)), kk
    assert np.isfinite(c["f64"]["loss"]) and c["f64"]["loss"] > 1e-3

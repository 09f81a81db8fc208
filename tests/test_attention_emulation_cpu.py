"""The yardstick of tests/test_infer_attention_bf16_gpu.py: with every rounding switched off, the bf16-emulating forward of the attention
generator is oracle.models.upscaler_attention_forward."""
import numpy as np
import pytest
import torch

from _attention_bf16_emulation import attention_forward_emulated


def _weights(shape, k, f, res, seed):
    from oracle import models as M
    w = M.init_upscaler_attention(shape, kernel_size=k, upscale_factor=f, res_block_num=res, seed=seed)
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


@pytest.mark.parametrize("k,f", [(3, 2), (5, 4)])
def test_emulation_without_roundings_is_the_oracle(k, f):
    from oracle import models as M
    res, h, w = 2, 5, 6
    wd = _weights((f * h, f * w, 3), k, f, res, 3)
    x = torch.tensor(np.random.RandomState(0).randint(0, 256, (2, h, w, 3)) / 127.5 - 1, dtype=torch.float64)
    with torch.no_grad():
        ref, _ = M.upscaler_attention_forward(wd, x, False, res, f)
        got = attention_forward_emulated(wd, x, res, f, bf16=False)
        rounded = attention_forward_emulated(wd, x, res, f, bf16=True)
    assert got.shape == ref.shape == (2, f * h, f * w, 3)
    assert float((got - ref).abs().max()) <= 1e-12
    # ... and with them on it is a different function, by about what bf16 storage does
    d = float((rounded - ref).abs().max())
    assert 1e-6 < d < 0.1, d

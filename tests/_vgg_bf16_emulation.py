"""The bf16-emulating VGG19 feature extractor (oracle.models.vgg19_block5_conv4, upscaling/upscaler/model.py:101-157) on oracle.keras_ops:
what ``VGG19Features(dtype='bf16')`` and the bf16 branch of ``_content_loss_and_grad`` compute, with the rounding points switchable.

Forward (``forward``), rounding points with ``bf16=True``:
  * rounded as operands: the frames and every convolution kernel;
  * rounded when stored: every ReLU output (pooling selects stored values: exact);
  * kept unrounded (fp32 on the device, fp64 here): biases and the accumulation.
With ``bf16=False`` nothing is rounded and the function IS the oracle's (tests/test_vgg_bf16_emulation_cpu.py).

Backward (``backward``): a LINEAR map of the gradient dz in front of block5_conv4's ReLU, given the list of the sixteen stored ReLU
outputs: masks are [a > 0], the pooling gradient goes to the first maximum of each window, the kernels are the bf16-rounded ones
(``bf16_kernels``).  ``round_grads=True`` rounds the gradient to bf16 wherever the device stores one: after every data gradient that is
stored as bf16 (layers 16 .. 2; block1_conv1's result is the fp32 image gradient) -- the pooling backward copies stored values and the
loss kernel's rounding is ``loss_grad``'s.  Because the activations are an argument, a test can evaluate it on the DEVICE's own taps: the
comparison then has no ReLU / arg-max flips by construction.

``reference(shape)`` caches, per test shape, the frames, the fp64 oracle's features and the emulation's -- computed once and shared."""
import functools

import numpy as np
import torch

from oracle import keras_ops as K, models as M

LAYERS = [("block%d_conv%d" % (b, i + 1), i == 0) for b, nconv, _ in M.VGG19_BLOCKS for i in range(nconv)]     # (name, first of its block)
SHAPES = [(2, 64, 64, 3), (2, 40, 24, 3), (1, 32, 32, 3)]
D_REF_CAP = 1.5e-2          # relative L2 of the bf16 features against the fp64 oracle (measured 7.6e-3 .. 8.4e-3 on SHAPES)
E_CHAIN_CAP = 1.5e-2        # relative L2 of the gradient-rounding chain: seventeen roundings of 2^-9 / sqrt(3) rms predict 5e-3


def r_bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def forward(w, x_nhwc, bf16=True, taps=None):
    """w: torch weights dict; x_nhwc: frames.  Returns the block5_conv4 features (NHWC); taps receives the sixteen stored ReLU outputs (NCHW)"""
    r = r_bf16 if bf16 else (lambda t: t)
    x = r(x_nhwc.permute(0, 3, 1, 2))
    for name, first in LAYERS:
        if first and name != "block1_conv1":
            x = torch.nn.functional.max_pool2d(x, 2, 2)
        x = r(torch.relu(K.conv2d(x, r(w[name + "/kernel"]), w[name + "/bias"], 1, "same")))
        if taps is not None:
            taps.append(x)
    return x.permute(0, 2, 3, 1)


def _dgrad(kernel, dz, in_shape):
    """data gradient of a 3x3 'same' stride-1 convolution: the transpose of the oracle's own convolution, through its autograd"""
    x0 = torch.zeros(in_shape, dtype=dz.dtype, requires_grad=True)
    return torch.autograd.grad(K.conv2d(x0, kernel, None, 1, "same"), x0, dz)[0]


def _pool_bwd(a, dy):
    """gradient of max_pool2d(a, 2, 2) to the first maximum of each window; zero in rows / columns no window covers"""
    _, idx = torch.nn.functional.max_pool2d(a, 2, 2, return_indices=True)
    return torch.nn.functional.max_unpool2d(dy, idx, 2, 2, output_size=a.shape[-2:])


def backward(w, acts, dz, frames_shape, bf16_kernels=True, round_grads=True):
    """acts: the sixteen stored ReLU outputs (NCHW); dz: gradient in front of block5_conv4's ReLU (NCHW); frames_shape: (n, 3, h, w).
    Returns the image gradient (NCHW)."""
    rk = r_bf16 if bf16_kernels else (lambda t: t)
    rg = r_bf16 if round_grads else (lambda t: t)
    d = dz
    for k in range(15, 0, -1):
        name, first = LAYERS[k]
        a = acts[k - 1]
        if first:
            pooled_shape = (a.shape[0], a.shape[1], a.shape[2] // 2, a.shape[3] // 2)
            d = rg(_dgrad(rk(w[name + "/kernel"]), d, pooled_shape))
            d = _pool_bwd(a, d) * (a > 0)
        else:
            d = rg(_dgrad(rk(w[name + "/kernel"]), d, a.shape) * (a > 0))
    return _dgrad(rk(w["block1_conv1/kernel"]), d, tuple(frames_shape))


def loss_value(f_true, f_pred, kind):
    d = f_pred.double() - f_true.double()
    return float((d * d).mean() if kind == "mse" else d.abs().mean())


def loss_grad(f_true, f_pred, kind, grad_scale=1.0, round_grads=True):
    """gradient of grad_scale x the feature loss in front of the ReLU that produced f_pred (any layout; same shape as f_pred)"""
    d = f_pred.double() - f_true.double()
    g = (2.0 * d if kind == "mse" else torch.sign(d)) * (grad_scale / d.numel()) * (f_pred > 0)
    return r_bf16(g) if round_grads else g


def frames(shape):
    return (np.random.RandomState(3).randint(0, 256, shape) / 127.5 - 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def weights():
    return M.init_vgg19_features(seed=19)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """per test shape: frames (numpy fp32 NHWC), fp64 torch weights, the oracle's features and taps, the emulation's features and taps, d_ref"""
    x = frames(shape)
    w = M.to_torch(weights(), torch.float64)
    xt = torch.tensor(x, dtype=torch.float64)
    with torch.no_grad():
        otaps, etaps = [], []
        f_or = M.vgg19_block5_conv4(w, xt, otaps)
        f_em = forward(w, xt, True, etaps)
    return {"x": x, "w": w, "f_oracle": f_or, "taps_oracle": otaps, "f_emu": f_em, "taps_emu": etaps, "d_ref": rel_l2(f_em, f_or)}


@functools.lru_cache(maxsize=None)
def chain_error(shape):
    """e_chain: the backward with the gradient roundings against the same backward without them, on the emulation's own taps and a random
    bf16 gradient in front of block5_conv4's ReLU"""
    ref = reference(shape)
    a = ref["taps_emu"]
    g = torch.Generator().manual_seed(5)
    dz = r_bf16(torch.randn(a[-1].shape, generator=g, dtype=torch.float64)) * (a[-1] > 0)
    fs = (shape[0], 3, shape[1], shape[2])
    g_round = backward(ref["w"], a, dz, fs, True, True)
    g_exact = backward(ref["w"], a, dz, fs, True, False)
    return rel_l2(g_round, g_exact)

"""The storage-emulating forward of make_upscaler_attention(trunk_dtype='bf16', tail_dtype='bf16') on oracle.keras_ops: the rounding rules of
tests/_attention_bf16_train_emulation.py (whose trunk lines are repeated here unchanged) continued behind after_res/add:

  * operands (K.bf16_round_fwd): the gates' 6-channel input u = [nearest, bilinear resize of the frames] and the gate kernel, the
    Conv2DTranspose kernel, final/conv's kernel; biases stay fp32;
  * stores (K.bf16_store): the gate product sigmoid(a) * m, y_act = LeakyReLU(Conv2DTranspose + bias), y = y_act + to_add_input;
  * rounded in the backward only (K.bf16_round_grad): da in front of the gate convolution's bias, and dz in front of the LeakyReLU (what
    vcg_input_convt_add_bf16_bwd stores): y_act = st(lrelu(rg(convT + bias)));
  * to_add_input runs on its fp32 weights and the fp32 atanh of the unrounded frames; its result only exists inside the sum;
  * final/conv's output, the tanh and the gradient behind it are not rounded, as for the bf16 tail of make_upscaler_orig
    (oracle/models.py) and head/conv (tests/_cyclegan_bf16_train_emulation.py): the device rounds that gradient only as an MFMA operand.
With ``bf16=False`` it is oracle.models.upscaler_attention_forward (tests/test_train_attention_tail_emulation_cpu.py).

``training_case`` evaluates one case of tests/test_train_attention_tail_bf16_gpu.py once per process, as the trunk module's does."""
import math
from collections import OrderedDict

import numpy as np
import torch

from _attention_bf16_train_emulation import CASES, FLOOR, H, N, RES, W, allowed_zero_gradients, l2, randomized_weights  # noqa: F401
from oracle import keras_ops as K
from oracle.models import resize_images_tf1


def attention_tail_train_forward_emulated(w, x_nhwc, res_block_num, upscale_factor, training=True, bf16=True):
    """[N,h,w,3] -> ([N,h*f,w*f,3], {moving statistic: value after the step}); the kernel size is that of the weights"""
    rf = K.bf16_round_fwd if bf16 else (lambda v: v)
    st = K.bf16_store if bf16 else (lambda v: v)
    rg = K.bf16_round_grad if bf16 else (lambda v: v)
    upd = OrderedDict()

    def bn(z, name):
        y, mm, mv = K.batchnorm(z, w[name + "/gamma"], w[name + "/beta"], w[name + "/moving_mean"], w[name + "/moving_variance"], training)
        if training:
            upd[name + "/moving_mean"], upd[name + "/moving_variance"] = mm, mv
        return y

    def conv(x, name):          # a convolution on a bf16 kernel: bf16 copy of the fp32 master weights, fp32 bias
        return K.conv2d(x, rf(w[name + "/kernel"]), w[name + "/bias"], 1, "same")

    x = x_nhwc.permute(0, 3, 1, 2)
    xb = rf(x)
    m = st(K.prelu(conv(xb, "initial/conv"), w["initial/prelu/alpha"]))
    skip = m
    for i in range(res_block_num):
        n = "res_block/%d" % i
        gen = m
        m = st(torch.sigmoid(rg(conv(xb, n + "/attention"))) * m)
        m = st(K.prelu(bn(st(conv(m, n + "/conv_pre")), n + "/batch_norm_pre"), w[n + "/prelu/alpha"]))
        m = st(gen + bn(st(conv(m, n + "/conv_post")), n + "/batch_norm_post"))
    m = st(skip + bn(st(conv(m, "after_res/conv")), "after_res/batch_norm"))
    for i in range(int(math.log(upscale_factor, 2))):
        n, scale = "upscaling/%d/block" % i, 2 ** (i + 1)
        up = torch.cat([resize_images_tf1(x, scale // 2, "nearest"), resize_images_tf1(x, scale // 2, "bilinear")], 1)
        m = st(torch.sigmoid(rg(conv(rf(up), n + "/attention"))) * m)
        m = st(K.leaky_relu(rg(K.conv2d_transpose_same(m, rf(w[n + "/conv_transp/kernel"]), w[n + "/conv_transp/bias"], 2)), 0.2))
        t = torch.atanh(0.99999 * x)
        m = st(m + K.conv2d_transpose_same(t, w[n + "/to_add_input_conv_transp/kernel"], w[n + "/to_add_input_conv_transp/bias"], scale))
    m = torch.tanh(conv(m, "final/conv"))
    return m.permute(0, 2, 3, 1), upd


# Weight-draw seeds of the model test's cases (CASES of the trunk module, same sizes): per case a draw for which every gradient but the
# allowed zero ones stays above the floor in the emulation's fp64 and fp32 pass alike, now that the tail rounds too
# (tests/test_train_attention_tail_emulation_cpu.py asserts it).
SEEDS = {(3, 2): 5, (5, 4): 29, (3, 4): 6}
_cache = {}


def training_case(k, f):
    """dict: weights (numpy), x, t (numpy NHWC), and per dtype in ('f64', 'f32') the emulation's training output, loss, gradients, moving
    statistics and its learning-phase-0 output"""
    key = (k, f)
    if key in _cache:
        return _cache[key]
    from oracle import models as M
    wd = randomized_weights(k, f, SEEDS[key])
    x = (np.random.RandomState(1).randint(0, 256, (N, H, W, 3)) / 127.5 - 1).astype(np.float32)
    t = (np.random.RandomState(2).randint(0, 256, (N, f * H, f * W, 3)) / 127.5 - 1).astype(np.float32)
    out = dict(weights=wd, x=x, t=t)
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        leaf = M.to_torch(wd, dt, requires_grad=True)
        y, upd = attention_tail_train_forward_emulated(leaf, torch.tensor(x, dtype=dt), RES, f, True, bf16=True)
        loss = ((y - torch.tensor(t, dtype=dt)) ** 2).mean()
        names = [kk for kk, v in leaf.items() if v.requires_grad]
        grads = torch.autograd.grad(loss, [leaf[kk] for kk in names])
        with torch.no_grad():
            y0, _ = attention_tail_train_forward_emulated(leaf, torch.tensor(x, dtype=dt), RES, f, False, bf16=True)
        out[tag] = dict(y=y.detach().double(), loss=float(loss.detach()), grads=dict(zip(names, [g.double() for g in grads])),
                        upd={kk: v.detach().double().numpy() for kk, v in upd.items()}, y0=y0.double())
    _cache[key] = out
    return out


def below_floor(r):
    """names of the gradients of one pass (training_case(...)['f64' | 'f32']) that count as numerically zero"""
    gmax = max(float(g.abs().max()) for g in r["grads"].values())
    return sorted(kk for kk, b in r["grads"].items() if float(b.norm()) < FLOOR * gmax * b.numel() ** 0.5)

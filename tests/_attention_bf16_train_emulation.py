"""The storage-emulating forward of make_upscaler_attention(trunk_dtype='bf16') on oracle.keras_ops, in training mode (BatchNormalization
on the batch statistics of the tensor it reads, moving statistics returned) and in learning phase 0 (moving statistics), in the style of
tests/_cyclegan_bf16_train_emulation.py.  Autograd carries the rounding points into the backward pass:

  * operands (K.bf16_round_fwd: value rounded, gradient passed through to the fp32 master tensor): the frames as initial/conv and the
    residual blocks' gates read them, and every convolution kernel of the trunk; biases, BatchNormalization and PReLU parameters stay fp32;
  * stores (K.bf16_store: value rounded forward, gradient rounded backward): initial/prelu's output, the gate product sigmoid(a) * m
    (the attention tensor a itself is never stored), every z = convolution + bias in front of a norm -- the norm's statistics are those of
    the stored values --, every PReLU output, every final_add and after_res/add.  A block input feeds the gate (as m) and the Add: its two
    gradients are summed in fp32 and rounded once (the backward of its one bf16_store), which is what vcg_conv_in_gate_bf16_bwd does with
    its dres operand;
  * da, the gradient in front of the gate convolution's bias, is rounded in the backward only (K.bf16_round_grad: identity forward);
  * nothing is rounded after after_res/add: the up-sampling blocks and final/conv run in fp32 on the device.
Block 0's three-way join (gate, final_add, long skip) is rounded once here; the device rounds the first pair in the gate's kernel and the
sum with the long skip again where the PReLU backward stores its result.
With ``bf16=False`` it is oracle.models.upscaler_attention_forward (tests/test_train_attention_emulation_cpu.py).

``training_case`` evaluates one case of tests/test_train_attention_bf16_gpu.py -- output, MSE loss, every parameter gradient, moving
statistics, in fp64 and in fp32, and the learning-phase-0 output -- once per process."""
import math
from collections import OrderedDict

import numpy as np
import torch

from oracle import keras_ops as K
from oracle.models import resize_images_tf1


def attention_train_forward_emulated(w, x_nhwc, res_block_num, upscale_factor, training=True, bf16=True):
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
    for i in range(int(math.log(upscale_factor, 2))):          # fp32 from here on
        n, scale = "upscaling/%d/block" % i, 2 ** (i + 1)
        up = torch.cat([resize_images_tf1(x, scale // 2, "nearest"), resize_images_tf1(x, scale // 2, "bilinear")], 1)
        m = torch.sigmoid(K.conv2d(up, w[n + "/attention/kernel"], w[n + "/attention/bias"], 1, "same")) * m
        m = K.leaky_relu(K.conv2d_transpose_same(m, w[n + "/conv_transp/kernel"], w[n + "/conv_transp/bias"], 2), 0.2)
        t = torch.atanh(0.99999 * x)
        m = m + K.conv2d_transpose_same(t, w[n + "/to_add_input_conv_transp/kernel"], w[n + "/to_add_input_conv_transp/bias"], scale)
    m = torch.tanh(K.conv2d(m, w["final/conv/kernel"], w["final/conv/bias"], 1, "same"))
    return m.permute(0, 2, 3, 1), upd


# ---- the cases of the model test: (kernel_size, upscale_factor) on res_block_num 2, batch 2, 16 x 24 frames ----
CASES = [(3, 2), (5, 4), (3, 4)]
RES, N, H, W = 2, 2, 16, 24
FLOOR = 1e-4          # a gradient below FLOOR * max|g| * sqrt(numel) counts as numerically zero (test_cyclegan_bf16_training_forward_and_gradients)
# The floor is relative to the largest gradient element of the model, which is final/conv/bias's: with a random target its size follows
# the mean of y - t, i.e. the drawn biases (0.05 to 0.25 over the draws tried).  At x4 the trunk's gradients are about four orders of
# magnitude below that, so per case the draw is one where that element is small enough for every trunk tensor to stay above the floor
# -- in the emulation's fp64 and fp32 pass alike (tests/test_train_attention_emulation_cpu.py asserts it).
SEEDS = {(3, 2): 5, (5, 4): 29, (3, 4): 6}
_cache = {}


def randomized_weights(k, f, seed=None):
    """{name: float32 array}: kernels as the oracle initialises them; norm statistics, affine parameters, PReLU slopes and biases drawn as
    _cyclegan_bf16_train_emulation.randomized_weights draws them (seed: SEEDS[k, f])"""
    from oracle import models as M
    seed = SEEDS[(k, f)] if seed is None else seed
    w = M.init_upscaler_attention((f * H, f * W, 3), kernel_size=k, upscale_factor=f, res_block_num=RES, seed=7)
    rng = np.random.RandomState(seed)
    for name, v in w.items():
        if name.endswith("/gamma"):
            w[name] = rng.uniform(0.7, 1.3, v.shape).astype(np.float32)
        elif name.endswith(("/beta", "/moving_mean", "/bias")):
            w[name] = rng.uniform(-0.2, 0.2, v.shape).astype(np.float32)
        elif name.endswith("/moving_variance"):
            w[name] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif name.endswith("/alpha"):
            w[name] = rng.uniform(0.0, 0.3, v.shape).astype(np.float32)
    return w


def allowed_zero_gradients():
    """biases of convolutions that a BatchNormalization follows: the norm subtracts the mean, the bias gradient is zero up to rounding"""
    return set(["res_block/%d/conv_%s/bias" % (i, p) for i in range(RES) for p in ("pre", "post")] + ["after_res/conv/bias"])


def training_case(k, f):
    """dict: weights (numpy), x, t (numpy NHWC), and per dtype in ('f64', 'f32') the emulation's training output, loss, gradients, moving
    statistics and its learning-phase-0 output"""
    key = (k, f)
    if key in _cache:
        return _cache[key]
    from oracle import models as M
    wd = randomized_weights(k, f)
    x = (np.random.RandomState(1).randint(0, 256, (N, H, W, 3)) / 127.5 - 1).astype(np.float32)
    t = (np.random.RandomState(2).randint(0, 256, (N, f * H, f * W, 3)) / 127.5 - 1).astype(np.float32)
    out = dict(weights=wd, x=x, t=t)
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        leaf = M.to_torch(wd, dt, requires_grad=True)
        y, upd = attention_train_forward_emulated(leaf, torch.tensor(x, dtype=dt), RES, f, True, bf16=True)
        loss = ((y - torch.tensor(t, dtype=dt)) ** 2).mean()
        names = [kk for kk, v in leaf.items() if v.requires_grad]
        grads = torch.autograd.grad(loss, [leaf[kk] for kk in names])
        with torch.no_grad():
            y0, _ = attention_train_forward_emulated(leaf, torch.tensor(x, dtype=dt), RES, f, False, bf16=True)
        out[tag] = dict(y=y.detach().double(), loss=float(loss.detach()), grads=dict(zip(names, [g.double() for g in grads])),
                        upd={kk: v.detach().double().numpy() for kk, v in upd.items()}, y0=y0.double())
    _cache[key] = out
    return out


def l2(a, b, floor=0.0):
    return float((a - b).norm() / (b.norm() + floor))

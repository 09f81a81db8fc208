"""The storage-emulating TRAINING forward of make_generator_cyclegan(dtype='bf16') on oracle.keras_ops: tests/_cyclegan_bf16_emulation.py
with the norms in training mode (BatchNormalization on the batch statistics of the tensor it reads, moving statistics returned; instance
norm as before) and the same rounding points, which autograd carries into the backward pass:

  * operands: the frames as stem/conv reads them and every convolution kernel (K.bf16_round_fwd: value rounded, gradient passed
    through to the fp32 master tensor); biases, BatchNormalization and PReLU parameters stay fp32;
  * stores (K.bf16_store: value rounded forward, gradient rounded backward): every z = convolution + bias, in front of its norm -- the
    norm's statistics are those of the stored values, and the gradient the norm's backward hands the convolution is stored in bf16 --,
    every PReLU output and every final_add.  A block input feeds conv_pre and the Add: its two gradients are summed in fp32 and rounded
    once (the backward of its one bf16_store), which is what vcg_conv2d_nhwc_bf16_dgrad_add does;
  * not rounded: head/conv's output and the gradient arriving there (fp32 on the device).
With ``bf16=False`` it is oracle.generators.generator_cyclegan in training mode (tests/test_train_cyclegan_emulation_cpu.py).

``training_case`` evaluates one case of tests/test_train_cyclegan_bf16_gpu.py -- output, MSE loss, every parameter gradient, moving
statistics, in fp64 and in fp32 -- once per process."""
import math
from collections import OrderedDict

import numpy as np
import torch

from oracle import keras_ops as K


def cyclegan_train_forward_emulated(w, x_nhwc, n_downsample=2, res_block_num=9, upscale_factor=1, norm="instance", bf16=True):
    """[N,h,w,3] -> ([N,h*f,w*f,3], {moving statistic: value after the step}); the kernel size is that of the weights"""
    rf = K.bf16_round_fwd if bf16 else (lambda v: v)
    st = K.bf16_store if bf16 else (lambda v: v)
    upd = OrderedDict()

    def nrm(z, name):
        if norm == "instance":
            return K.instancenorm(z)
        y, mm, mv = K.batchnorm(z, w[name + "/gamma"], w[name + "/beta"], w[name + "/moving_mean"], w[name + "/moving_variance"], True)
        upd[name + "/moving_mean"], upd[name + "/moving_variance"] = mm, mv
        return y

    def conv(x, name, stride):
        return st(K.conv2d(x, rf(w[name + "/kernel"]), w[name + "/bias"], stride, "same"))

    def convt(x, name):
        return st(K.conv2d_transpose_same(x, rf(w[name + "/kernel"]), w[name + "/bias"], 2))

    def act(z, nname, pname):
        return st(K.prelu(nrm(z, nname), w[pname + "/alpha"]))

    m = rf(x_nhwc.permute(0, 3, 1, 2))
    m = act(conv(m, "stem/conv", 1), "stem/norm", "stem/prelu")
    for i in range(n_downsample):
        m = act(conv(m, "down/%d/conv" % i, 2), "down/%d/norm" % i, "down/%d/prelu" % i)
    for i in range(res_block_num):
        n = "res_block/%d" % i
        gen = m
        m = act(conv(m, n + "/conv_pre", 1), n + "/batch_norm_pre", n + "/prelu")
        m = st(gen + nrm(conv(m, n + "/conv_post", 1), n + "/batch_norm_post"))
    for i in range(n_downsample + int(math.log(upscale_factor, 2))):
        m = act(convt(m, "up/%d/conv_transp" % i), "up/%d/norm" % i, "up/%d/prelu" % i)
    m = torch.tanh(K.conv2d(m, rf(w["head/conv/kernel"]), w["head/conv/bias"], 1, "same"))
    return m.permute(0, 2, 3, 1), upd


# ---- the cases of the model test: (norm, upscale_factor, n_downsample) on res_block_num 2, batch 2, 16 x 24 frames ----
CASES = [("instance", 1, 2), ("batch", 2, 2), ("instance", 4, 1)]
RES, N, H, W = 2, 2, 16, 24
FLOOR = 1e-4          # a gradient below FLOOR * max|g| * sqrt(numel) counts as numerically zero (test_k5_x4_generator_training_forward_and_gradients)
_cache = {}


def randomized_weights(norm, f, down, seed=5):
    """{name: float32 array}: Glorot kernels as the oracle initialises them; norm statistics, affine parameters, PReLU slopes and biases
    drawn as tests/test_train_k5_bf16_gpu.py's _randomize_bn draws them"""
    from oracle import generators as OG
    w = OG.init_weights(OG.generator_cyclegan, (H, W, 3), 7, filters=64, n_downsample=down, res_block_num=RES, upscale_factor=f, norm=norm, kernel_size=3)
    rng = np.random.RandomState(seed)
    for k, v in w.items():
        if k.endswith("/gamma"):
            w[k] = rng.uniform(0.7, 1.3, v.shape).astype(np.float32)
        elif k.endswith(("/beta", "/moving_mean", "/bias")):
            w[k] = rng.uniform(-0.2, 0.2, v.shape).astype(np.float32)
        elif k.endswith("/moving_variance"):
            w[k] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif k.endswith("/alpha"):
            w[k] = rng.uniform(0.0, 0.3, v.shape).astype(np.float32)
    return w


def allowed_zero_gradients(f, down):
    """biases of convolutions that a norm follows: the norm subtracts the mean, the bias gradient is zero up to rounding"""
    names = ["stem/conv/bias"] + ["down/%d/conv/bias" % i for i in range(down)]
    names += ["res_block/%d/conv_%s/bias" % (i, p) for i in range(RES) for p in ("pre", "post")]
    names += ["up/%d/conv_transp/bias" % i for i in range(down + int(math.log(f, 2)))]
    return set(names)


def training_case(norm, f, down):
    """dict: weights (numpy), x, t (numpy NHWC), and per dtype in ('f64', 'f32') the emulation's output, loss, gradients, moving statistics"""
    key = (norm, f, down)
    if key in _cache:
        return _cache[key]
    from oracle import models as M
    wd = randomized_weights(norm, f, down)
    x = (np.random.RandomState(1).randint(0, 256, (N, H, W, 3)) / 127.5 - 1).astype(np.float32)
    t = (np.random.RandomState(2).randint(0, 256, (N, f * H, f * W, 3)) / 127.5 - 1).astype(np.float32)
    out = dict(weights=wd, x=x, t=t)
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        leaf = M.to_torch(wd, dt, requires_grad=True)
        y, upd = cyclegan_train_forward_emulated(leaf, torch.tensor(x, dtype=dt), down, RES, f, norm, bf16=True)
        loss = ((y - torch.tensor(t, dtype=dt)) ** 2).mean()
        names = [k for k, v in leaf.items() if v.requires_grad]
        grads = torch.autograd.grad(loss, [leaf[k] for k in names])
        out[tag] = dict(y=y.detach().double(), loss=float(loss.detach()), grads=dict(zip(names, [g.double() for g in grads])),
                        upd={k: v.detach().double().numpy() for k, v in upd.items()})
    _cache[key] = out
    return out


def l2(a, b, floor=0.0):
    return float((a - b).norm() / (b.norm() + floor))

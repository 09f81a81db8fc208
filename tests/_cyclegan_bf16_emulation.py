"""The bf16-emulating forward of make_generator_cyclegan (oracle.generators.generator_cyclegan) on oracle.keras_ops: what
``Bf16CycleGanGenerator`` computes, with its storage roundings marked, as tests/_attention_bf16_emulation.py does for the attention
generator.  Inference only (BatchNormalization on its moving statistics; instance norm on the statistics of the tensor it reads).

Rounding points (``bf16=True``):
  * operands: the frames as stem/conv reads them and every convolution kernel -- all of them run on bf16 kernels -- (K.bf16_round_fwd);
    biases, BatchNormalization and PReLU parameters stay fp32;
  * stores (K.bf16_store): every z = convolution + bias, in front of its norm -- the norm's statistics are those of the stored values --,
    every PReLU output and every final_add;
  * not rounded: head/conv's output (fp32 on the device).
With ``bf16=False`` no rounding happens and the function is oracle.generators.generator_cyclegan (tests/test_cyclegan_emulation_cpu.py).

``taps``: a dict that receives every stored tensor (NCHW) under the name the engine's ``forward(x, taps=...)`` uses."""
import math

import torch

from oracle import keras_ops as K


def cyclegan_forward_emulated(w, x_nhwc, n_downsample=2, res_block_num=9, upscale_factor=1, norm="instance", bf16=True, taps=None):
    """[N,h,w,3] -> [N,h*f,w*f,3]; the kernel size is that of the weights"""
    rf = K.bf16_round_fwd if bf16 else (lambda v: v)
    st = K.bf16_store if bf16 else (lambda v: v)

    def keep(name, t):
        if taps is not None:
            taps[name] = t
        return t

    def nrm(z, name):
        if norm == "instance":
            return K.instancenorm(z)
        y, _, _ = K.batchnorm(z, w[name + "/gamma"], w[name + "/beta"], w[name + "/moving_mean"], w[name + "/moving_variance"], False)
        return y

    def conv(x, name, stride):
        return keep(name, st(K.conv2d(x, rf(w[name + "/kernel"]), w[name + "/bias"], stride, "same")))

    def convt(x, name):
        return keep(name, st(K.conv2d_transpose_same(x, rf(w[name + "/kernel"]), w[name + "/bias"], 2)))

    def act(z, nname, pname):
        return keep(pname, st(K.prelu(nrm(z, nname), w[pname + "/alpha"])))

    m = rf(x_nhwc.permute(0, 3, 1, 2))
    m = act(conv(m, "stem/conv", 1), "stem/norm", "stem/prelu")
    for i in range(n_downsample):
        m = act(conv(m, "down/%d/conv" % i, 2), "down/%d/norm" % i, "down/%d/prelu" % i)
    for i in range(res_block_num):
        n = "res_block/%d" % i
        gen = m
        m = act(conv(m, n + "/conv_pre", 1), n + "/batch_norm_pre", n + "/prelu")
        m = keep(n + "/final_add", st(gen + nrm(conv(m, n + "/conv_post", 1), n + "/batch_norm_post")))
    for i in range(n_downsample + int(math.log(upscale_factor, 2))):
        m = act(convt(m, "up/%d/conv_transp" % i), "up/%d/norm" % i, "up/%d/prelu" % i)
    m = keep("head/conv", torch.tanh(K.conv2d(m, rf(w["head/conv/kernel"]), w["head/conv/bias"], 1, "same")))
    return m.permute(0, 2, 3, 1)

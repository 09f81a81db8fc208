"""The bf16-emulating forward of make_upscaler_attention (upscaling/upscaler/model.py:299-328) on oracle.keras_ops: what
``Bf16AttentionGenerator`` computes, with its storage roundings marked, as ``upscaler_orig_forward(trunk_bf16=True, tail_bf16=True,
fold_inference=True)`` does for make_upscaler_orig.  Inference only (BatchNormalization on its moving statistics).

Rounding points (``bf16=True``):
  * operands: the frames and the resized [nearest, bilinear] inputs as read by initial/conv and by the attention convolutions, and every
    convolution kernel that runs on a bf16 kernel (K.bf16_round_fwd); biases, BatchNormalization and PReLU parameters stay fp32;
  * stores: initial/prelu, the gate product sigmoid(a) * m (once; the attention tensor a itself is never stored), the trunk tensors as in the
    orig emulation (conv + folded BN + PReLU, conv + folded BN + Add), after_res/add, each stage's LeakyReLU output, and the to_add sum
    again;
  * not rounded: the atanh branch, its Conv2DTranspose kernel and bias (fp32 on the device).
With ``bf16=False`` no rounding happens and the function is oracle.models.upscaler_attention_forward (tests/test_attention_emulation_cpu.py)."""
import math

import torch

from oracle import keras_ops as K
from oracle.models import resize_images_tf1


def attention_forward_emulated(w, x_nhwc, res_block_num, upscale_factor, bf16=True):
    """[N,h,w,3] -> [N,h*f,w*f,3]"""
    rf = K.bf16_round_fwd if bf16 else (lambda v: v)
    st = K.bf16_store if bf16 else (lambda v: v)

    def bn(x, name):
        y, _, _ = K.batchnorm(x, w[name + "/gamma"], w[name + "/beta"], w[name + "/moving_mean"], w[name + "/moving_variance"], False)
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
        m = st(torch.sigmoid(conv(xb, n + "/attention")) * m)
        m = st(K.prelu(bn(conv(m, n + "/conv_pre"), n + "/batch_norm_pre"), w[n + "/prelu/alpha"]))
        m = st(gen + bn(conv(m, n + "/conv_post"), n + "/batch_norm_post"))
    m = st(skip + bn(conv(m, "after_res/conv"), "after_res/batch_norm"))
    for i in range(int(math.log(upscale_factor, 2))):
        n, scale = "upscaling/%d/block" % i, 2 ** (i + 1)
        up = torch.cat([resize_images_tf1(x, scale // 2, "nearest"), resize_images_tf1(x, scale // 2, "bilinear")], 1)
        m = st(torch.sigmoid(conv(rf(up), n + "/attention")) * m)
        m = st(K.leaky_relu(K.conv2d_transpose_same(m, rf(w[n + "/conv_transp/kernel"]), w[n + "/conv_transp/bias"], 2), 0.2))
        t = torch.atanh(0.99999 * x)
        t = K.conv2d_transpose_same(t, w[n + "/to_add_input_conv_transp/kernel"], w[n + "/to_add_input_conv_transp/bias"], scale)
        m = st(m + t)
    m = torch.tanh(conv(m, "final/conv"))
    return m.permute(0, 2, 3, 1)

"""The fp32 convolution kernels' tile prologue and epilogue (csrc/conv_fwd.hip: conv_fwd_kernel, conv_c3_kernel) at the
smallest shapes where their address paths can go wrong.  The epilogue writes y -- and reads the residual -- through one
buffer descriptor per (image, 64-channel block) with 32-bit offsets, drops the channels past cout by the descriptor's
size and the rows / columns past the ragged edge by an out-of-range offset; the prologue carries the halo tile's
(channel, row, column) from one staged element to the next.  So: cin no multiple of the chunk, cout no multiple of 64,
ragged bottom and right edges, a partial second x-tile of the 64-column instantiation, more than one image and channel
block, every stride / kernel size with its own instantiation, bias, LeakyReLU, PReLU, residual, flipped taps.

Reference: the fp64 oracle (oracle.keras_ops) under TOL = 1e-3, the file-wide bound of tests/test_kernels_gpu.py (the
kernels are exact fp32 FMA chains: errors of about 1e-6 are what is seen).  The statistics case uses the bound of
test_kernels_gpu.test_conv2d_stats_epilogue_matches_the_statistics_pass (1e-5)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err, report

pytestmark = pytest.mark.gpu
TOL = 1e-3           # the file-wide bound of tests/test_kernels_gpu.py

# kind, cin, cout, k, stride, padding, n, h, w, epilogue
#   epilogue: "prelu" = bias + per-channel PReLU (C ABI's prelu_alpha), "lrelu_res" = bias + LeakyReLU(0.2) + residual, None = bias
CASES = {
    "k3_ragged": ("conv", 5, 70, 3, 1, "same", 2, 13, 75, "prelu"),        # XT=2, partial second x-tile, ragged rows, cout = 64 + 6
    "k3_interior": ("conv", 5, 64, 3, 1, "same", 2, 16, 128, "lrelu_res"),  # every tile full
    "k3_ow30": ("conv", 5, 70, 3, 1, "same", 2, 13, 30, "prelu"),          # the 32-column instantiation
    "k4s1": ("conv", 40, 72, 4, 1, 1, 2, 41, 71, None),
    "k4s2": ("conv", 12, 130, 4, 2, 1, 2, 37, 50, None),
    "k3s2": ("conv", 12, 70, 3, 2, "same", 2, 13, 37, None),
    "convT_k3": ("convT", 70, 12, 3, 2, "same", 2, 7, 19, None),           # its data gradient is the 3x3 stride-2 kernel on 14x38 -> 7x19
    "k5": ("conv", 12, 70, 5, 1, "same", 2, 20, 40, None),
    "c3_fwd": ("conv", 3, 70, 9, 1, "same", 2, 20, 45, None),              # conv_c3_kernel
    "c3_dgrad": ("conv", 70, 3, 9, 1, "same", 2, 20, 45, None),            # its data gradient: conv_c3_kernel, flipped taps, 3 -> 70
}
FWD = ["k3_ragged", "k3_interior", "k3_ow30", "k4s1", "k4s2", "k3s2", "k5", "c3_fwd"]
DGRAD = ["k3_ragged", "k4s1", "k4s2", "convT_k3", "c3_dgrad"]              # the Conv2D ones with a skip gradient added

_REF = {}


def _case(rt, name):
    """layer, parameters, device inputs and the fp64 references of one case: computed once, shared, never written to"""
    if name in _REF:
        return _REF[name]
    from upscaler import _engine as E, _lib as L
    from oracle import keras_ops as K
    from test_kernels_gpu import _standalone
    kind, cin, cout, k, stride, padding, n, h, w, epi = CASES[name]
    act, alpha = (L.ACT_LRELU, 0.2) if epi == "lrelu_res" else (L.ACT_NONE, 0.0)
    layer = E.Conv2D("c", cin, cout, k, stride, padding, act, alpha) if kind == "conv" else E.ConvT2D("c", cin, cout, k)
    ps, wd = _standalone(rt, layer, seed=cin + cout + k)
    g = torch.Generator().manual_seed(23)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    zr = K.conv2d(xr, wd["c/kernel"], wd["c/bias"], stride, padding) if kind == "conv" else K.conv2d_transpose_same(xr, wd["c/kernel"], wd["c/bias"], 2)
    res = torch.randn(*zr.shape, generator=g, dtype=torch.float64)
    slopes = torch.rand(cout, generator=g, dtype=torch.float64) - 0.25
    dy = torch.randn(*zr.shape, generator=g, dtype=torch.float64)
    skip = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    (zr * dy).sum().backward()                                               # data gradient of the layer without activation
    if epi == "prelu":
        yr = K.prelu(zr.detach(), slopes)
    elif epi == "lrelu_res":
        yr = K.leaky_relu(zr.detach(), 0.2) + res
    else:
        yr = zr.detach()
    dev = lambda t: t.float().to(rt.device)
    _REF[name] = dict(layer=layer, ps=ps, x=dev(x), res=dev(res), slopes=dev(slopes), dy=dev(dy), skip=dev(skip),
                      y_ref=yr, dx_ref=xr.grad.detach(), skip64=skip, epi=epi)
    return _REF[name]


def _forward(rt, c):
    from upscaler import _lib as L
    layer, epi = c["layer"], c["epi"]
    if epi == "prelu":
        # no layer fuses PReLU into a convolution: the layer's descriptor and parameters, the C ABI's epilogue
        n, _, h, w = c["x"].shape
        d = layer.desc(n, h, w)
        y = rt.empty(n, layer.cout, d.oh, d.ow)
        ep = L.Epilogue(c["ps"]["c/bias"].data_ptr(), L.ACT_PRELU, 0.0, c["slopes"].data_ptr(), None)
        L.check(rt.lib.vcg_conv2d_fwd(ctypes.byref(d), c["x"].data_ptr(), c["ps"]["c/kernel"].data_ptr(), y.data_ptr(), ctypes.byref(ep), rt.stream),
                "vcg_conv2d_fwd")
        return y
    if epi == "lrelu_res":
        return layer.forward(c["x"], residual=c["res"])[0]
    return layer.forward(c["x"])[0]


@pytest.mark.parametrize("name", FWD)
def test_conv_forward_edges(rt, name):
    c = _case(rt, name)
    e = rel_err(_forward(rt, c), c["y_ref"])
    report("conv f32 edges fwd   %-12s %.3e" % (name, e))
    assert e < TOL


@pytest.mark.parametrize("name", DGRAD)
def test_conv_dgrad_edges(rt, name):
    """the data gradient runs the same kernels with flipped taps (stride 1), as a stride-2 convolution (ConvT2D) or through the
    transposed kernel (stride 2); the skip gradient of a residual block is the `residual` of that launch"""
    from upscaler import _engine as E
    c = _case(rt, name)
    layer = c["layer"]
    if isinstance(layer, E.ConvT2D):
        _, ctx = layer.forward(c["x"])
        dx, ref = layer.backward(ctx, c["dy"], True, False, 0), c["dx_ref"]
    else:
        ctx = (c["x"], None, layer.desc(*[c["x"].shape[i] for i in (0, 2, 3)]))
        dx, ref = layer.backward(ctx, c["dy"], True, False, 0, dx_residual=c["skip"]), c["dx_ref"] + c["skip64"]
    e = rel_err(dx, ref)
    report("conv f32 edges dgrad %-12s %.3e" % (name, e))
    assert e < TOL


def test_conv_stats_epilogue_on_ragged_tiles(rt):
    """the first shape in front of a BatchNormalization: mean and 1/sigma from the convolution's statistics epilogue
    (vcg_norm_finalize_partials_shifted) against the fp64 statistics of the output"""
    from upscaler import _engine as E, _lib as L
    from test_kernels_gpu import _standalone
    _, cin, cout, k, stride, padding, n, h, w, _ = CASES["k3_ragged"]
    conv = E.Conv2D("c", cin, cout, k, stride, padding)
    _standalone(rt, conv, seed=cin + cout + h)
    norm = E.NormAct("nm", cout, "batch", L.ACT_PRELU, 0.0, prelu_name="pr")
    _standalone(rt, norm, seed=3)
    x = torch.randn(n, cin, h, w, generator=torch.Generator().manual_seed(h * 100 + w)).to(rt.device)
    y, _, st = conv.forward_stats(x, False)
    assert st is not None, "this shape must be served by the statistics epilogue"
    y_ref, _ = conv.forward(x)
    assert torch.equal(y, y_ref)
    _, ctx = norm.forward(y, True, stats=st)
    yd = y_ref.double().cpu()
    mean64, var64 = yd.mean((0, 2, 3)), yd.var((0, 2, 3), unbiased=False)
    mean, invstd = ctx[1]
    e_mean = float(((mean.cpu().double().reshape(mean64.shape) - mean64).abs() / (var64.sqrt() + 1e-6)).max())
    e_is = rel_err(invstd.cpu().double().reshape(var64.shape), 1.0 / torch.sqrt(var64 + 1e-3))
    report("conv f32 edges stats k3_ragged mean (in sigmas)=%.2e invstd=%.2e" % (e_mean, e_is))
    assert e_mean < 1e-5 and e_is < 1e-5


def test_conv_edges_are_deterministic(rt):
    c = _case(rt, "k3_ragged")
    assert torch.equal(_forward(rt, c), _forward(rt, c))
    c = _case(rt, "k3_interior")
    assert torch.equal(_forward(rt, c), _forward(rt, c))


@pytest.mark.parametrize("cin,k", [(8, 3), (3, 9)])
def test_conv_block_past_32_bit_offsets_is_unsupported(rt, cin, k):
    """include/vcg.h: a 64-channel block of one output image must stay below 0xFFFFFFE0 bytes.  Asked from the shape
    arguments alone: the answer comes before anything is launched, the pointers are never followed."""
    from upscaler import _lib as L
    side = 4100                                                  # 64 channels x 4100^2 pixels x 4 bytes = 4.30e9 > 0xFFFFFFE0
    assert 64 * side * side * 4 > 0xFFFFFFE0
    d = L.ConvDesc(1, cin, side, side, 64, side, side, k, k, 1, k // 2, k // 2)
    token = rt.empty(4)
    ep = L.Epilogue(None, L.ACT_NONE, 0.0, None, None)
    rc = rt.lib.vcg_conv2d_fwd(ctypes.byref(d), token.data_ptr(), token.data_ptr(), token.data_ptr(), ctypes.byref(ep), rt.stream)
    assert rc == L.E_UNSUPPORTED

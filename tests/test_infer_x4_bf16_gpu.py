"""bf16 inference of the reference's DEFAULT generator (make_upscaler_orig(shape): kernel_size 5, upscale_factor 4, 16 residual blocks;
upscaling/upscaler/model.py:267) and of the other k / upscale_factor topologies: the 5x5 trunk convolution of vcg_conv2d_bf16_fwd (the
generic kernels with the folded-BN / PReLU / residual epilogue), the stride-2 transposed convolutions the engine runs for these
topologies (vcg_conv_transpose2d_nhwc_bf16_fwd: 5x5, and 3x3 on 256 channels), and Bf16Generator end to end.

Kernel bounds as in test_bf16_gpu.py: fp64 oracle on the SAME bf16-rounded operands, max-norm relative error < 2^-8 and the ulp-scaled
element-wise check < 1.  End-to-end bounds as the C5 tests: the bf16-emulating oracle within 2.5x the emulation's own fp32-vs-fp64
distance (computed here), the plain fp64 oracle within 3e-2."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err, report

pytestmark = pytest.mark.gpu
TOL_BF16 = 2.0 ** -8


def _bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _to_nhwc_bf16(rt, x):
    from upscaler import _lib as L
    n, c, h, w = x.shape
    y = torch.empty(n, h, w, c, dtype=torch.bfloat16, device=rt.device)
    L.check(rt.lib.vcg_f32_nchw_to_bf16_nhwc(x.data_ptr(), y.data_ptr(), n, c, h, w, rt.stream), "to_bf16")
    return y


def _nchw(y):
    return y.float().permute(0, 3, 1, 2).cpu().double()


def _ulp_scaled(got, ref):
    return float(((got - ref).abs() / (ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max())).max())


def _randomize_bn(G, seed):
    """non-trivial BatchNormalization statistics / affine parameters / PReLU slopes, as after training (test_bf16_gpu.py)"""
    rng = np.random.RandomState(seed)
    w = G.get_weights_dict()
    for k, v in w.items():
        if k.endswith("/gamma"):
            w[k] = rng.uniform(0.7, 1.3, v.shape).astype(np.float32)
        elif k.endswith(("/beta", "/moving_mean", "/bias")):
            w[k] = rng.uniform(-0.2, 0.2, v.shape).astype(np.float32)
        elif k.endswith("/moving_variance"):
            w[k] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif k.endswith("/alpha"):
            w[k] = rng.uniform(0.0, 0.3, v.shape).astype(np.float32)
    G.set_weights_dict(w)
    return w


# ---- 1. the 5x5 trunk convolution ---------------------------------------------------------------------------------------------------
EPILOGUES = ["plain", "affine", "affine_prelu", "affine_res", "lrelu"]
SHAPES = [(1, 8, 32), (2, 16, 64), (1, 13, 45), (3, 40, 72), (2, 5, 7), (1, 1, 1)]


@pytest.mark.parametrize("n,h,w", SHAPES)
@pytest.mark.parametrize("epi", EPILOGUES)
def test_conv5x5_c64_bf16(rt, n, h, w, epi):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + w + len(epi))
    x = torch.randn(n, 64, h, w, generator=g)
    wk = torch.randn(5, 5, 64, 64, generator=g) * 0.04            # Keras (kh,kw,in,out)
    affine = epi.startswith("affine")
    scale, shift = torch.rand(64, generator=g) + 0.5, torch.rand(64, generator=g) - 0.5
    alpha = torch.rand(64, generator=g) * 0.5
    res = torch.randn(n, 64, h, w, generator=g)
    xd = _to_nhwc_bf16(rt, x.to(rt.device))
    wd = wk.to(rt.device)
    wp = torch.empty(25, 64, 64, dtype=torch.bfloat16, device=rt.device)           # the generic kernels' fragments (mode 0: forward)
    L.check(rt.lib.vcg_pack_conv_frag_bf16(wd.data_ptr(), 25, 64, 64, 0, wp.data_ptr(), rt.stream), "pack frag")
    rd = _to_nhwc_bf16(rt, res.to(rt.device))
    sd, hd, ad = scale.to(rt.device), shift.to(rt.device), alpha.to(rt.device)
    y = torch.full((n, h, w, 64), float("nan"), dtype=torch.bfloat16, device=rt.device)
    d = L.ConvDesc(n, 64, h, w, 64, h, w, 5, 5, 1, 2, 2)
    ep = L.EpilogueBf16(sd.data_ptr() if affine else None, hd.data_ptr() if affine else None,
                        {"affine_prelu": L.ACT_PRELU, "lrelu": L.ACT_LRELU}.get(epi, L.ACT_NONE), 0.2,
                        ad.data_ptr() if epi == "affine_prelu" else None, rd.data_ptr() if epi == "affine_res" else None)
    L.check(rt.lib.vcg_conv2d_bf16_fwd(ctypes.byref(d), xd.data_ptr(), wp.data_ptr(), y.data_ptr(), ctypes.byref(ep), rt.stream),
            "vcg_conv2d_bf16_fwd")
    got = _nchw(y)
    ref = K.conv2d(_bf16_round(x), _bf16_round(wk), None, 1, "same")
    if affine:
        ref = ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if epi == "affine_prelu":
        ref = torch.clamp(ref, min=0) + alpha.double().view(1, -1, 1, 1) * torch.clamp(ref, max=0)
    if epi == "lrelu":
        ref = torch.where(ref >= 0, ref, 0.2 * ref)
    if epi == "affine_res":
        ref = ref + _bf16_round(res)
    e, ew = rel_err(got, ref), _ulp_scaled(got, ref)
    report("bf16 conv5x5 c64 n=%d %dx%d %s  err=%.2e  elementwise(ulp-scaled)=%.2f" % (n, h, w, epi, e, ew))
    assert e < TOL_BF16 and ew < 1.0


# ---- 2. the stride-2 transposed convolutions ---------------------------------------------------------------------------------------
CT_CASES = [
    # k, cin, n, h, w, lrelu
    (5, 64, 2, 12, 32, True),
    (5, 64, 1, 13, 45, False),
    (5, 256, 2, 9, 17, True),
    (5, 256, 1, 5, 7, False),
    (5, 256, 3, 20, 36, True),
    (3, 256, 2, 11, 33, True),
    (3, 256, 1, 7, 5, False),
    (5, 64, 1, 1, 1, True),
]


@pytest.mark.parametrize("k,cin,n,h,w,lrelu", CT_CASES)
def test_conv_transpose_s2_bf16(rt, k, cin, n, h, w, lrelu):
    """the up-sampling stages of the k5 / x4 topologies as the engine runs them (vcg_conv_transpose2d_nhwc_bf16_fwd, weights packed
    with mode 1); the entry point of the k3 64-channel stage does not take these shapes"""
    from oracle import keras_ops as K
    from upscaler import _lib as L
    cout = 256
    g = torch.Generator().manual_seed(k * 100000 + cin * 100 + h * 10 + w)
    x = torch.randn(n, cin, h, w, generator=g)
    wk = torch.randn(k, k, cout, cin, generator=g) * (0.5 / (k * (cin ** 0.5)))    # Keras Conv2DTranspose (kh,kw,out,in)
    bias = torch.randn(cout, generator=g) * 0.3
    xd = _to_nhwc_bf16(rt, x.to(rt.device))
    wd, bd = wk.to(rt.device), bias.to(rt.device)
    crop = (k - 2) // 2
    d = L.ConvDesc(n, cin, h, w, cout, 2 * h, 2 * w, k, k, 2, crop, crop)
    act = L.ACT_LRELU if lrelu else L.ACT_NONE
    wfr = torch.empty(k * k * cout * cin, dtype=torch.bfloat16, device=rt.device)
    L.check(rt.lib.vcg_pack_conv_frag_bf16(wd.data_ptr(), k * k, cout, cin, 1, wfr.data_ptr(), rt.stream), "pack frag")
    y = torch.full((n, 2 * h, 2 * w, cout), float("nan"), dtype=torch.bfloat16, device=rt.device)
    L.check(rt.lib.vcg_conv_transpose2d_nhwc_bf16_fwd(ctypes.byref(d), xd.data_ptr(), wfr.data_ptr(), bd.data_ptr(), act, 0.2, y.data_ptr(),
                                                      rt.stream), "vcg_conv_transpose2d_nhwc_bf16_fwd")
    got = _nchw(y)
    ref = K.conv2d_transpose_same(_bf16_round(x), _bf16_round(wk), bias.double(), 2)
    if lrelu:
        ref = torch.where(ref >= 0, ref, 0.2 * ref)
    e, ew = rel_err(got, ref), _ulp_scaled(got, ref)
    report("bf16 convT%dx%d s2 %d->%d (generic) n=%d %dx%d lrelu=%s  err=%.2e  elementwise(ulp-scaled)=%.2f" % (k, k, cin, cout, n, h, w, lrelu, e, ew))
    assert e < TOL_BF16 and ew < 1.0


# ---- 3. the reference's default generator end to end --------------------------------------------------------------------------------
def _emulation_bounds(wd, x, res, f, k_unused=None, norm="batch"):
    """the bf16-emulating oracle in fp64 (the reference output of a bf16 engine) and its own fp32-vs-fp64 distance (the yardstick)"""
    from oracle import models as M
    with torch.no_grad():
        y64, _ = M.upscaler_orig_forward(M.to_torch(wd, torch.float64), torch.tensor(x, dtype=torch.float64), False, res, f,
                                         norm=norm, trunk_bf16=True, tail_bf16=True)
        y32, _ = M.upscaler_orig_forward(M.to_torch(wd, torch.float32), torch.tensor(x, dtype=torch.float32), False, res, f,
                                         norm=norm, trunk_bf16=True, tail_bf16=True)
        yp, _ = M.upscaler_orig_forward(M.to_torch(wd, torch.float64), torch.tensor(x, dtype=torch.float64), False, res, f, norm=norm)
    y64, y32, yp = y64.numpy(), y32.double().numpy(), yp.numpy()
    d_max = rel_err(y32, y64)
    d_l2 = float(np.linalg.norm(y32 - y64) / np.linalg.norm(y64))
    return y64, yp, d_max, d_l2


def _check_generator(G, wd, x, res, f, label, norm="batch"):
    inf = G.to_inference_bf16()
    got = inf.predict(x)
    got2 = inf.predict(x)                                   # second call: pure graph replay
    assert got.shape == (x.shape[0], x.shape[1] * f, x.shape[2] * f, 3)
    assert np.array_equal(got, got2)
    y64, yp, d_max, d_l2 = _emulation_bounds(wd, x, res, f, norm=norm)
    g = got.astype(np.float64)
    e_max, e_l2 = rel_err(g, y64), float(np.linalg.norm(g - y64) / np.linalg.norm(y64))
    e_plain, e_plain_l2 = rel_err(g, yp), float(np.linalg.norm(g - yp) / np.linalg.norm(yp))
    # what bf16 storage alone does to the output, in exact arithmetic: the emulating oracle against the plain one (both fp64)
    d_store = rel_err(y64, yp)
    # the plain fp64 oracle: max-norm 3e-2 as the C5 test bounds it, widened to what the computed yardsticks allow where they allow more --
    # bf16 storage by itself moves the output by d_store (the emulating oracle against the plain one, both fp64), and the product may sit
    # 2.5 d_max from the emulation, so |got - plain| <= d_store + 2.5 d_max (triangle inequality).  The default network stores 36 tensors
    # in bf16 (C5's network 21); the L2 distance keeps the fixed 3e-2.
    bound = max(3e-2, d_store + 2.5 * d_max)
    report("%s: vs bf16-emulating oracle max-norm %.2e L2 %.2e (emulation fp32-vs-fp64: %.2e / %.2e); vs fp64 oracle max-norm %.2e L2 %.2e "
           "(bf16 storage in exact arithmetic: %.2e; max-norm bound %.2e set by %s)"
           % (label, e_max, e_l2, d_max, d_l2, e_plain, e_plain_l2, d_store, bound, "the fixed 3e-2" if bound == 3e-2 else "d_store + 2.5 d_max"))
    assert e_max <= 2.5 * d_max and e_l2 <= 2.5 * d_l2
    assert e_plain < bound
    assert e_plain_l2 < 3e-2


def test_reference_default_generator_bf16_inference(rt):
    """make_upscaler_orig((96, 128, 3)) with no other arguments: kernel_size 5, x4, 16 residual blocks"""
    from upscaler import model as PM
    G = PM.make_upscaler_orig((96, 128, 3))
    assert G.blocks[0][0].k == 5 and G.upscale_times == 2 and len(G.blocks) == 16
    wd = _randomize_bn(G, 3)
    x = (np.random.RandomState(1).randint(0, 256, (2, 24, 32, 3)) / 127.5 - 1).astype(np.float32)
    _check_generator(G, wd, x, 16, 4, "bf16 inference, reference default (k5 x4 16 blocks) n=2 24x32")


@pytest.mark.parametrize("k,f", [(3, 4), (5, 2), (5, 4)])
def test_bf16_generator_topologies(rt, k, f):
    from upscaler import model as PM
    h, w, res = 24, 40, 2
    G = PM.make_upscaler_orig((f * h, f * w, 3), kernel_size=k, upscale_factor=f, res_block_num=res, seed=7)
    wd = _randomize_bn(G, 5)
    x = (np.random.RandomState(2).randint(0, 256, (2, h, w, 3)) / 127.5 - 1).astype(np.float32)
    _check_generator(G, wd, x, res, f, "bf16 inference k=%d x%d res=%d n=2 %dx%d" % (k, f, res, h, w))


def test_bf16_generator_instance_norm_k5_x4(rt):
    from oracle import models as M
    from upscaler import model as PM
    n, h, w, res = 2, 24, 40, 2
    G = PM.make_upscaler_orig((4 * h, 4 * w, 3), kernel_size=5, upscale_factor=4, res_block_num=res, norm="instance", seed=7)
    wd = _randomize_bn(G, 3)
    x = (np.random.RandomState(1).randint(0, 256, (n, h, w, 3)) / 127.5 - 1).astype(np.float32)
    with torch.no_grad():
        ref, _ = M.upscaler_orig_forward(M.to_torch(wd, torch.float64), torch.tensor(x, dtype=torch.float64), False, res, 4, norm="instance")
    got = G.to_inference_bf16().predict(x)
    e = rel_err(got, ref.numpy())
    report("bf16 generator (instance norm) k5 x4 res=%d n=%d %dx%d  err=%.2e" % (res, n, h, w, e))
    assert e < 3e-2


def test_bf16_generator_refuses_unserved_topologies(rt):
    """filters != 64 and non-RGB frames stay on model.predict: the engine raises NotImplementedError and says what it serves"""
    from upscaler import model as PM
    G = PM.make_upscaler_orig((48, 64, 3), kernel_size=5, filters=32, upscale_factor=2, res_block_num=1, seed=7)
    with pytest.raises(NotImplementedError, match="filters=64"):
        G.to_inference_bf16()
    G = PM.make_upscaler_orig((48, 64, 1), kernel_size=5, upscale_factor=2, res_block_num=1, seed=7)
    with pytest.raises(NotImplementedError, match="RGB"):
        G.to_inference_bf16()


# ---- 5. frame independence and the 4 GiB edge -------------------------------------------------------------------------------------
def test_reference_default_1080p_batch4_frames_independent(rt):
    """270x480 -> 1080x1920, batch 4: upscaling/1's output is 4.25 GB (the tail runs in frame chunks below 4 GiB)"""
    from upscaler import model as PM
    G = PM.make_upscaler_orig((1080, 1920, 3))
    _randomize_bn(G, 3)
    x = (np.random.RandomState(4).randint(0, 256, (4, 270, 480, 3)) / 127.5 - 1).astype(np.float32)
    inf = G.to_inference_bf16()
    y = inf.predict(x, batch_size=4)
    for i in range(4):
        y1 = inf.predict(x[i:i + 1], batch_size=1)
        assert np.array_equal(y[i:i + 1], y1), i
    y32 = G.predict(x[:1], batch_size=1)
    e = float(np.abs(y[:1] - y32).max() / np.abs(y32).max())
    e_l2 = float(np.linalg.norm((y[:1] - y32).astype(np.float64)) / np.linalg.norm(y32.astype(np.float64)))
    report("reference default 1080p batch 4 bf16: frame 0 vs fp32 product max-norm err=%.2e  L2 err=%.2e" % (e, e_l2))
    assert e_l2 < 3e-2


def test_reference_default_batch32_repeated_frames_identical(rt):
    from upscaler import model as PM
    G = PM.make_upscaler_orig((512, 512, 3))
    _randomize_bn(G, 3)
    x4 = (np.random.RandomState(6).randint(0, 256, (4, 128, 128, 3)) / 127.5 - 1).astype(np.float32)
    x = np.concatenate([x4] * 8, 0)
    y = G.to_inference_bf16().predict(x, batch_size=32)
    assert y.shape == (32, 512, 512, 3) and np.isfinite(y).all()
    for rep in range(1, 8):
        assert np.array_equal(y[:4], y[4 * rep:4 * rep + 4]), rep

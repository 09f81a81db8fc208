"""bf16 inference of the attention generator (make_upscaler_attention, upscaling/upscaler/model.py:299-328: train_gan3.py's default -gm): the
three kernels this topology adds -- the input-driven sigmoid gate (vcg_conv_in_gate_bf16_fwd), final/conv on 128 channels
(vcg_conv9x9_to3_bf16_fwd with cin 128) and to_add_input (vcg_input_convt_add_bf16) --, the stride-2 transposed convolutions at the
channel counts it uses, and Bf16AttentionGenerator end to end.

Kernel bounds as in test_infer_x4_bf16_gpu.py: fp64 oracle on the SAME bf16-rounded operands, max-norm relative error < 2^-8 and the ulp-scaled
element-wise check < 1, outputs pre-filled with NaN.  End-to-end bounds are _check_generator's of that file: the bf16-emulating oracle
(tests/_attention_bf16_emulation.py) within 2.5x the emulation's own fp32-vs-fp64 distance (computed here), the plain fp64 oracle within
max(3e-2, d_store + 2.5 d_max) and 3e-2 in L2, a second predict bit-identical."""
import ctypes

import numpy as np
import pytest
import torch

from _attention_bf16_emulation import attention_forward_emulated
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
    """non-trivial BatchNormalization statistics / affine parameters / PReLU slopes, as after training (test_infer_x4_bf16_gpu.py)"""
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


# ---- 1. the gate ---------------------------------------------------------------------------------------------------------------------
GATE_SHAPES = [(1, 1, 1), (2, 5, 7), (1, 13, 45), (2, 25, 70)]          # the output tile is 12 x 32: the last two cross it both ways, ragged


def _run_gate(rt, n, h, w, cin, k, cout, ones):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    g = torch.Generator().manual_seed(n * 100000 + h * 1000 + w * 10 + cin + k + cout)
    u = torch.rand(n, cin, h, w, generator=g) * 2 - 1
    # pre-sigmoid values spanning about +-6: the convolution's standard deviation is s sqrt(k k cin / 3) for u uniform in [-1, 1]
    wk = torch.randn(k, k, cin, cout, generator=g) * (2.5 / (k * k * cin / 3.0) ** 0.5)
    bias = torch.rand(cout, generator=g) * 2 - 1
    m = torch.ones(n, cout, h, w) if ones else torch.randn(n, cout, h, w, generator=g)
    ud, wd, bd = u.to(rt.device), wk.to(rt.device), bias.to(rt.device)
    md = _to_nhwc_bf16(rt, m.to(rt.device))
    nbytes = rt.lib.vcg_conv_in_gate_bf16_wfrag_bytes(cin, k, k, cout)
    assert nbytes == (cout // 64) * (cin // 3) * k * ((k + 3) // 4) * 2048
    wf = torch.empty(nbytes, dtype=torch.uint8, device=rt.device)
    L.check(rt.lib.vcg_pack_conv_in_gate_bf16(wd.data_ptr(), cin, k, k, cout, wf.data_ptr(), rt.stream), "vcg_pack_conv_in_gate_bf16")
    y = torch.full((n, h, w, cout), float("nan"), dtype=torch.bfloat16, device=rt.device)
    m_before = md.clone()
    d = L.ConvDesc(n, cin, h, w, cout, h, w, k, k, 1, k // 2, k // 2)
    L.check(rt.lib.vcg_conv_in_gate_bf16_fwd(ctypes.byref(d), ud.data_ptr(), wf.data_ptr(), bd.data_ptr(), md.data_ptr(), y.data_ptr(), rt.stream),
            "vcg_conv_in_gate_bf16_fwd")
    assert torch.equal(md.view(torch.int16), m_before.view(torch.int16))
    a = K.conv2d(_bf16_round(u), _bf16_round(wk), bias.double(), 1, "same")
    if ones:                # an upper bound of every partial sum of the pre-activation: sum |u| |w| + |bias|
        return _nchw(y), a, K.conv2d(_bf16_round(u).abs(), _bf16_round(wk).abs(), bias.double().abs(), 1, "same")
    return _nchw(y), a, _bf16_round(m)


@pytest.mark.parametrize("n,h,w", GATE_SHAPES)
@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("cin", [3, 6])
def test_conv_in_gate_bf16(rt, n, h, w, cin, k, cout):
    got, a, m = _run_gate(rt, n, h, w, cin, k, cout, ones=False)
    ref = torch.sigmoid(a) * m
    e, ew = rel_err(got, ref), _ulp_scaled(got, ref)
    report("bf16 in-gate cin=%d k=%d cout=%d n=%d %dx%d  pre-sigmoid range [%.1f, %.1f]  err=%.2e  elementwise(ulp-scaled)=%.2f"
           % (cin, k, cout, n, h, w, float(a.min()), float(a.max()), e, ew))
    assert e < TOL_BF16 and ew < 1.0


def test_conv_in_gate_bf16_sigmoid_alone(rt):
    """m == 1 pins the sigmoid.  Bound per element: 2^-8 s + s (1 - s) da + 3e-7:
      * one rounding of s to bf16 -- 8 significant bits, half an ulp is at most 2^-8 s;
      * 3e-7: the absolute error of the v_exp_f32 / v_rcp_f32 sigmoid (bf16_conv3x3_3ch.hip, fast_sigmoid);
      * da: the fp32 accumulation of the pre-activation a, moved through the sigmoid's slope s (1 - s).  The kernel adds 2 sources x 5 rows x
        8 columns x 4 channels = 320 products (zero-weight slots included) and the bias, each addition rounding a partial sum that
        sum |u| |w| + |bias| =: A bounds, so da <= 321 * 2^-24 * A, with A computed here from the operands."""
    got, a, absum = _run_gate(rt, 2, 25, 70, 6, 5, 128, ones=True)
    s = torch.sigmoid(a)
    assert float(a.min()) < -5 and float(a.max()) > 5
    da = 321 * 2.0 ** -24 * absum
    excess = float(((got - s).abs() - (2.0 ** -8 * s + s * (1 - s) * da + 3e-7)).max())
    report("bf16 in-gate, m = 1: max |y - sigmoid| = %.3e, max da = %.2e, worst excess over 2^-8 s + s(1-s) da + 3e-7: %.3e"
           % (float((got - s).abs().max()), float(da.max()), excess))
    assert excess <= 0.0


# ---- 2. final/conv on 128 (and, through the new pack entry, 256) channels -------------------------------------------------------------
F9_SHAPES = [(1, 1, 1), (1, 9, 70), (2, 40, 130), (1, 140, 66)]         # work item: a 64-column strip x a 32..128-row segment


@pytest.mark.parametrize("n,h,w", F9_SHAPES)
@pytest.mark.parametrize("tanh", [1, 0])
@pytest.mark.parametrize("cin", [128, 256])
def test_conv9x9_to3_bf16(rt, cin, tanh, n, h, w):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    g = torch.Generator().manual_seed(cin * 1000 + h * 10 + w + tanh)
    x = torch.randn(n, cin, h, w, generator=g)
    wk = torch.randn(9, 9, cin, 3, generator=g) * (1.0 / (9 * cin ** 0.5))
    bias = torch.randn(3, generator=g) * 0.3
    xd, wd, bd = _to_nhwc_bf16(rt, x.to(rt.device)), wk.to(rt.device), bias.to(rt.device)
    nbytes = rt.lib.vcg_conv9x9_to3_bf16_wfrag_bytes(cin)
    assert nbytes == ((cin // 64) * 2304 + 4) * 16
    wf = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=rt.device)
    L.check(rt.lib.vcg_pack_conv9x9_to3_bf16(wd.data_ptr(), cin, wf.data_ptr(), rt.stream), "vcg_pack_conv9x9_to3_bf16")
    y = torch.full((n, 3, h, w), float("nan"), dtype=torch.float32, device=rt.device)
    d = L.ConvDesc(n, cin, h, w, 3, h, w, 9, 9, 1, 4, 4)
    L.check(rt.lib.vcg_conv9x9_to3_bf16_fwd(ctypes.byref(d), xd.data_ptr(), wf.data_ptr(), bd.data_ptr(), tanh, y.data_ptr(), rt.stream),
            "vcg_conv9x9_to3_bf16_fwd")
    if cin == 256:          # the new pack entry and the existing one: the same bytes, the same output
        assert nbytes == L.FINAL9X9_WFRAG_BYTES
        wf0 = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=rt.device)
        L.check(rt.lib.vcg_pack_final9x9_bf16(wd.data_ptr(), wf0.data_ptr(), rt.stream), "vcg_pack_final9x9_bf16")
        assert torch.equal(wf, wf0)
        y0 = torch.full((n, 3, h, w), float("nan"), dtype=torch.float32, device=rt.device)
        L.check(rt.lib.vcg_conv9x9_to3_bf16_fwd(ctypes.byref(d), xd.data_ptr(), wf0.data_ptr(), bd.data_ptr(), tanh, y0.data_ptr(), rt.stream),
                "vcg_conv9x9_to3_bf16_fwd")
        assert torch.equal(y.view(torch.int32), y0.view(torch.int32))
    got = y.cpu().double()
    ref = K.conv2d(_bf16_round(x), _bf16_round(wk), bias.double(), 1, "same")
    if tanh:
        ref = torch.tanh(ref)
    e, ew = rel_err(got, ref), _ulp_scaled(got, ref)
    report("bf16 conv9x9 %d->3 n=%d %dx%d tanh=%d  err=%.2e  elementwise(ulp-scaled)=%.2f" % (cin, n, h, w, tanh, e, ew))
    assert e < TOL_BF16 and ew < 1.0


# ---- 3. to_add_input ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 5, 7), (1, 13, 45)])
@pytest.mark.parametrize("s", [2, 4])
def test_input_convt_add_bf16(rt, s, n, h, w):
    """y = bf16(y + bias + ConvT_{k=s+1, strides s, 'same'}(atanh(0.99999 x))) in place; x holds exact +-1 pixels.
    Reference: K.conv2d_transpose_same(atanh(0.99999 x), ...) in fp64 added to the bf16 y.  Bound per element: one bf16 rounding of the sum,
    2^-8 |ref|, plus what the operands' number format costs before that rounding: the kernel evaluates atanh((double)0.99999f * x) as
    vcg_atanh_scale does and keeps the result in fp32.  |0.99999f - 0.99999| = 1.34e-8 and atanh' = 1 / (1 - 0.99999^2) = 5.0e4 at |x| = 1
    move t by at most 6.7e-4 there; the fp32 copy of t (|t| <= 6.11) by 2^-24 * 6.11 = 3.7e-7; the fp32 sum of at most 12 products by
    12 * 2^-24 of their magnitude.  So the allowance is dt * sum|w| over the at most 12 weights that reach an output, with dt = 6.8e-4."""
    from oracle import keras_ops as K
    from upscaler import _lib as L
    cout, k = 128, s + 1
    g = torch.Generator().manual_seed(s * 10000 + h * 100 + w)
    x = (torch.randint(0, 256, (n, 3, h, w), generator=g).float() / 127.5 - 1)
    flat = x.view(-1)
    flat[::5] = 1.0
    flat[2::7] = -1.0
    wk = torch.randn(k, k, cout, 3, generator=g) * 0.1                  # Keras Conv2DTranspose (kh,kw,out,in)
    bias = torch.randn(cout, generator=g) * 0.3
    y0 = torch.randn(n, cout, s * h, s * w, generator=g)
    yd = _to_nhwc_bf16(rt, y0.to(rt.device))
    xd, wd, bd = x.to(rt.device), wk.to(rt.device), bias.to(rt.device)
    x_before = xd.clone()
    d = L.ConvDesc(n, 3, h, w, cout, s * h, s * w, k, k, s, 0, 0)
    L.check(rt.lib.vcg_input_convt_add_bf16(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(), rt.stream),
            "vcg_input_convt_add_bf16")
    assert torch.equal(xd, x_before)
    got = _nchw(yd)
    t = K.conv2d_transpose_same(torch.atanh(0.99999 * x.double()), wk.double(), bias.double(), s)
    ref = _bf16_round(y0) + t
    # sum of |w| over the taps that can reach one output: at most 2 x 2 input pixels x 3 channels
    wsum = K.conv2d_transpose_same(torch.ones(n, 3, h, w, dtype=torch.float64), wk.double().abs(), None, s)
    excess = float(((got - ref).abs() - (2.0 ** -8 * ref.abs() + 6.8e-4 * wsum)).max())
    report("bf16 to_add_input s=%d n=%d %dx%d  max |y - ref| = %.3e  worst excess over one bf16 rounding + fp32 operand allowance: %.3e"
           % (s, n, h, w, float((got - ref).abs().max()), excess))
    assert excess <= 0.0


# ---- 4. the stride-2 transposed convolutions at this topology's channel counts (existing entry point) ------------------------------------
@pytest.mark.parametrize("k,cin,n,h,w,lrelu", [(5, 64, 2, 12, 32, True), (5, 128, 1, 13, 45, True), (3, 64, 1, 13, 45, True), (3, 128, 2, 9, 17, False),
                                               (5, 128, 1, 1, 1, True)])
def test_conv_transpose_s2_to128_bf16(rt, k, cin, n, h, w, lrelu):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    cout = 128
    g = torch.Generator().manual_seed(k * 100000 + cin * 100 + h * 10 + w)
    x = torch.randn(n, cin, h, w, generator=g)
    wk = torch.randn(k, k, cout, cin, generator=g) * (0.5 / (k * (cin ** 0.5)))
    bias = torch.randn(cout, generator=g) * 0.3
    xd = _to_nhwc_bf16(rt, x.to(rt.device))
    wd, bd = wk.to(rt.device), bias.to(rt.device)
    crop = (k - 2) // 2
    d = L.ConvDesc(n, cin, h, w, cout, 2 * h, 2 * w, k, k, 2, crop, crop)
    wfr = torch.empty(k * k * cout * cin, dtype=torch.bfloat16, device=rt.device)
    L.check(rt.lib.vcg_pack_conv_frag_bf16(wd.data_ptr(), k * k, cout, cin, 1, wfr.data_ptr(), rt.stream), "pack frag")
    y = torch.full((n, 2 * h, 2 * w, cout), float("nan"), dtype=torch.bfloat16, device=rt.device)
    L.check(rt.lib.vcg_conv_transpose2d_nhwc_bf16_fwd(ctypes.byref(d), xd.data_ptr(), wfr.data_ptr(), bd.data_ptr(), L.ACT_LRELU if lrelu else L.ACT_NONE,
                                                      0.2, y.data_ptr(), rt.stream), "vcg_conv_transpose2d_nhwc_bf16_fwd")
    got = _nchw(y)
    ref = K.conv2d_transpose_same(_bf16_round(x), _bf16_round(wk), bias.double(), 2)
    if lrelu:
        ref = torch.where(ref >= 0, ref, 0.2 * ref)
    e, ew = rel_err(got, ref), _ulp_scaled(got, ref)
    report("bf16 convT%dx%d s2 %d->%d (generic) n=%d %dx%d lrelu=%s  err=%.2e  elementwise(ulp-scaled)=%.2f" % (k, k, cin, cout, n, h, w, lrelu, e, ew))
    assert e < TOL_BF16 and ew < 1.0


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
def _emulation_bounds(wd, x, res, f):
    """the bf16-emulating oracle in fp64 (the reference output of a bf16 engine) and its own fp32-vs-fp64 distance (the yardstick)"""
    from oracle import models as M
    with torch.no_grad():
        y64 = attention_forward_emulated(M.to_torch(wd, torch.float64), torch.tensor(x, dtype=torch.float64), res, f)
        y32 = attention_forward_emulated(M.to_torch(wd, torch.float32), torch.tensor(x, dtype=torch.float32), res, f)
        yp, _ = M.upscaler_attention_forward(M.to_torch(wd, torch.float64), torch.tensor(x, dtype=torch.float64), False, res, f)
    y64, y32, yp = y64.numpy(), y32.double().numpy(), yp.numpy()
    return y64, yp, rel_err(y32, y64), float(np.linalg.norm(y32 - y64) / np.linalg.norm(y64))


def _check_generator(G, wd, x, res, f, label):
    """test_infer_x4_bf16_gpu.py's _check_generator, on the attention emulation"""
    inf = G.to_inference_bf16()
    got = inf.predict(x)
    got2 = inf.predict(x)                                   # second call: pure graph replay
    assert got.shape == (x.shape[0], x.shape[1] * f, x.shape[2] * f, 3)
    assert np.array_equal(got, got2)
    y64, yp, d_max, d_l2 = _emulation_bounds(wd, x, res, f)
    g = got.astype(np.float64)
    e_max, e_l2 = rel_err(g, y64), float(np.linalg.norm(g - y64) / np.linalg.norm(y64))
    e_plain, e_plain_l2 = rel_err(g, yp), float(np.linalg.norm(g - yp) / np.linalg.norm(yp))
    d_store = rel_err(y64, yp)
    bound = max(3e-2, d_store + 2.5 * d_max)
    report("%s: vs bf16-emulating oracle max-norm %.2e L2 %.2e (emulation fp32-vs-fp64: %.2e / %.2e); vs fp64 oracle max-norm %.2e L2 %.2e "
           "(bf16 storage in exact arithmetic: %.2e; max-norm bound %.2e)" % (label, e_max, e_l2, d_max, d_l2, e_plain, e_plain_l2, d_store, bound))
    assert e_max <= 2.5 * d_max and e_l2 <= 2.5 * d_l2
    assert e_plain < bound
    assert e_plain_l2 < 3e-2


def test_attention_default_generator_bf16_inference(rt):
    """make_upscaler_attention((96, 128, 3)) with no other arguments: kernel_size 5, x4, 16 residual blocks"""
    from upscaler import model as PM
    G = PM.make_upscaler_attention((96, 128, 3))
    assert G.attention_generator == {"kernel_size": 5, "filters": 64, "upscale_factor": 4, "res_block_num": 16, "norm": "batch", "channels": 3}
    wd = _randomize_bn(G, 3)
    x = (np.random.RandomState(1).randint(0, 256, (2, 24, 32, 3)) / 127.5 - 1).astype(np.float32)
    _check_generator(G, wd, x, 16, 4, "bf16 inference, attention default (k5 x4 16 blocks) n=2 24x32")


@pytest.mark.parametrize("k,f", [(3, 2), (3, 4), (5, 2)])
def test_attention_generator_topologies(rt, k, f):
    from upscaler import model as PM
    h, w, res = 24, 40, 2
    G = PM.make_upscaler_attention((f * h, f * w, 3), kernel_size=k, upscale_factor=f, res_block_num=res, seed=7)
    wd = _randomize_bn(G, 5)
    x = (np.random.RandomState(2).randint(0, 256, (2, h, w, 3)) / 127.5 - 1).astype(np.float32)
    _check_generator(G, wd, x, res, f, "bf16 attention inference k=%d x%d res=%d n=2 %dx%d" % (k, f, res, h, w))


def test_attention_generator_frames_independent(rt):
    """batch 3 equals three single-frame calls bit for bit"""
    from upscaler import model as PM
    G = PM.make_upscaler_attention((96, 160, 3), res_block_num=2)
    _randomize_bn(G, 3)
    x = (np.random.RandomState(4).randint(0, 256, (3, 24, 40, 3)) / 127.5 - 1).astype(np.float32)
    inf = G.to_inference_bf16()
    y = inf.predict(x, batch_size=3)
    for i in range(3):
        assert np.array_equal(y[i:i + 1], inf.predict(x[i:i + 1], batch_size=1)), i
    # the same batch with the tail forced into frame chunks of 2 + 1 (what the 4 GiB rule does to large batches of large frames)
    chunked = G.to_inference_bf16()
    chunked._tail_chunk = lambda n, h, w: min(n, 2)
    assert np.array_equal(chunked.predict(x, batch_size=3), y)


def test_attention_1080p_batch8_at_the_4gib_edge(rt):
    """270x480 -> 1080x1920, 2 blocks, batch 8: upscaling/1's output is 4.25e9 bytes, the largest batch of these frames below the 4 GiB
    (4.29e9) of one launch -- the rule's edge: one more frame and the tail runs as 5 + 4"""
    from upscaler import model as PM
    G = PM.make_upscaler_attention((1080, 1920, 3), res_block_num=2)
    _randomize_bn(G, 3)
    x = (np.random.RandomState(4).randint(0, 256, (8, 270, 480, 3)) / 127.5 - 1).astype(np.float32)
    inf = G.to_inference_bf16()
    assert 0.98 * 2 ** 32 < 8 * 1080 * 1920 * 128 * 2 < 2 ** 32 and inf._tail_chunk(8, 270, 480) == 8 and inf._tail_chunk(9, 270, 480) == 5
    y = inf.predict(x, batch_size=8)
    for i in range(8):
        assert np.array_equal(y[i:i + 1], inf.predict(x[i:i + 1], batch_size=1)), i
    y32 = G.predict(x[:1], batch_size=1)
    e_l2 = float(np.linalg.norm((y[:1] - y32).astype(np.float64)) / np.linalg.norm(y32.astype(np.float64)))
    report("attention 1080p batch 8 bf16: frame 0 vs fp32 product L2 err=%.2e" % e_l2)
    assert e_l2 < 3e-2


def test_attention_generator_refuses_unserved_topologies(rt):
    from upscaler import model as PM
    for kw, pat in (({"filters": 32}, "filters=64"), ({"norm": "instance"}, "norm='batch'"), ({"upscale_factor": 8}, "upscale_factor 2 or 4")):
        f = kw.get("upscale_factor", 2)
        G = PM.make_upscaler_attention((24 * f, 32 * f, 3), **dict({"kernel_size": 3, "upscale_factor": f, "res_block_num": 1}, **kw))
        with pytest.raises(NotImplementedError, match=pat):
            G.to_inference_bf16()
    G = PM.make_upscaler_attention((48, 64, 1), kernel_size=3, upscale_factor=2, res_block_num=1)
    with pytest.raises(NotImplementedError, match="RGB"):
        G.to_inference_bf16()
    assert not hasattr(PM.make_upscaler_orig_functional((48, 64, 3), kernel_size=3, upscale_factor=2, res_block_num=1), "attention_generator")

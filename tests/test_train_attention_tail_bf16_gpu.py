"""bf16 tail TRAINING of make_upscaler_attention (tail_dtype='bf16'): the entry points behind after_res/add through the C ABI --
(1) vcg_conv_in_gate_up_bf16_bwd, (2) vcg_conv_in_gate_up_bf16_wgrad, (3) vcg_conv9x9_c128to3_bf16_wgrad and the 128-channel data gradient,
(4) vcg_input_convt_add_bf16_to, (5) vcg_input_convt_add_bf16_bwd, (6) the Conv2DTranspose gradients at 64 -> 128 and 128 -> 128 -- the layer
classes built on them against the fp32 graph's nodes, and the model against the storage-emulating fp64 oracle
(tests/_attention_bf16_tail_train_emulation.py)."""
import ctypes

import numpy as np
import pytest
import torch

from _attention_bf16_tail_train_emulation import CASES, FLOOR, N, H, W, RES, allowed_zero_gradients, l2, training_case
from conftest import rel_err, report
from test_infer_attention_bf16_gpu import GATE_SHAPES, TOL_BF16, _ulp_scaled

pytestmark = pytest.mark.gpu


def _r(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _nhwc_bf16(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def _nchw_f64(y_nhwc_bf16):
    return y_nhwc_bf16.cpu().double().permute(0, 3, 1, 2)


def _bits(t):
    return t.view(torch.int16)


def _nan(rt, *shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=rt.device)


# ---------------------------------------------------------------------------------------------------------------
# (1) vcg_conv_in_gate_up_bf16_bwd
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", GATE_SHAPES)
@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("k", [3, 5])
def test_conv_in_gate_up_bf16_bwd(rt, n, h, w, k, cout):
    """test_conv_in_gate_bf16_bwd at cin 6 and cout 64 / 128: dm = bf16(dy s + dres), da = bf16(dy m s (1 - s)) against the fp64 formula on
    the same bf16-rounded operands, max-norm < 2^-8 and ulp-scaled < 1, with and without dres; NULL dres = a dres of zeros; a second call
    is bit-identical.  The kernel scale (that test's 2.5 over sqrt 2, for twice the input channels) keeps the pre-sigmoid values within about +-12."""
    from oracle import keras_ops as K
    from upscaler import _engine as E, _lib as L
    g = torch.Generator().manual_seed(n * 100000 + h * 1000 + w * 10 + k + cout)
    u = torch.rand(n, 6, h, w, generator=g) * 2 - 1
    wk = torch.randn(k, k, 6, cout, generator=g) * (1.8 / (k * k) ** 0.5)
    bias = torch.rand(cout, generator=g) * 2 - 1
    m, dy, dres = (torch.randn(n, cout, h, w, generator=g) for _ in range(3))
    ud, bd = u.to(rt.device), bias.to(rt.device)
    wf = E.pack_conv_in_gate_bf16(rt, wk.to(rt.device), 6, k, k, cout)
    md, dyd, drd = (_nhwc_bf16(t).to(rt.device) for t in (m, dy, dres))
    d = L.ConvDesc(n, 6, h, w, cout, h, w, k, k, 1, k // 2, k // 2)

    def run(res):
        dm, da = _nan(rt, n, h, w, cout, dtype=torch.bfloat16), _nan(rt, n, h, w, cout, dtype=torch.bfloat16)
        L.check(rt.lib.vcg_conv_in_gate_up_bf16_bwd(ctypes.byref(d), ud.data_ptr(), wf.data_ptr(), bd.data_ptr(), md.data_ptr(), dyd.data_ptr(),
                                                    None if res is None else res.data_ptr(), dm.data_ptr(), da.data_ptr(), rt.stream),
                "vcg_conv_in_gate_up_bf16_bwd")
        torch.cuda.synchronize()
        return dm, da
    before = [t.clone() for t in (md, dyd, drd)]
    dm1, da1 = run(drd)
    dm2, da2 = run(drd)
    dm0, da0 = run(None)
    dmz, daz = run(torch.zeros_like(drd))
    for t, b in zip((md, dyd, drd), before):
        assert torch.equal(_bits(t), _bits(b))
    a = K.conv2d(_r(u), _r(wk), bias.double(), 1, "same")
    s = torch.sigmoid(a)
    ref_da = _r(dy) * _r(m) * s * (1 - s)
    line = "bf16 up-gate bwd k=%d cout=%d n=%d %dx%d  pre-sigmoid range [%.1f, %.1f]" % (k, cout, n, h, w, float(a.min()), float(a.max()))
    for name, got, ref in (("dm+dres", dm1, _r(dy) * s + _r(dres)), ("dm", dm0, _r(dy) * s), ("da", da1, ref_da), ("da(no dres)", da0, ref_da)):
        assert not bool(torch.isnan(got.float()).any()), name
        e, ew = rel_err(_nchw_f64(got), ref), _ulp_scaled(_nchw_f64(got), ref)
        line += "  %s err=%.2e ulp-scaled=%.2f" % (name, e, ew)
        assert e < TOL_BF16 and ew < 1.0, (name, e, ew)
    report(line)
    assert torch.equal(_bits(dm1), _bits(dm2)) and torch.equal(_bits(da1), _bits(da2))
    assert torch.equal(_bits(dm0), _bits(dmz)) and torch.equal(_bits(da0), _bits(daz)) and torch.equal(_bits(da0), _bits(da1))


# ---------------------------------------------------------------------------------------------------------------
# (2) vcg_conv_in_gate_up_bf16_wgrad
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(2, 9, 20), (1, 37, 70)])
@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("k", [3, 5])
def test_conv_in_gate_up_bf16_wgrad(rt, n, h, w, k, cout):
    """dW (k,k,6,cout) and dbias from fp32 NCHW u and bf16 NHWC da against fp64 autograd on the bf16-rounded operands, to 1e-4 max-norm
    (test_conv3ch_bf16_wgrad_k5's rule); a second call over another workspace fill is bit-identical"""
    from oracle import keras_ops as K
    from upscaler import _lib as L
    g = torch.Generator().manual_seed(7 * h + w + k + cout)
    u, da = torch.rand(n, 6, h, w, generator=g) * 2 - 1, torch.randn(n, cout, h, w, generator=g)
    wr = torch.zeros(k, k, 6, cout, dtype=torch.float64, requires_grad=True)
    br = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    gw, gb = torch.autograd.grad((K.conv2d(_r(u), wr, br, 1, "same") * _r(da)).sum(), [wr, br])
    d = L.ConvDesc(n, 6, h, w, cout, h, w, k, k, 1, k // 2, k // 2)
    need = rt.lib.vcg_conv_in_gate_up_bf16_wgrad_ws_bytes(ctypes.byref(d))
    assert need > 0
    ud, dad = u.to(rt.device), _nhwc_bf16(da).to(rt.device)
    out = []
    for fill in (0xFF, 0x3F):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=rt.device)
        dw, db = _nan(rt, k, k, 6, cout), _nan(rt, cout)
        L.check(rt.lib.vcg_conv_in_gate_up_bf16_wgrad(ctypes.byref(d), ud.data_ptr(), dad.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), need,
                                                      rt.stream), "vcg_conv_in_gate_up_bf16_wgrad")
        torch.cuda.synchronize()
        out.append((dw, db))
    e_w, e_b = rel_err(out[0][0], gw), rel_err(out[0][1], gb)
    report("up-gate wgrad k=%d cout=%d n=%d %dx%d: dw=%.2e db=%.2e (workspace %d bytes)" % (k, cout, n, h, w, e_w, e_b, need))
    assert not bool(torch.isnan(out[0][0]).any()) and not bool(torch.isnan(out[0][1]).any())
    assert e_w < 1e-4 and e_b < 1e-4
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---------------------------------------------------------------------------------------------------------------
# (3) final/conv at 128 channels
# ---------------------------------------------------------------------------------------------------------------
_f9_cache = {}


def _f9_data(n, h, w):
    if (n, h, w) not in _f9_cache:
        from oracle import keras_ops as K
        g = torch.Generator().manual_seed(9 * h + w)
        x = torch.randn(n, 128, h, w, generator=g)
        wk = torch.randn(9, 9, 128, 3, generator=g) * 0.01
        dy = torch.randn(n, 3, h, w, generator=g)
        xr = _r(x).requires_grad_(True)
        wr = torch.zeros(9, 9, 128, 3, dtype=torch.float64, requires_grad=True)
        (gx,) = torch.autograd.grad((K.conv2d(xr, _r(wk), None, 1, "same") * _r(dy)).sum(), [xr])
        (gw,) = torch.autograd.grad((K.conv2d(_r(x), wr, None, 1, "same") * _r(dy)).sum(), [wr])
        _f9_cache[(n, h, w)] = dict(x=x, wk=wk, dy=dy, gx=gx, gw=gw)
    return _f9_cache[(n, h, w)]


@pytest.mark.parametrize("n,h,w", [(2, 9, 20), (1, 37, 70)])
def test_final_conv_c128_wgrad(rt, n, h, w):
    """dW (9,9,128,3) from bf16 NHWC x and fp32 NCHW dz against fp64 autograd on the bf16-rounded operands to 1e-5 max-norm (the rule
    tests/test_abi_memory_contract_gpu.py applies to the 256 form); deterministic"""
    from upscaler import _lib as L
    D = _f9_data(n, h, w)
    d = L.ConvDesc(n, 128, h, w, 3, h, w, 9, 9, 1, 4, 4)
    need = rt.lib.vcg_conv9x9_c128to3_bf16_wgrad_ws_bytes(ctypes.byref(d))
    assert need > 0
    xd, dzd = _nhwc_bf16(D["x"]).to(rt.device), D["dy"].to(rt.device)
    out = []
    for fill in (0xFF, 0x3F):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=rt.device)
        dw = _nan(rt, 9, 9, 128, 3)
        L.check(rt.lib.vcg_conv9x9_c128to3_bf16_wgrad(ctypes.byref(d), xd.data_ptr(), dzd.data_ptr(), dw.data_ptr(), ws.data_ptr(), need, rt.stream),
                "vcg_conv9x9_c128to3_bf16_wgrad")
        torch.cuda.synchronize()
        out.append(dw)
    e = rel_err(out[0], D["gw"])
    report("final/conv wgrad cin 128 n=%d %dx%d: dw=%.2e (workspace %d bytes)" % (n, h, w, e, need))
    assert not bool(torch.isnan(out[0]).any()) and e < 1e-5
    assert torch.equal(out[0], out[1])


@pytest.mark.parametrize("n,h,w", [(2, 9, 20), (1, 37, 70)])
def test_final_conv_c128_dgrad(rt, n, h, w):
    """vcg_conv9x9_to3_bf16_dgrad at cin 128 with y_prev NULL -- documented for 64 * {1,2,4,8}, run by no test before -- to the rule that file
    applies to the 256 form's bf16 output: 2^-8 max-norm and ulp-scaled < 1"""
    from upscaler import _lib as L
    D = _f9_data(n, h, w)
    d = L.ConvDesc(n, 128, h, w, 3, h, w, 9, 9, 1, 4, 4)
    wd = torch.empty(2 * L.FIRST9X9_WFRAG_BYTES, dtype=torch.uint8, device=rt.device)
    L.check(rt.lib.vcg_pack_conv9x9_3ch_bf16(D["wk"].to(rt.device).data_ptr(), 128, 1, wd.data_ptr(), rt.stream), "vcg_pack_conv9x9_3ch_bf16")
    dyd = D["dy"].to(rt.device)
    dx = _nan(rt, n, h, w, 128, dtype=torch.bfloat16)
    L.check(rt.lib.vcg_conv9x9_to3_bf16_dgrad(ctypes.byref(d), dyd.data_ptr(), wd.data_ptr(), None, 0.0, dx.data_ptr(), rt.stream),
            "vcg_conv9x9_to3_bf16_dgrad")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dx.float()).any())
    e, ew = rel_err(_nchw_f64(dx), D["gx"]), _ulp_scaled(_nchw_f64(dx), D["gx"])
    report("final/conv dgrad cin 128 n=%d %dx%d: err=%.2e ulp-scaled=%.2f" % (n, h, w, e, ew))
    assert e < TOL_BF16 and ew < 1.0


# ---------------------------------------------------------------------------------------------------------------
# (4) vcg_input_convt_add_bf16_to and (5) vcg_input_convt_add_bf16_bwd
# ---------------------------------------------------------------------------------------------------------------
ADD_INPUT_SHAPES = [(2, 5, 7), (1, 9, 12)]          # no multiple of the 4 x 8 tile; the last row / column meets the dropped tap


def _add_input_desc(L, n, h, w, s, cout):
    return L.ConvDesc(n, 3, h, w, cout, s * h, s * w, s + 1, s + 1, s, 0, 0)


@pytest.mark.parametrize("n,h,w", ADD_INPUT_SHAPES)
@pytest.mark.parametrize("s", [2, 4])
def test_input_convt_add_bf16_to(rt, n, h, w, s):
    """y_out has the bits the in-place entry leaves in a copy of y_in; y_in keeps its own"""
    from upscaler import _lib as L
    cout = 128
    g = torch.Generator().manual_seed(1000 * s + 10 * h + w)
    x = (torch.rand(n, 3, h, w, generator=g) * 2 - 1).to(rt.device)
    wk = (torch.randn(s + 1, s + 1, cout, 3, generator=g) * 0.2).to(rt.device)
    bias = torch.randn(cout, generator=g).to(rt.device)
    yin = torch.randn(n, s * h, s * w, cout, generator=g).to(torch.bfloat16).to(rt.device)
    keep, inplace = yin.clone(), yin.clone()
    yout = _nan(rt, *yin.shape, dtype=torch.bfloat16)
    d = _add_input_desc(L, n, h, w, s, cout)
    L.check(rt.lib.vcg_input_convt_add_bf16(ctypes.byref(d), x.data_ptr(), wk.data_ptr(), bias.data_ptr(), inplace.data_ptr(), rt.stream),
            "vcg_input_convt_add_bf16")
    L.check(rt.lib.vcg_input_convt_add_bf16_to(ctypes.byref(d), x.data_ptr(), wk.data_ptr(), bias.data_ptr(), yin.data_ptr(), yout.data_ptr(), rt.stream),
            "vcg_input_convt_add_bf16_to")
    torch.cuda.synchronize()
    assert torch.equal(_bits(yin), _bits(keep))
    assert torch.equal(_bits(yout), _bits(inplace)) and not torch.equal(_bits(yout), _bits(keep))


@pytest.mark.parametrize("n,h,w", ADD_INPUT_SHAPES)
@pytest.mark.parametrize("s", [2, 4])
def test_input_convt_add_bf16_bwd(rt, n, h, w, s):
    """dz bit-equal to vcg_lrelu_bwd_bf16 on the same operands; dbias_convt (sum of the stored dz), dbias_to_add (sum of dY) and dw within
    1e-4 max-norm of fp64 on the same operands -- dw against autograd of K.conv2d_transpose_same on a = fp32(atanh(0.99999f x)) --; a
    second call over another workspace fill is bit-identical"""
    from oracle import keras_ops as K
    from upscaler import _lib as L
    cout, slope = 128, 0.2
    g = torch.Generator().manual_seed(77 * s + 10 * h + w)
    x = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    x[0, :, 0, 0] = torch.tensor([1.0, -1.0, 0.0])                    # the ends of the range: atanh's steepest points
    dY = torch.randn(n, s * h, s * w, cout, generator=g).to(torch.bfloat16)
    yact = torch.randn(n, s * h, s * w, cout, generator=g).to(torch.bfloat16)
    xd, dYd, yd = x.to(rt.device), dY.to(rt.device), yact.to(rt.device)
    d = _add_input_desc(L, n, h, w, s, cout)
    need = rt.lib.vcg_input_convt_add_bf16_bwd_ws_bytes(ctypes.byref(d))
    assert need > 0
    out = []
    for fill in (0xFF, 0x3F):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=rt.device)
        dz = _nan(rt, *dY.shape, dtype=torch.bfloat16)
        dw, dba, dbc = _nan(rt, s + 1, s + 1, cout, 3), _nan(rt, cout), _nan(rt, cout)
        L.check(rt.lib.vcg_input_convt_add_bf16_bwd(ctypes.byref(d), xd.data_ptr(), dYd.data_ptr(), yd.data_ptr(), slope, dz.data_ptr(), dw.data_ptr(),
                                                    dba.data_ptr(), dbc.data_ptr(), ws.data_ptr(), need, rt.stream), "vcg_input_convt_add_bf16_bwd")
        torch.cuda.synchronize()
        out.append((dz, dw, dba, dbc))
    dz, dw, dba, dbc = out[0]
    ref_dz = torch.empty_like(dz)
    L.check(rt.lib.vcg_lrelu_bwd_bf16(dYd.data_ptr(), yd.data_ptr(), slope, ref_dz.data_ptr(), dz.numel(), rt.stream), "vcg_lrelu_bwd_bf16")
    torch.cuda.synchronize()
    assert torch.equal(_bits(dz), _bits(ref_dz))
    a = torch.atanh(np.float32(0.99999).item() * x.double()).float().double()      # evaluated in double, used as fp32
    wr = torch.zeros(s + 1, s + 1, cout, 3, dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad((K.conv2d_transpose_same(a, wr, None, s) * dY.double().permute(0, 3, 1, 2)).sum(), [wr])
    e_w = rel_err(dw, gw)
    e_a = rel_err(dba, dY.double().sum((0, 1, 2)))
    e_c = rel_err(dbc, dz.cpu().double().sum((0, 1, 2)))
    report("add_input bwd s=%d n=%d %dx%d: dw=%.2e dbias_to_add=%.2e dbias_convt=%.2e (workspace %d bytes)" % (s, n, h, w, e_w, e_a, e_c, need))
    for t in (dw, dba, dbc):
        assert not bool(torch.isnan(t).any())
    assert e_w < 1e-4 and e_a < 1e-4 and e_c < 1e-4
    for a_, b_ in zip(out[0], out[1]):
        assert torch.equal(a_.view(torch.int16) if a_.dtype == torch.bfloat16 else a_, b_.view(torch.int16) if b_.dtype == torch.bfloat16 else b_)


# ---------------------------------------------------------------------------------------------------------------
# (6) the Conv2DTranspose gradients at the tail's shapes, on entries that served them untested
# ---------------------------------------------------------------------------------------------------------------
_ct_cache = {}


def _ct_data(cin, k, n=2, h=6, w=10, cout=128):
    if (cin, k) not in _ct_cache:
        from oracle import keras_ops as K
        g = torch.Generator().manual_seed(13 * cin + k)
        x = torch.randn(n, cin, h, w, generator=g)
        wk = torch.randn(k, k, cout, cin, generator=g) * (0.5 / (k * cin ** 0.5))
        dz = torch.randn(n, cout, 2 * h, 2 * w, generator=g)
        xr, wr = _r(x).requires_grad_(True), _r(wk).requires_grad_(True)
        gx, gw = torch.autograd.grad((K.conv2d_transpose_same(xr, wr, None, 2) * _r(dz)).sum(), [xr, wr])
        _ct_cache[(cin, k)] = dict(x=x, wk=wk, dz=dz, gx=gx, gw=gw, n=n, h=h, w=w, cout=cout)
    return _ct_cache[(cin, k)]


@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("k", [3, 5])
def test_conv_transpose_tail_shapes_wgrad(rt, cin, k):
    """vcg_conv_transpose2d_nhwc_bf16_wgrad at 64 -> 128 and 128 -> 128, 3x3 and 5x5, 6x10 input at batch 2: 1e-4 max-norm against fp64
    autograd of K.conv2d_transpose_same on the bf16-rounded operands"""
    from upscaler import _lib as L
    D = _ct_data(cin, k)
    n, h, w, cout, crop = D["n"], D["h"], D["w"], D["cout"], max(k - 2, 0) // 2
    d = L.ConvDesc(n, cin, h, w, cout, 2 * h, 2 * w, k, k, 2, crop, crop)
    need = rt.lib.vcg_conv_transpose2d_nhwc_bf16_wgrad_workspace_bytes(ctypes.byref(d))
    assert need > 0
    xd, dzd = _nhwc_bf16(D["x"]).to(rt.device), _nhwc_bf16(D["dz"]).to(rt.device)
    ws = torch.empty(need, dtype=torch.uint8, device=rt.device)
    dw = _nan(rt, k, k, cout, cin)
    L.check(rt.lib.vcg_conv_transpose2d_nhwc_bf16_wgrad(ctypes.byref(d), xd.data_ptr(), dzd.data_ptr(), dw.data_ptr(), ws.data_ptr(), need, rt.stream),
            "vcg_conv_transpose2d_nhwc_bf16_wgrad")
    torch.cuda.synchronize()
    e = rel_err(dw, D["gw"])
    report("convT wgrad %d->%d k%d n=%d %dx%d: dw=%.2e" % (cin, cout, k, n, h, w, e))
    assert not bool(torch.isnan(dw).any()) and e < 1e-4


@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("k", [3, 5])
def test_conv_transpose_tail_shapes_dgrad(rt, cin, k):
    """the data gradient as E.ConvTBf16.backward runs it -- the stride-2 vcg_conv2d_nhwc_bf16_fwd over dz, 128 -> 64 and 128 -> 128 -- against
    the same fp64 reference.  The result is STORED in bf16, whose rounding alone is up to 2^-9 of an element: the bound is the project's
    for bf16-stored tensors (2^-8 max-norm, ulp-scaled < 1), as for the final convolution's data gradient above; the 1e-4 rule is the
    one for fp32 weight gradients and is applied to them in the test above."""
    from upscaler import _engine as E, _lib as L
    D = _ct_data(cin, k)
    n, h, w, cout, crop = D["n"], D["h"], D["w"], D["cout"], max(k - 2, 0) // 2
    wg = E.pack_conv_frag_bf16(rt, D["wk"].to(rt.device), k * k, cin, cout, 0)
    dd = L.ConvDesc(n, cout, 2 * h, 2 * w, cin, h, w, k, k, 2, crop, crop)
    dzd = _nhwc_bf16(D["dz"]).to(rt.device)
    dx = _nan(rt, n, h, w, cin, dtype=torch.bfloat16)
    L.check(rt.lib.vcg_conv2d_nhwc_bf16_fwd(ctypes.byref(dd), dzd.data_ptr(), wg.data_ptr(), None, L.ACT_NONE, 0.0, dx.data_ptr(), rt.stream),
            "vcg_conv2d_nhwc_bf16_fwd")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dx.float()).any())
    e, ew = rel_err(_nchw_f64(dx), D["gx"]), _ulp_scaled(_nchw_f64(dx), D["gx"])
    report("convT dgrad %d<-%d k%d n=%d %dx%d: err=%.2e ulp-scaled=%.2f" % (cin, cout, k, n, h, w, e, ew))
    assert e < TOL_BF16 and ew < 1.0


# ---------------------------------------------------------------------------------------------------------------
# (7) the layer classes against the fp32 graph's nodes on the same weights
# ---------------------------------------------------------------------------------------------------------------
def _bind(rt, layer, weights):
    from upscaler import _engine as E
    ps = E.ParamStore()
    layer.declare(ps)
    ps.materialize(rt)
    layer.bind(rt, ps)
    ps.set_weights({k: v.numpy() for k, v in weights.items()})
    return ps


def _rb(t):
    return t.to(torch.bfloat16).float()


@pytest.mark.parametrize("k,cout,n,h,w", [(3, 128, 2, 9, 20), (5, 64, 1, 13, 21)])          # w = 21: the weight gradient's fp32 fallback at odd widths
def test_up_gate_conv_bf16_layer_matches_the_fp32_nodes(rt, k, cout, n, h, w):
    """test_gate_conv_bf16_layer_matches_the_fp32_nodes for E.UpGateConvBf16: bf16-representable u, kernel, m, dy and dres on both paths;
    y and dm (with the joining gradient) to 2^-8 max-norm and ulp-scaled < 1 against the fp32 Conv2D + sigmoid gate nodes; per element of
    dW and dbias the difference is at most 2^-9 sum |da| |u| (half a bf16 ulp of every da, the sum evaluated by the fp32 kernel on the
    absolute values) plus 1e-5 of that sum for the fp32 summation"""
    from upscaler import _engine as E, _lib as L
    g = torch.Generator().manual_seed(100 * k + w + cout)
    u = _rb(torch.rand(n, 6, h, w, generator=g) * 2 - 1)
    wk = _rb(torch.randn(k, k, 6, cout, generator=g) * (1.8 / (k * k) ** 0.5))
    bias = torch.rand(cout, generator=g) * 2 - 1
    m, dy, dres = (_rb(torch.randn(n, cout, h, w, generator=g)) for _ in range(3))
    gate, conv = E.UpGateConvBf16("g", 6, cout, k), E.Conv2D("g", 6, cout, k)
    ps_b, ps_f = _bind(rt, gate, {"g/kernel": wk, "g/bias": bias}), _bind(rt, conv, {"g/kernel": wk, "g/bias": bias})
    ud, md, dyd, drd = (t.to(rt.device) for t in (u, m, dy, dres))
    a, cctx = conv.forward(ud)
    y32, da32, dm32 = rt.empty(*md.shape), rt.empty(*md.shape), rt.empty(*md.shape)
    L.check(rt.lib.vcg_sigmoid_gate_fwd(a.data_ptr(), md.data_ptr(), y32.data_ptr(), md.numel(), rt.stream), "vcg_sigmoid_gate_fwd")
    L.check(rt.lib.vcg_sigmoid_gate_bwd(a.data_ptr(), md.data_ptr(), dyd.data_ptr(), da32.data_ptr(), dm32.data_ptr(), md.numel(), rt.stream),
            "vcg_sigmoid_gate_bwd")
    conv.backward(cctx, da32, False, True, 0)
    conv.backward((ud.abs(), None, cctx[2]), da32.abs(), False, True, 1)          # slot 1: sum |da| |u| and sum |da|
    mb = _nhwc_bf16(m).to(rt.device)
    y, ctx = gate.forward(ud, mb)
    dm = gate.backward(ctx, _nhwc_bf16(dy).to(rt.device), 0, dx_residual=_nhwc_bf16(dres).to(rt.device))
    torch.cuda.synchronize()
    line = "UpGateConvBf16 k=%d cout=%d n=%d %dx%d vs fp32 nodes:" % (k, cout, n, h, w)
    for name, got, ref in (("y", y, y32), ("dm", dm, dm32 + drd)):
        e, ew = rel_err(_nchw_f64(got), ref.cpu().double()), _ulp_scaled(_nchw_f64(got), ref.cpu().double())
        line += " %s err=%.2e ulp-scaled=%.2f" % (name, e, ew)
        assert e < TOL_BF16 and ew < 1.0, (name, e, ew)
    for name in ("g/kernel", "g/bias"):
        got, ref, bound = (p.grad(name, s).cpu().double() for p, s in ((ps_b, 0), (ps_f, 0), (ps_f, 1)))
        excess = float(((got - ref).abs() - (2.0 ** -9 + 1e-5) * bound).max())
        line += " d%s max-norm=%.2e worst excess over the bound=%.2e" % (name[2:], rel_err(got, ref), excess)
        assert excess <= 0.0, (name, excess)
    report(line)


@pytest.mark.parametrize("k,cin,s,n,h,w", [(3, 64, 2, 2, 6, 10), (5, 128, 4, 1, 10, 14)])
def test_up_block_bf16_layers_match_the_fp32_nodes(rt, k, cin, s, n, h, w):
    """E.UpConvTBf16 + E.ToAddInputBf16 against the fp32 graph's ConvT2D(+LeakyReLU), atanh, to_add_input transposed convolution and Add
    on the same weights; the frames are h*2/s x w*2/s so both branches meet at 2h x 2w.  Operands (x, the ConvT kernel, dY) are
    bf16-representable.  Stored in bf16: y_act, y, dz, dx -- 2^-8 max-norm and ulp-scaled < 1 against fp32, where y = bf16(y_act + to_add)
    is compared with the stored y_act plus fp32's to_add (one rounding; against fp32's own sum, which does not round y_act, two half
    ulps of the larger of the two: 2^-8 max|.|) and dz through the mask the bf16 path itself used (a y_act within rounding of 0 may fall
    on either side).  The ConvT kernel gradient reads dz
    rounded to bf16 where fp32 reads it exactly: per element at most 2^-9 sum |dz| |x| (the sum in fp64 on the CPU) plus 1e-5 of it; its
    bias gradient is the sum of the stored dz (1e-5 of sum |dz|, plus the rounding 2^-9 sum |dz| against fp32's); to_add_input's kernel
    and bias gradients read the same dY on both paths: 1e-4 max-norm, the rule of fp32 weight gradients."""
    from oracle import keras_ops as K
    from upscaler import _engine as E, _lib as L
    g = torch.Generator().manual_seed(31 * k + cin + s)
    fh, fw = 2 * h // s, 2 * w // s
    x = _rb(torch.randn(n, cin, h, w, generator=g))
    frames = torch.rand(n, 3, fh, fw, generator=g) * 2 - 1
    wt = _rb(torch.randn(k, k, 128, cin, generator=g) * (0.5 / (k * cin ** 0.5)))
    bt = torch.randn(128, generator=g) * 0.3
    wa = torch.randn(s + 1, s + 1, 128, 3, generator=g) * 0.2
    ba = torch.randn(128, generator=g) * 0.3
    dY = _rb(torch.randn(n, 128, 2 * h, 2 * w, generator=g))
    W = {"t/kernel": wt, "t/bias": bt}
    WA = {"a/kernel": wa, "a/bias": ba}
    # fp32 nodes
    ct32 = E.ConvT2D("t", cin, 128, k, L.ACT_LRELU, 0.2)
    ta32 = E.ConvT2D("a", 3, 128, 3) if s == 2 else E.ConvTDilated("a", 3, 128, 5, 4)
    ps_t32, ps_a32 = _bind(rt, ct32, W), _bind(rt, ta32, WA)
    xd, fd, dYd = x.to(rt.device), frames.to(rt.device), dY.to(rt.device)
    yact32, c32 = ct32.forward(xd)
    at = rt.empty(*fd.shape)
    L.check(rt.lib.vcg_atanh_scale(fd.data_ptr(), at.data_ptr(), fd.numel(), 0.99999, rt.stream), "vcg_atanh_scale")
    t32, ca32 = ta32.forward(at)
    y32 = yact32 + t32
    dx32 = ct32.backward(c32, dYd, True, True, 0)
    ta32.backward(ca32, dYd, False, True, 0)
    # bf16 layers
    ct, ta = E.UpConvTBf16("t", cin, 128, k, L.ACT_LRELU, 0.2), E.ToAddInputBf16("a", 3, 128, s, 0.2)
    ps_t, ps_a = _bind(rt, ct, W), _bind(rt, ta, WA)
    yact, cctx = ct.forward(_nhwc_bf16(x).to(rt.device))
    keep = yact.clone()
    y, actx = ta.forward(fd, yact, True)
    y0, _ = ta.forward(fd, yact.clone(), False)                       # learning phase 0: in place, the same bits
    dz, sums = ta.backward(actx, _nhwc_bf16(dY).to(rt.device), 0)
    dx = ct.backward(cctx, dz, True, True, 0, dz_channel_sums=sums)
    torch.cuda.synchronize()
    assert torch.equal(_bits(yact), _bits(keep)) and torch.equal(_bits(y), _bits(y0))
    mask = _nchw_f64(yact) > 0
    dz_ref = torch.where(mask, dY.double(), 0.2 * dY.double())
    line = "UpConvTBf16 + ToAddInputBf16 k=%d cin=%d s=%d n=%d %dx%d vs fp32 nodes:" % (k, cin, s, n, h, w)
    # dx against fp32 is compared where the two masks agree everywhere; otherwise against fp64 on the bf16 path's own dz
    wr = wt.double().requires_grad_(True)
    xr = x.double().requires_grad_(True)
    gx, gw = torch.autograd.grad((K.conv2d_transpose_same(xr, wr, None, 2) * _nchw_f64(dz)).sum(), [xr, wr])
    (bound_w,) = torch.autograd.grad((K.conv2d_transpose_same(x.double().abs(), wr, None, 2) * dz_ref.abs()).sum(), [wr])
    # y = bf16(y_act + to_add) is ONE rounding of the stored y_act plus fp32's to_add; against fp32's own sum it carries y_act's rounding too
    y_ref = _nchw_f64(yact) + t32.cpu().double()
    assert float((_nchw_f64(y) - y32.cpu().double()).abs().max()) <= 2.0 ** -8 * float(torch.maximum(y32.abs().max(), yact32.abs().max()))
    for name, got, ref in (("y_act", yact, yact32.cpu().double()), ("y", y, y_ref), ("dz", dz, dz_ref), ("dx", dx, gx)):
        e, ew = rel_err(_nchw_f64(got), ref), _ulp_scaled(_nchw_f64(got), ref)
        line += " %s err=%.2e ulp-scaled=%.2f" % (name, e, ew)
        assert e < TOL_BF16 and ew < 1.0, (name, e, ew)
    flips = int((mask != (yact32.cpu() > 0)).sum())
    got_w, ref_w = ps_t.grad("t/kernel", 0).cpu().double(), ps_t32.grad("t/kernel", 0).cpu().double()
    if flips == 0:
        excess = float(((got_w - ref_w).abs() - (2.0 ** -9 + 1e-5) * bound_w).max())
        line += " dkernel vs fp32 max-norm=%.2e worst excess=%.2e" % (rel_err(got_w, ref_w), excess)
        assert excess <= 0.0, excess
        assert float((dx32.cpu().double() - _nchw_f64(dx)).abs().max()) <= 2.0 ** -7 * float(gx.abs().max())
    e_w = rel_err(got_w, gw)                                          # fp64 on the operands the bf16 kernels read
    e_b = rel_err(ps_t.grad("t/bias", 0), _nchw_f64(dz).sum((0, 2, 3)))
    e_aw, e_ab = rel_err(ps_a.grad("a/kernel", 0), ps_a32.grad("a/kernel", 0)), rel_err(ps_a.grad("a/bias", 0), ps_a32.grad("a/bias", 0))
    line += " mask flips=%d dkernel=%.2e dbias=%.2e to_add dkernel=%.2e dbias=%.2e" % (flips, e_w, e_b, e_aw, e_ab)
    report(line)
    assert e_w < 1e-4 and e_b < 1e-4 and e_aw < 1e-4 and e_ab < 1e-4


@pytest.mark.parametrize("n,h,w", [(2, 9, 20), (1, 13, 21)])          # w = 21: the weight gradient's fp32 fallback at odd widths
def test_final_conv_c128_layer_matches_the_fp32_node(rt, n, h, w):
    """E.FinalConv9x9C128Bf16 against the fp32 Conv2D(3, 9, tanh) node on a bf16-representable input and kernel: output 1e-4 max-norm (fp32
    both, fast tanh: the bound tests/test_abi_memory_contract_gpu.py gives the 256 form's forward), bias gradient 1e-4, data gradient
    2^-8 max-norm / ulp-scaled < 1 (stored bf16) against fp64 on the bf16-rounded dz the kernel multiplies, kernel gradient within 2^-9 sum |dz| |x| + 1e-5 of it per element (dz enters as a bf16
    operand; the sum from the fp32 kernel on the absolute values)"""
    from oracle import keras_ops as K
    from upscaler import _engine as E, _lib as L
    g = torch.Generator().manual_seed(17 * h + w)
    x = _rb(torch.randn(n, 128, h, w, generator=g))
    wk = _rb(torch.randn(9, 9, 128, 3, generator=g) * 0.01)
    bias = torch.randn(3, generator=g) * 0.1
    dy = torch.randn(n, 3, h, w, generator=g)
    W = {"f/kernel": wk, "f/bias": bias}
    c32, cb = E.Conv2D("f", 128, 3, 9, act=L.ACT_TANH), E.FinalConv9x9C128Bf16("f", 128, 3, 9)
    ps32, psb = _bind(rt, c32, W), _bind(rt, cb, W)
    xd, dyd = x.to(rt.device), dy.to(rt.device)
    y32, ctx32 = c32.forward(xd)
    dx32 = c32.backward(ctx32, dyd, True, True, 0)
    dz32 = dyd * (1 - y32 * y32)
    c32_lin = E.Conv2D("f", 128, 3, 9)
    c32_lin.bind(rt, ps32)
    c32_lin.backward((xd.abs(), None, ctx32[2]), dz32.abs(), False, True, 1)          # slot 1: sum |dz| |x|
    y, ctx = cb.forward(_nhwc_bf16(x).to(rt.device))
    dx = cb.backward(ctx, dyd, True, True, 0)
    torch.cuda.synchronize()
    e_y, e_b = rel_err(y, y32), rel_err(psb.grad("f/bias", 0), ps32.grad("f/bias", 0))
    # the data gradient multiplies dz ROUNDED to bf16 (its MFMA operand) where the fp32 node multiplies dz itself: the one-rounding bound holds
    # against fp64 on that operand; against the fp32 node the operand roundings add up to another rounding's worth (2^-7 max-norm in all)
    xr = x.double().requires_grad_(True)
    (gx,) = torch.autograd.grad((K.conv2d(xr, wk.double(), None, 1, "same") * _r(dz32.cpu())).sum(), [xr])
    e_x, ew_x = rel_err(_nchw_f64(dx), gx), _ulp_scaled(_nchw_f64(dx), gx)
    assert rel_err(_nchw_f64(dx), dx32.cpu().double()) < 2.0 ** -7
    got, ref, bound = psb.grad("f/kernel", 0).cpu().double(), ps32.grad("f/kernel", 0).cpu().double(), ps32.grad("f/kernel", 1).cpu().double()
    excess = float(((got - ref).abs() - (2.0 ** -9 + 1e-5) * bound).max())
    report("FinalConv9x9C128Bf16 n=%d %dx%d vs fp32 node: y=%.2e dbias=%.2e dx err=%.2e ulp-scaled=%.2f dkernel max-norm=%.2e worst excess=%.2e"
           % (n, h, w, e_y, e_b, e_x, ew_x, rel_err(got, ref), excess))
    assert e_y < 1e-4 and e_b < 1e-4 and e_x < TOL_BF16 and ew_x < 1.0 and excess <= 0.0


# ---------------------------------------------------------------------------------------------------------------
# (8) the model
# ---------------------------------------------------------------------------------------------------------------


def _model(k, f, **kw):
    from upscaler import model as PM
    return PM.make_upscaler_attention((f * H, f * W, 3), kernel_size=k, upscale_factor=f, res_block_num=RES, seed=7, **kw)


BF = dict(trunk_dtype="bf16", tail_dtype="bf16")


@pytest.mark.parametrize("k,f", CASES)
def test_attention_tail_bf16_training_forward_and_gradients(rt, k, f):
    """The rule of test_attention_bf16_training_forward_and_gradients unchanged, against the emulation that also rounds the tail: per tensor
    relative L2 below max(1e-2, 2.5 x that tensor's fp32-vs-fp64 distance under the same emulation), output below max(1e-3, 2.5 x its
    own), loss 1e-4, moving statistics 1e-4; only allowed zero gradients are excluded; no device masks go to the oracle."""
    from upscaler import model as PM, _engine as E
    c = training_case(k, f)
    G = _model(k, f, **BF)
    assert (G.trunk_dtype, G.tail_dtype) == ("bf16", "bf16")
    G.set_weights_dict(c["weights"])
    r64, r32 = c["f64"], c["f32"]
    y, tape = G.forward(E.to_device_nchw(rt, c["x"]), True)
    assert tuple(y.shape) == (N, 3, f * H, f * W) and y.dtype == torch.float32
    val, dy = PM._pixel_loss(rt, y, E.to_device_nchw(rt, c["t"]), "mse", 1.0)
    G.backward(tape, dy, 0)
    e_y, e32_y = l2(E.to_nhwc(rt, y).cpu().double(), r64["y"]), l2(r32["y"], r64["y"])
    e_loss = abs(float(val.item()) - r64["loss"]) / r64["loss"]
    gmax = max(float(g.abs().max()) for g in r64["grads"].values())
    excluded, failed = [], []
    for kk, b in r64["grads"].items():
        a = G.ps.grad(kk).cpu().double()
        floor = FLOOR * gmax * b.numel() ** 0.5
        real = float(b.norm()) >= floor
        e, e32 = l2(a, b, floor), l2(r32["grads"][kk], b, floor)
        report("    attention bf16 tail k%d x%d %-50s |g|2=%.2e rel L2 err=%.2e (oracle fp32-vs-fp64, same storage: %.2e)%s"
               % (k, f, kk, float(b.norm()), e, e32, "" if real else "   [zero gradient: excluded]"))
        if not real:
            excluded.append(kk)
        elif not e < max(1e-2, 2.5 * e32):
            failed.append((kk, e, e32))
    report("attention bf16 tail training pass k%d x%d vs oracle with the same storage: output err (rel L2)=%.2e (oracle fp32-vs-fp64 %.2e) loss err=%.1e excluded=%s"
           % (k, f, e_y, e32_y, e_loss, excluded))
    assert not failed, failed
    assert set(excluded) <= allowed_zero_gradients(), sorted(set(excluded) - allowed_zero_gradients())
    assert e_y < max(1e-3, 2.5 * e32_y) and e_loss < 1e-4, (e_y, e32_y, e_loss)
    sw = G.get_weights_dict()
    assert len(r64["upd"]) == 2 * (2 * RES + 1)
    for kk, v in r64["upd"].items():
        assert np.max(np.abs(sw[kk] - v)) < 1e-4 * (np.max(np.abs(v)) + 1e-3), kk


def test_attention_tail_bf16_gradients_reach_both_slots(rt):
    from upscaler import model as PM, _engine as E
    k, f = CASES[1]
    c = training_case(k, f)
    G = _model(k, f, **BF)
    got = []
    for which in (0, 1):
        G.set_weights_dict(c["weights"])
        y, tape = G.forward(E.to_device_nchw(rt, c["x"]), True)
        _, dy = PM._pixel_loss(rt, y, E.to_device_nchw(rt, c["t"]), "mse", 1.0)
        G.backward(tape, dy, which)
        got.append({kk: G.ps.grad(kk, which).clone() for kk in c["f64"]["grads"]})
    for kk in got[0]:
        assert torch.equal(got[0][kk], got[1][kk]), kk


@pytest.mark.parametrize("k,f", CASES)
def test_attention_tail_bf16_learning_phase_0(rt, k, f):
    """predict against the emulation in inference mode: the trunk file's rule -- 3e-2 in relative L2, or 2.5 x the emulation's own
    fp32-vs-fp64 distance where that is larger; a second predict is bit-identical; the moving statistics do not move"""
    c = training_case(k, f)
    G = _model(k, f, **BF)
    G.set_weights_dict(c["weights"])
    got = G.predict(c["x"])
    e, e32 = l2(torch.tensor(got).double(), c["f64"]["y0"]), l2(c["f32"]["y0"], c["f64"]["y0"])
    report("attention bf16 tail k%d x%d learning phase 0 vs emulation: rel L2 %.2e (oracle fp32-vs-fp64 %.2e)" % (k, f, e, e32))
    assert got.shape == (N, f * H, f * W, 3) and e < max(3e-2, 2.5 * e32)
    assert np.array_equal(got, G.predict(c["x"]))
    assert G.get_weights_dict()["after_res/batch_norm/moving_mean"].tolist() == c["weights"]["after_res/batch_norm/moving_mean"].tolist()


def test_attention_tail_bf16_names_weights_and_inference_engine(rt, tmp_path):
    """weight names and order are the fp32 model's, and so are the initial weights; set / get and a checkpoint round trip keep every
    array; to_inference_bf16() computes the bits it computes from the fp32 model with the same weights"""
    k, f = CASES[1]
    c = training_case(k, f)
    Gb, Gf = _model(k, f, **BF), _model(k, f)
    assert Gb.attention_generator == Gf.attention_generator and (Gf.trunk_dtype, Gf.tail_dtype) == ("fp32", "fp32")
    assert list(Gb.get_weights_dict()) == list(Gf.get_weights_dict())
    for kk, v in Gf.get_weights_dict().items():
        assert np.array_equal(v, Gb.get_weights_dict()[kk]), kk
    kinds = {kind for kind, _, _, _ in Gb.graph.nodes}
    assert "to_f32" not in kinds and "add_input" in kinds and not kinds & {"gate", "atanh"}
    for i in range({2: 1, 4: 2}[f]):
        assert {"upscaling/%d/block/%s" % (i, s) for s in ("attention_multiply", "to_add_input_atanh", "add_input")} <= Gb.graph.names
    Gb.set_weights_dict(c["weights"])
    Gf.set_weights_dict(c["weights"])
    for kk, v in Gb.get_weights_dict().items():
        assert np.array_equal(v, c["weights"][kk]), kk
    path = str(tmp_path / "g.safetensors")
    Gb.save(path)
    G2 = _model(k, f, **BF)
    G2.load_weights(path)
    for kk, v in G2.get_weights_dict().items():
        assert np.array_equal(v, c["weights"][kk]), kk
    assert np.array_equal(G2.predict(c["x"]), Gb.predict(c["x"]))
    assert np.array_equal(Gb.to_inference_bf16().predict(c["x"]), Gf.to_inference_bf16().predict(c["x"]))


def test_attention_tail_fp32_keyword_builds_the_bf16_trunk_model(rt):
    """tail_dtype='fp32' is today's trunk_dtype='bf16' model: the same node list and a bit-equal forward"""
    k, f = CASES[0]
    c = training_case(k, f)
    Ga, Gb = _model(k, f, trunk_dtype="bf16"), _model(k, f, trunk_dtype="bf16", tail_dtype="fp32")
    sig = lambda G: [(kind, type(layer).__name__, ins) for kind, layer, ins, _ in G.graph.nodes]
    assert sig(Ga) == sig(Gb) and (Ga.tail_dtype, Gb.tail_dtype) == ("fp32", "fp32")
    Ga.set_weights_dict(c["weights"])
    Gb.set_weights_dict(c["weights"])
    assert np.array_equal(Ga.predict(c["x"]), Gb.predict(c["x"]))


def test_attention_tail_bf16_train_step_graph_replay_matches_eager(rt):
    """the bf16-tail generator with the bf16 PatchGAN inside make_and_compile_gan2, 32x32 -> 64x64 frames, batch 2: two recorded steps
    reproduce two eagerly launched ones bit for bit (weights and the four losses); every value is finite"""
    from upscaler import model as PM, _engine as E
    h, bs = 32, 2

    def run(graph):
        G = PM.make_upscaler_attention((2 * h, 2 * h, 3), kernel_size=3, upscale_factor=2, res_block_num=2, **BF)
        D = PM.make_discriminator_patchgan_70((2 * h, 2 * h, 3), seed=11, dtype="bf16")
        _, _, gan = PM.make_and_compile_gan2(G, D, (h, h, 3), (2 * h, 2 * h, 3), "mse", 1.0, lambda: PM.WassersteinLosses(), 1e-2,
                                             optimizer=PM.Adam())
        tr = gan.trainer
        rng = np.random.RandomState(5)
        steps = [(E.to_device_nchw(rt, rng.randint(0, 256, (bs, h, h, 3)) / 127.5 - 1),
                  E.to_device_nchw(rt, rng.randint(0, 256, (bs, 2 * h, 2 * h, 3)) / 127.5 - 1)) for _ in range(3)]
        out = []
        if graph:
            tr.capture_train_step(*steps[0])
            for a, b in steps[1:]:
                out.append(tr.train_step_graph(a, b))
        else:
            for a, b in steps:
                out.append(tr.train_step(a, b))
            out = out[1:]
        return out, G.ps.params.clone(), D.ps.params.clone()
    oe, ge, de = run(False)
    og, gg, dg = run(True)
    assert len(og) == 2 and all(len(s) == 4 for s in og)
    assert oe == og, (oe, og)
    assert torch.equal(ge, gg) and torch.equal(de, dg)
    assert all(np.isfinite(v) for step in og for v in step)
    assert bool(torch.isfinite(gg).all()) and bool(torch.isfinite(dg).all())

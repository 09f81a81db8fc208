"""The memory contract of the attention generator's entry points (include/vcg.h), as tests/test_abi_memory_contract_gpu.py checks the
others: every buffer inside a guarded arena (tests/_arena.py), weight packs of EXACTLY the byte count their *_wfrag_bytes query returns;
after each call the guards are intact, the inputs hold their bytes, the outputs are fully written (their NaN prefill is gone) and match the
fp64 reference on the same bf16-rounded operands (2^-8 max-norm, ulp-scaled < 1).  None of these entry points takes a workspace.  Unsupported
descriptors return VCG_E_UNSUPPORTED and leave every output at its prefill."""
import ctypes

import pytest
import torch

import _arena as A
from conftest import rel_err, report

pytestmark = pytest.mark.gpu
OK, E_UNSUPPORTED = 0, -3
TOL_BF16 = 2.0 ** -8


def _r(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _nhwc_bf16(t):
    return t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def _ulp_scaled(got, ref):
    return float(((got - ref).abs() / (ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max())).max())


def _finish(name, arenas, inputs, got, ref):
    """guards, inputs unmodified, output fully written and within the bf16 bounds"""
    torch.cuda.current_stream().synchronize()
    for a in arenas:
        a.check()
    for a, t in inputs:
        raw = t.contiguous().view(-1).view(torch.uint8)
        assert torch.equal(a.payload.cpu(), raw), "%s modified its input %s" % (name, a.name)
    assert not torch.isnan(got).any(), "%s left %d NaN in its output" % (name, int(torch.isnan(got).sum()))
    e, ew = rel_err(got, ref), _ulp_scaled(got, ref)
    report("abi contract %-40s err=%.2e ulp-scaled=%.2f" % (name, e, ew))
    assert e < TOL_BF16 and ew < 1.0


def _pack_gate(rt, wk, cin, k, cout):
    nbytes = rt.lib.vcg_conv_in_gate_bf16_wfrag_bytes(cin, k, k, cout)
    assert nbytes > 0
    wa = A.input_arena(wk, rt.device, name="w_hwio")
    out = A.output_arena((nbytes,), torch.uint8, rt.device, name="wfrag")
    assert rt.lib.vcg_pack_conv_in_gate_bf16(wa.ptr, cin, k, k, cout, out.ptr, rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    wa.check()
    out.check()
    assert torch.equal(wa.payload.cpu(), wk.contiguous().view(-1).view(torch.uint8))
    assert not torch.isnan(out.view(torch.bfloat16).float()).any()          # every fragment written (the prefill reads as NaN)
    return out.payload.clone()


@pytest.mark.parametrize("cin,k,cout,n,h,w", [(3, 5, 64, 2, 13, 45), (6, 5, 128, 1, 25, 33), (6, 3, 64, 1, 5, 7), (3, 3, 128, 1, 1, 1)])
def test_conv_in_gate_contract(rt, cin, k, cout, n, h, w):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    g = torch.Generator().manual_seed(cin * 100 + k * 10 + cout + h)
    u = torch.rand(n, cin, h, w, generator=g) * 2 - 1
    wk = torch.randn(k, k, cin, cout, generator=g) * (2.5 / (k * k * cin / 3.0) ** 0.5)
    bias = torch.rand(cout, generator=g) * 2 - 1
    m = _nhwc_bf16(torch.randn(n, cout, h, w, generator=g))
    wf = _pack_gate(rt, wk, cin, k, cout).cpu()
    ua, fa, ba, ma = (A.input_arena(t, rt.device, name=nm) for t, nm in ((u, "u"), (wf, "wfrag"), (bias, "bias"), (m, "m")))
    ya = A.output_arena((n, h, w, cout), torch.bfloat16, rt.device, name="y")
    d = L.ConvDesc(n, cin, h, w, cout, h, w, k, k, 1, k // 2, k // 2)
    assert rt.lib.vcg_conv_in_gate_bf16_fwd(ctypes.byref(d), ua.ptr, fa.ptr, ba.ptr, ma.ptr, ya.ptr, rt.stream) == OK
    ref = torch.sigmoid(K.conv2d(_r(u), _r(wk), bias.double(), 1, "same")) * m.double().permute(0, 3, 1, 2)
    got = ya.view(torch.bfloat16, (n, h, w, cout)).cpu().double().permute(0, 3, 1, 2)
    _finish("vcg_conv_in_gate_bf16_fwd cin%d k%d cout%d" % (cin, k, cout), [ua, fa, ba, ma, ya], [(ua, u), (fa, wf), (ba, bias), (ma, m)], got, ref)


@pytest.mark.parametrize("n,h,w", [(1, 9, 70), (2, 40, 66)])
def test_conv9x9_to3_cin128_contract(rt, n, h, w):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    cin = 128
    g = torch.Generator().manual_seed(h * 10 + w)
    x = torch.randn(n, cin, h, w, generator=g)
    wk = torch.randn(9, 9, cin, 3, generator=g) * (1.0 / (9 * cin ** 0.5))
    bias = torch.randn(3, generator=g) * 0.3
    nbytes = rt.lib.vcg_conv9x9_to3_bf16_wfrag_bytes(cin)
    assert nbytes == (2 * 2304 + 4) * 16
    wa = A.input_arena(wk, rt.device, name="w")
    pk = A.output_arena((nbytes,), torch.uint8, rt.device, name="wfrag")
    assert rt.lib.vcg_pack_conv9x9_to3_bf16(wa.ptr, cin, pk.ptr, rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    wa.check()
    pk.check()
    assert not torch.isnan(pk.view(torch.bfloat16).float()).any()
    assert not pk.payload[-64:].any()                                         # the zero bytes the kernel fetches its padding pixels from
    wf, xb = pk.payload.cpu(), _nhwc_bf16(x)
    xa, fa, ba = (A.input_arena(t, rt.device, name=nm) for t, nm in ((xb, "x"), (wf, "wfrag"), (bias, "bias")))
    ya = A.output_arena((n, 3, h, w), torch.float32, rt.device, name="y")
    d = L.ConvDesc(n, cin, h, w, 3, h, w, 9, 9, 1, 4, 4)
    assert rt.lib.vcg_conv9x9_to3_bf16_fwd(ctypes.byref(d), xa.ptr, fa.ptr, ba.ptr, 1, ya.ptr, rt.stream) == OK
    ref = torch.tanh(K.conv2d(_r(x), _r(wk), bias.double(), 1, "same"))
    got = ya.view(torch.float32, (n, 3, h, w)).cpu().double()
    _finish("vcg_conv9x9_to3_bf16_fwd cin128 %dx%d" % (h, w), [xa, fa, ba, ya], [(xa, xb), (fa, wf), (ba, bias)], got, ref)


@pytest.mark.parametrize("s,n,h,w", [(2, 2, 5, 7), (4, 1, 13, 10)])
def test_input_convt_add_contract(rt, s, n, h, w):
    """y is read and written in place: its arena starts as the bf16 tensor (guards as an output arena's)"""
    from oracle import keras_ops as K
    from upscaler import _lib as L
    cout, k = 128, s + 1
    g = torch.Generator().manual_seed(s * 100 + h)
    x = torch.rand(n, 3, h, w, generator=g) * 1.9 - 0.95
    wk = torch.randn(k, k, cout, 3, generator=g) * 0.1
    bias = torch.randn(cout, generator=g) * 0.3
    y0 = _nhwc_bf16(torch.randn(n, cout, s * h, s * w, generator=g))
    xa, wa, ba = (A.input_arena(t, rt.device, name=nm) for t, nm in ((x, "x"), (wk, "w_hwoi"), (bias, "bias")))
    ya = A.output_arena((n, s * h, s * w, cout), torch.bfloat16, rt.device, name="y")
    ya.payload.copy_(y0.view(-1).view(torch.uint8))
    d = L.ConvDesc(n, 3, h, w, cout, s * h, s * w, k, k, s, 0, 0)
    assert rt.lib.vcg_input_convt_add_bf16(ctypes.byref(d), xa.ptr, wa.ptr, ba.ptr, ya.ptr, rt.stream) == OK
    ref = y0.double().permute(0, 3, 1, 2) + K.conv2d_transpose_same(torch.atanh(0.99999 * x.double()), wk.double(), bias.double(), s)
    got = ya.view(torch.bfloat16, (n, s * h, s * w, cout)).cpu().double().permute(0, 3, 1, 2)
    _finish("vcg_input_convt_add_bf16 s%d" % s, [xa, wa, ba, ya], [(xa, x), (wa, wk), (ba, bias)], got, ref)


def test_unsupported_descriptors_are_refused_before_any_launch(rt):
    from upscaler import _lib as L
    lib = rt.lib
    one = A.input_arena(torch.zeros(4096), rt.device, name="operand")
    out = A.output_arena((4096,), torch.float32, rt.device, name="out")
    # the gate: cin, kernel size, channel count, stride, pads, and y == m
    for cin, k, cout in ((4, 3, 64), (3, 7, 64), (3, 4, 64), (6, 5, 96), (3, 5, 1024), (9, 3, 64)):
        assert lib.vcg_conv_in_gate_bf16_wfrag_bytes(cin, k, k, cout) == 0
        assert lib.vcg_pack_conv_in_gate_bf16(one.ptr, cin, k, k, cout, out.ptr, rt.stream) == E_UNSUPPORTED
        d = L.ConvDesc(1, cin, 4, 4, cout, 4, 4, k, k, 1, k // 2, k // 2)
        assert lib.vcg_conv_in_gate_bf16_fwd(ctypes.byref(d), one.ptr, one.ptr, one.ptr, one.ptr, out.ptr, rt.stream) == E_UNSUPPORTED
    assert lib.vcg_conv_in_gate_bf16_wfrag_bytes(3, 5, 3, 64) == 0
    for d in (L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 3, 3, 2, 1, 1), L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 5, 5, 1, 1, 1), L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 5, 3, 1, 2, 1)):
        assert lib.vcg_conv_in_gate_bf16_fwd(ctypes.byref(d), one.ptr, one.ptr, one.ptr, one.ptr, out.ptr, rt.stream) == E_UNSUPPORTED
    d = L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 3, 3, 1, 1, 1)
    assert lib.vcg_conv_in_gate_bf16_fwd(ctypes.byref(d), one.ptr, one.ptr, one.ptr, out.ptr, out.ptr, rt.stream) == E_UNSUPPORTED      # y is m
    # final/conv: 128 and 256 input channels only
    for cin in (64, 192, 512):
        assert lib.vcg_conv9x9_to3_bf16_wfrag_bytes(cin) == 0
        assert lib.vcg_pack_conv9x9_to3_bf16(one.ptr, cin, out.ptr, rt.stream) == E_UNSUPPORTED
        d = L.ConvDesc(1, cin, 4, 4, 3, 4, 4, 9, 9, 1, 4, 4)
        assert lib.vcg_conv9x9_to3_bf16_fwd(ctypes.byref(d), one.ptr, one.ptr, one.ptr, 1, out.ptr, rt.stream) == E_UNSUPPORTED
    # to_add_input: strides 2 and 4, kernel s + 1, three input channels, weights inside the LDS
    for d in (L.ConvDesc(1, 3, 2, 2, 128, 6, 6, 4, 4, 3, 0, 0), L.ConvDesc(1, 3, 2, 2, 128, 4, 4, 5, 5, 2, 0, 0), L.ConvDesc(1, 6, 2, 2, 128, 4, 4, 3, 3, 2, 0, 0),
              L.ConvDesc(1, 3, 2, 2, 128, 4, 4, 3, 3, 2, 1, 1), L.ConvDesc(1, 3, 2, 2, 100, 4, 4, 3, 3, 2, 0, 0), L.ConvDesc(1, 3, 2, 2, 256, 8, 8, 5, 5, 4, 0, 0)):
        assert lib.vcg_input_convt_add_bf16(ctypes.byref(d), one.ptr, one.ptr, one.ptr, out.ptr, rt.stream) == E_UNSUPPORTED
    torch.cuda.current_stream().synchronize()
    one.check()
    out.check()
    assert out.untouched()

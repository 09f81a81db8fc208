"""The memory contract of the entry points the bf16 tail training of make_upscaler_attention adds (include/vcg.h), as
tests/test_abi_attention_train_contract_gpu.py checks the trunk's: every buffer inside a guarded arena (tests/_arena.py), packs, workspaces
and outputs of EXACTLY the queried byte counts; after each call the guards are intact, the inputs hold their bytes, the outputs are fully
written (their NaN prefill is gone) and match the fp64 reference on the same operands.  A workspace one byte short is refused with nothing
written; refused calls leave every output at its prefill."""
import ctypes

import pytest
import torch

import _arena as A
from conftest import rel_err, report

pytestmark = pytest.mark.gpu
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_WORKSPACE = 0, -1, -2, -3, -4
TOL_BF16 = 2.0 ** -8


def _r(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _nhwc_bf16(t):
    return t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _ulp_scaled(got, ref):
    return float(((got - ref).abs() / (ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max())).max())


def _check_inputs(name, inputs):
    for a, t in inputs:
        a.check()
        assert torch.equal(a.payload.cpu(), t.contiguous().view(-1).view(torch.uint8)), "%s modified its input %s" % (name, a.name)


@pytest.mark.parametrize("k,cout,n,h,w,with_dres", [(5, 128, 2, 13, 46, False), (3, 64, 1, 25, 34, True), (3, 128, 1, 1, 1, True)])
def test_up_gate_bwd_and_wgrad_contract(rt, k, cout, n, h, w, with_dres):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    g = torch.Generator().manual_seed(k * 1000 + h * 10 + w + cout)
    u = torch.rand(n, 6, h, w, generator=g) * 2 - 1
    wk = torch.randn(k, k, 6, cout, generator=g) * (1.8 / (k * k) ** 0.5)
    bias = torch.rand(cout, generator=g) * 2 - 1
    m, dy, dres = (_nhwc_bf16(torch.randn(n, cout, h, w, generator=g)) for _ in range(3))
    nbytes = rt.lib.vcg_conv_in_gate_bf16_wfrag_bytes(6, k, k, cout)
    assert nbytes == (cout // 64) * 2 * k * ((k + 3) // 4) * 2048
    wa = A.input_arena(wk, rt.device, name="w_hwio")
    pk = A.output_arena((nbytes,), torch.uint8, rt.device, name="wfrag")
    assert rt.lib.vcg_pack_conv_in_gate_bf16(wa.ptr, 6, k, k, cout, pk.ptr, rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    pk.check()
    wf = pk.payload.cpu()
    ua, fa, ba, ma, ya, ra = (A.input_arena(t, rt.device, name=nm) for t, nm in ((u, "u"), (wf, "wfrag"), (bias, "bias"), (m, "m"), (dy, "dy"), (dres, "dres")))
    dma, daa = (A.output_arena((n, h, w, cout), torch.bfloat16, rt.device, name=nm) for nm in ("dm", "da"))
    d = L.ConvDesc(n, 6, h, w, cout, h, w, k, k, 1, k // 2, k // 2)
    assert rt.lib.vcg_conv_in_gate_up_bf16_bwd(ctypes.byref(d), ua.ptr, fa.ptr, ba.ptr, ma.ptr, ya.ptr, ra.ptr if with_dres else None, dma.ptr, daa.ptr,
                                               rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    name = "vcg_conv_in_gate_up_bf16_bwd k%d cout%d %dx%d%s" % (k, cout, h, w, " +dres" if with_dres else "")
    _check_inputs(name, [(ua, u), (fa, wf), (ba, bias), (ma, m), (ya, dy), (ra, dres)])
    s = torch.sigmoid(K.conv2d(_r(u), _r(wk), bias.double(), 1, "same"))
    ref_dm = _nchw(dy) * s + (_nchw(dres) if with_dres else 0.0)
    ref_da = _nchw(dy) * _nchw(m) * s * (1 - s)
    for a, ref, nm in ((dma, ref_dm, "dm"), (daa, ref_da, "da")):
        a.check()
        got = _nchw(a.view(torch.bfloat16, (n, h, w, cout)).cpu())
        assert not torch.isnan(got).any(), "%s left NaN in %s" % (name, nm)
        e, ew = rel_err(got, ref), _ulp_scaled(got, ref)
        report("abi contract %-48s %s err=%.2e ulp-scaled=%.2f" % (name, nm, e, ew))
        assert e < TOL_BF16 and ew < 1.0
    # the weight gradient from the da just written
    need = rt.lib.vcg_conv_in_gate_up_bf16_wgrad_ws_bytes(ctypes.byref(d))
    if w % 2:
        assert need == 0
        return
    assert need > 0
    da = daa.view(torch.bfloat16, (n, h, w, cout)).cpu()
    za = A.input_arena(da, rt.device, name="da")
    ws = A.workspace_arena(need, rt.device)
    dwa, dba = A.output_arena((k, k, 6, cout), torch.float32, rt.device, name="dw"), A.output_arena((cout,), torch.float32, rt.device, name="db")
    assert rt.lib.vcg_conv_in_gate_up_bf16_wgrad(ctypes.byref(d), ua.ptr, za.ptr, dwa.ptr, dba.ptr, ws.ptr, need, rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    _check_inputs("vcg_conv_in_gate_up_bf16_wgrad", [(ua, u), (za, da)])
    for a in (ws, dwa, dba):
        a.check()
    wr = torch.zeros(k, k, 6, cout, dtype=torch.float64, requires_grad=True)
    br = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    gw, gb = torch.autograd.grad((K.conv2d(_r(u), wr, br, 1, "same") * _nchw(da)).sum(), [wr, br])
    dw, db = dwa.view(torch.float32, (k, k, 6, cout)).cpu(), dba.view(torch.float32).cpu()
    assert not torch.isnan(dw).any() and not torch.isnan(db).any()
    e_w, e_b = rel_err(dw, gw), rel_err(db, gb)
    report("abi contract vcg_conv_in_gate_up_bf16_wgrad k%d cout%d n=%d %dx%d: dw=%.2e db=%.2e (workspace %d bytes)" % (k, cout, n, h, w, e_w, e_b, need))
    assert e_w < 1e-4 and e_b < 1e-4
    dw2 = A.output_arena((k, k, 6, cout), torch.float32, rt.device, name="dw")
    ws2 = A.workspace_arena(need - 1, rt.device)
    assert rt.lib.vcg_conv_in_gate_up_bf16_wgrad(ctypes.byref(d), ua.ptr, za.ptr, dw2.ptr, None, ws2.ptr, need - 1, rt.stream) == E_WORKSPACE
    torch.cuda.current_stream().synchronize()
    dw2.check()
    ws2.check()
    assert dw2.untouched() and ws2.untouched()


@pytest.mark.parametrize("n,h,w", [(2, 9, 20), (1, 37, 70)])
def test_final_conv_c128_wgrad_contract(rt, n, h, w):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    g = torch.Generator().manual_seed(90 * h + w)
    x, dz = _nhwc_bf16(torch.randn(n, 128, h, w, generator=g)), torch.randn(n, 3, h, w, generator=g)
    wr = torch.zeros(9, 9, 128, 3, dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad((K.conv2d(_nchw(x), wr, None, 1, "same") * _r(dz)).sum(), [wr])
    d = L.ConvDesc(n, 128, h, w, 3, h, w, 9, 9, 1, 4, 4)
    need = rt.lib.vcg_conv9x9_c128to3_bf16_wgrad_ws_bytes(ctypes.byref(d))
    assert need > 0
    xa, za = A.input_arena(x, rt.device, name="x"), A.input_arena(dz, rt.device, name="dz")
    ws = A.workspace_arena(need, rt.device)
    dwa = A.output_arena((9, 9, 128, 3), torch.float32, rt.device, name="dw")
    assert rt.lib.vcg_conv9x9_c128to3_bf16_wgrad(ctypes.byref(d), xa.ptr, za.ptr, dwa.ptr, ws.ptr, need, rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    _check_inputs("vcg_conv9x9_c128to3_bf16_wgrad", [(xa, x), (za, dz)])
    ws.check()
    dwa.check()
    dw = dwa.view(torch.float32, (9, 9, 128, 3)).cpu()
    e = rel_err(dw, gw)
    report("abi contract vcg_conv9x9_c128to3_bf16_wgrad n=%d %dx%d: dw=%.2e (workspace %d bytes)" % (n, h, w, e, need))
    assert not torch.isnan(dw).any() and e < 1e-5
    dw2 = A.output_arena((9, 9, 128, 3), torch.float32, rt.device, name="dw")
    ws2 = A.workspace_arena(need - 1, rt.device)
    assert rt.lib.vcg_conv9x9_c128to3_bf16_wgrad(ctypes.byref(d), xa.ptr, za.ptr, dw2.ptr, ws2.ptr, need - 1, rt.stream) == E_WORKSPACE
    torch.cuda.current_stream().synchronize()
    dw2.check()
    ws2.check()
    assert dw2.untouched() and ws2.untouched()


@pytest.mark.parametrize("s,n,h,w", [(2, 2, 5, 7), (4, 1, 9, 12)])
def test_add_input_fwd_and_bwd_contract(rt, s, n, h, w):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    cout, slope = 128, 0.2
    g = torch.Generator().manual_seed(70 * s + 10 * h + w)
    x = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    wk = torch.randn(s + 1, s + 1, cout, 3, generator=g) * 0.2
    bias = torch.randn(cout, generator=g)
    yact = torch.randn(n, s * h, s * w, cout, generator=g).to(torch.bfloat16)
    dY = torch.randn(n, s * h, s * w, cout, generator=g).to(torch.bfloat16)
    d = L.ConvDesc(n, 3, h, w, cout, s * h, s * w, s + 1, s + 1, s, 0, 0)
    xa, wa, ba, ya, ga = (A.input_arena(t, rt.device, name=nm) for t, nm in ((x, "x"), (wk, "w_hwoi"), (bias, "bias"), (yact, "y_act"), (dY, "dY")))
    shape = (n, s * h, s * w, cout)
    # forward, out of place
    yo = A.output_arena(shape, torch.bfloat16, rt.device, name="y_out")
    assert rt.lib.vcg_input_convt_add_bf16_to(ctypes.byref(d), xa.ptr, wa.ptr, ba.ptr, ya.ptr, yo.ptr, rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    _check_inputs("vcg_input_convt_add_bf16_to", [(xa, x), (wa, wk), (ba, bias), (ya, yact)])
    yo.check()
    a = torch.atanh(float(torch.tensor(0.99999, dtype=torch.float32)) * x.double())          # the kernel's fp32 constant
    ref = _nchw(yact) + K.conv2d_transpose_same(a, wk.double(), bias.double(), s)
    got = _nchw(yo.view(torch.bfloat16, shape).cpu())
    e, ew = rel_err(got, ref), _ulp_scaled(got, ref)
    report("abi contract vcg_input_convt_add_bf16_to s%d n=%d %dx%d: err=%.2e ulp-scaled=%.2f" % (s, n, h, w, e, ew))
    assert not torch.isnan(got).any() and e < TOL_BF16 and ew < 1.0
    # backward
    need = rt.lib.vcg_input_convt_add_bf16_bwd_ws_bytes(ctypes.byref(d))
    assert need > 0
    ws = A.workspace_arena(need, rt.device)
    dza = A.output_arena(shape, torch.bfloat16, rt.device, name="dz")
    dwa = A.output_arena((s + 1, s + 1, cout, 3), torch.float32, rt.device, name="dw")
    dba, dbc = (A.output_arena((cout,), torch.float32, rt.device, name=nm) for nm in ("dbias_to_add", "dbias_convt"))
    assert rt.lib.vcg_input_convt_add_bf16_bwd(ctypes.byref(d), xa.ptr, ga.ptr, ya.ptr, slope, dza.ptr, dwa.ptr, dba.ptr, dbc.ptr, ws.ptr, need,
                                               rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    _check_inputs("vcg_input_convt_add_bf16_bwd", [(xa, x), (ga, dY), (ya, yact)])
    for arena in (ws, dza, dwa, dba, dbc):
        arena.check()
    dz = dza.view(torch.bfloat16, shape).cpu()
    ref_dz = torch.where(yact.float() > 0, dY, (dY.float() * slope).to(torch.bfloat16))
    assert torch.equal(dz.view(torch.int16), ref_dz.view(torch.int16))
    wr = torch.zeros(s + 1, s + 1, cout, 3, dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad((K.conv2d_transpose_same(a.float().double(), wr, None, s) * _nchw(dY)).sum(), [wr])
    dw, db_a, db_c = dwa.view(torch.float32, (s + 1, s + 1, cout, 3)).cpu(), dba.view(torch.float32).cpu(), dbc.view(torch.float32).cpu()
    for t in (dw, db_a, db_c):
        assert not torch.isnan(t).any()
    e_w, e_a, e_c = rel_err(dw, gw), rel_err(db_a, dY.double().sum((0, 1, 2))), rel_err(db_c, dz.double().sum((0, 1, 2)))
    report("abi contract vcg_input_convt_add_bf16_bwd s%d n=%d %dx%d: dw=%.2e dbias_to_add=%.2e dbias_convt=%.2e (workspace %d bytes)"
           % (s, n, h, w, e_w, e_a, e_c, need))
    assert e_w < 1e-4 and e_a < 1e-4 and e_c < 1e-4
    # one byte short: refused, nothing written
    outs = [A.output_arena(shape, torch.bfloat16, rt.device, name="dz"), A.output_arena((s + 1, s + 1, cout, 3), torch.float32, rt.device, name="dw"),
            A.output_arena((cout,), torch.float32, rt.device, name="dbias_to_add"), A.output_arena((cout,), torch.float32, rt.device, name="dbias_convt"),
            A.workspace_arena(need - 1, rt.device)]
    assert rt.lib.vcg_input_convt_add_bf16_bwd(ctypes.byref(d), xa.ptr, ga.ptr, ya.ptr, slope, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr,
                                               outs[4].ptr, need - 1, rt.stream) == E_WORKSPACE
    torch.cuda.current_stream().synchronize()
    for arena in outs:
        arena.check()
        assert arena.untouched()


def test_tail_refusals_leave_everything_untouched(rt):
    from upscaler import _lib as L
    lib = rt.lib
    one = A.input_arena(torch.zeros(1 << 16), rt.device, name="operand")
    two = A.input_arena(torch.zeros(1 << 16), rt.device, name="operand 2")
    o1, o2, o3, o4 = (A.output_arena((1 << 16,), torch.float32, rt.device, name="out %d" % i) for i in range(4))
    ws = A.workspace_arena(1 << 20, rt.device)
    # the up-sampling gates' backward
    good = L.ConvDesc(1, 6, 4, 4, 128, 4, 4, 3, 3, 1, 1, 1)
    bwd = lambda d, m=two.ptr, dres=two.ptr, dm=o1.ptr, da=o2.ptr: lib.vcg_conv_in_gate_up_bf16_bwd(ctypes.byref(d), one.ptr, one.ptr, one.ptr, m, one.ptr, dres,
                                                                                                   dm, da, rt.stream)
    for d in (L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 3, 3, 1, 1, 1), L.ConvDesc(1, 6, 4, 4, 256, 4, 4, 3, 3, 1, 1, 1), L.ConvDesc(1, 6, 4, 4, 128, 4, 4, 7, 7, 1, 3, 3),
              L.ConvDesc(1, 6, 4, 4, 128, 4, 4, 3, 3, 2, 1, 1), L.ConvDesc(1, 6, 4, 4, 128, 4, 4, 5, 5, 1, 1, 1)):
        assert bwd(d) == E_UNSUPPORTED
    assert bwd(good, dres=o1.ptr) == E_UNSUPPORTED and bwd(good, m=o1.ptr) == E_UNSUPPORTED and bwd(good, da=o1.ptr) == E_UNSUPPORTED
    assert bwd(L.ConvDesc(0, 6, 4, 4, 128, 4, 4, 3, 3, 1, 1, 1)) == E_SHAPE
    # their weight gradient: odd width, cin 3, cout 256, k 7
    for d in (L.ConvDesc(1, 6, 4, 5, 128, 4, 5, 5, 5, 1, 2, 2), L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 5, 5, 1, 2, 2), L.ConvDesc(1, 6, 4, 4, 256, 4, 4, 3, 3, 1, 1, 1),
              L.ConvDesc(1, 6, 4, 4, 128, 4, 4, 7, 7, 1, 3, 3)):
        assert lib.vcg_conv_in_gate_up_bf16_wgrad_ws_bytes(ctypes.byref(d)) == 0
        assert lib.vcg_conv_in_gate_up_bf16_wgrad(ctypes.byref(d), one.ptr, one.ptr, o1.ptr, o2.ptr, ws.ptr, 1 << 20, rt.stream) == E_UNSUPPORTED
    assert lib.vcg_conv_in_gate_up_bf16_wgrad(ctypes.byref(good), one.ptr, one.ptr, None, o2.ptr, ws.ptr, 1 << 20, rt.stream) == E_NULL
    # final/conv at 128: other channel counts, odd width
    for d in (L.ConvDesc(1, 256, 4, 4, 3, 4, 4, 9, 9, 1, 4, 4), L.ConvDesc(1, 64, 4, 4, 3, 4, 4, 9, 9, 1, 4, 4), L.ConvDesc(1, 128, 4, 5, 3, 4, 5, 9, 9, 1, 4, 4)):
        assert lib.vcg_conv9x9_c128to3_bf16_wgrad(ctypes.byref(d), one.ptr, one.ptr, o1.ptr, ws.ptr, 1 << 20, rt.stream) == E_UNSUPPORTED
    # to_add_input out of place and its backward: stride 3, cin 6, cout 12; dz == dY, dz == y_act; more than 256 units
    ok4 = L.ConvDesc(1, 3, 2, 2, 128, 8, 8, 5, 5, 4, 0, 0)
    for d in (L.ConvDesc(1, 3, 2, 2, 128, 6, 6, 4, 4, 3, 0, 0), L.ConvDesc(1, 6, 2, 2, 128, 8, 8, 5, 5, 4, 0, 0), L.ConvDesc(1, 3, 2, 2, 12, 8, 8, 5, 5, 4, 0, 0)):
        assert lib.vcg_input_convt_add_bf16_to(ctypes.byref(d), one.ptr, one.ptr, one.ptr, two.ptr, o1.ptr, rt.stream) == E_UNSUPPORTED
        assert lib.vcg_input_convt_add_bf16_bwd(ctypes.byref(d), one.ptr, one.ptr, two.ptr, 0.2, o1.ptr, o2.ptr, o3.ptr, o4.ptr, ws.ptr, 1 << 20,
                                                rt.stream) == E_UNSUPPORTED
    abwd = lambda d, dy=one.ptr, ya=two.ptr, dz=o1.ptr: lib.vcg_input_convt_add_bf16_bwd(ctypes.byref(d), one.ptr, dy, ya, 0.2, dz, o2.ptr, o3.ptr, o4.ptr,
                                                                                        ws.ptr, 1 << 20, rt.stream)
    assert abwd(ok4, dy=o1.ptr) == E_UNSUPPORTED and abwd(ok4, ya=o1.ptr) == E_UNSUPPORTED
    assert abwd(L.ConvDesc(1, 3, 2, 2, 136, 8, 8, 5, 5, 4, 0, 0)) == E_UNSUPPORTED
    assert abwd(L.ConvDesc(1, 3, 2, 2, 128, 8, 9, 5, 5, 4, 0, 0)) == E_SHAPE
    torch.cuda.current_stream().synchronize()
    for a in (one, two, o1, o2, o3, o4, ws):
        a.check()
    assert all(a.untouched() for a in (o1, o2, o3, o4, ws))

"""The memory contract of the entry points the bf16 trunk training of make_upscaler_attention adds (include/vcg.h), as
tests/test_abi_attention_contract_gpu.py checks the inference ones: vcg_conv_in_gate_bf16_bwd and vcg_conv3ch_bf16_wgrad at 5x5 with every
buffer inside a guarded arena (tests/_arena.py), the weight pack and the workspace of EXACTLY the queried byte counts; after each call the
guards are intact, the inputs hold their bytes, the outputs are fully written (their NaN prefill is gone) and match the fp64 reference on
the same bf16-rounded operands.  Refused calls return their error code and leave every output at its prefill."""
import ctypes

import pytest
import torch

import _arena as A
from conftest import rel_err, report

pytestmark = pytest.mark.gpu
OK, E_NULL, E_UNSUPPORTED, E_WORKSPACE = 0, -1, -3, -4
TOL_BF16 = 2.0 ** -8


def _r(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _nhwc_bf16(t):
    return t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def _ulp_scaled(got, ref):
    return float(((got - ref).abs() / (ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max())).max())


def _check_inputs(name, inputs):
    for a, t in inputs:
        a.check()
        assert torch.equal(a.payload.cpu(), t.contiguous().view(-1).view(torch.uint8)), "%s modified its input %s" % (name, a.name)


@pytest.mark.parametrize("k,n,h,w,with_dres", [(5, 2, 13, 45, True), (3, 1, 25, 33, False), (3, 1, 1, 1, True)])
def test_conv_in_gate_bwd_contract(rt, k, n, h, w, with_dres):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    g = torch.Generator().manual_seed(k * 1000 + h * 10 + w)
    u = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    wk = torch.randn(k, k, 3, 64, generator=g) * (2.5 / (k * k) ** 0.5)
    bias = torch.rand(64, generator=g) * 2 - 1
    m, dy, dres = (_nhwc_bf16(torch.randn(n, 64, h, w, generator=g)) for _ in range(3))
    nbytes = rt.lib.vcg_conv_in_gate_bf16_wfrag_bytes(3, k, k, 64)
    assert nbytes == k * ((k + 3) // 4) * 2048
    wa = A.input_arena(wk, rt.device, name="w_hwio")
    pk = A.output_arena((nbytes,), torch.uint8, rt.device, name="wfrag")
    assert rt.lib.vcg_pack_conv_in_gate_bf16(wa.ptr, 3, k, k, 64, pk.ptr, rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    pk.check()
    wf = pk.payload.cpu()
    ua, fa, ba, ma, ya, ra = (A.input_arena(t, rt.device, name=nm) for t, nm in ((u, "u"), (wf, "wfrag"), (bias, "bias"), (m, "m"), (dy, "dy"), (dres, "dres")))
    dma, daa = (A.output_arena((n, h, w, 64), torch.bfloat16, rt.device, name=nm) for nm in ("dm", "da"))
    d = L.ConvDesc(n, 3, h, w, 64, h, w, k, k, 1, k // 2, k // 2)
    assert rt.lib.vcg_conv_in_gate_bf16_bwd(ctypes.byref(d), ua.ptr, fa.ptr, ba.ptr, ma.ptr, ya.ptr, ra.ptr if with_dres else None, dma.ptr, daa.ptr,
                                            rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    name = "vcg_conv_in_gate_bf16_bwd k%d %dx%d%s" % (k, h, w, " +dres" if with_dres else "")
    _check_inputs(name, [(ua, u), (fa, wf), (ba, bias), (ma, m), (ya, dy), (ra, dres)])
    s = torch.sigmoid(K.conv2d(_r(u), _r(wk), bias.double(), 1, "same"))
    nchw = lambda t: t.double().permute(0, 3, 1, 2)
    ref_dm = nchw(dy) * s + (nchw(dres) if with_dres else 0.0)
    ref_da = nchw(dy) * nchw(m) * s * (1 - s)
    for a, ref, nm in ((dma, ref_dm, "dm"), (daa, ref_da, "da")):
        a.check()
        got = nchw(a.view(torch.bfloat16, (n, h, w, 64)).cpu())
        assert not torch.isnan(got).any(), "%s left NaN in %s" % (name, nm)
        e, ew = rel_err(got, ref), _ulp_scaled(got, ref)
        report("abi contract %-44s %s err=%.2e ulp-scaled=%.2f" % (name, nm, e, ew))
        assert e < TOL_BF16 and ew < 1.0


@pytest.mark.parametrize("n,h,w", [(2, 9, 20), (1, 37, 70)])
def test_conv3ch_wgrad_k5_contract(rt, n, h, w):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    g = torch.Generator().manual_seed(50 * h + w)
    x, dz = torch.rand(n, 3, h, w, generator=g) * 2 - 1, _nhwc_bf16(torch.randn(n, 64, h, w, generator=g))
    wr = torch.zeros(5, 5, 3, 64, dtype=torch.float64, requires_grad=True)
    br = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    gw, gb = torch.autograd.grad((K.conv2d(_r(x), wr, br, 1, "same") * dz.double().permute(0, 3, 1, 2)).sum(), [wr, br])
    d = L.ConvDesc(n, 3, h, w, 64, h, w, 5, 5, 1, 2, 2)
    need = rt.lib.vcg_conv3ch_bf16_wgrad_workspace_bytes(ctypes.byref(d))
    assert need > 0
    xa, za = A.input_arena(x, rt.device, name="x"), A.input_arena(dz, rt.device, name="dz")
    ws = A.workspace_arena(need, rt.device)
    dwa, dba = A.output_arena((5, 5, 3, 64), torch.float32, rt.device, name="dw"), A.output_arena((64,), torch.float32, rt.device, name="db")
    assert rt.lib.vcg_conv3ch_bf16_wgrad(ctypes.byref(d), xa.ptr, za.ptr, dwa.ptr, dba.ptr, ws.ptr, need, rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    _check_inputs("vcg_conv3ch_bf16_wgrad k5", [(xa, x), (za, dz)])
    for a in (ws, dwa, dba):
        a.check()
    dw, db = dwa.view(torch.float32, (5, 5, 3, 64)).cpu(), dba.view(torch.float32).cpu()
    assert not torch.isnan(dw).any() and not torch.isnan(db).any()
    e_w, e_b = rel_err(dw, gw), rel_err(db, gb)
    report("abi contract vcg_conv3ch_bf16_wgrad k5 n=%d %dx%d: dw=%.2e db=%.2e (workspace %d bytes)" % (n, h, w, e_w, e_b, need))
    assert e_w < 1e-4 and e_b < 1e-4
    # one byte short: refused, nothing written
    dw2 = A.output_arena((5, 5, 3, 64), torch.float32, rt.device, name="dw")
    assert rt.lib.vcg_conv3ch_bf16_wgrad(ctypes.byref(d), xa.ptr, za.ptr, dw2.ptr, None, ws.ptr, need - 1, rt.stream) == E_WORKSPACE
    torch.cuda.current_stream().synchronize()
    dw2.check()
    assert dw2.untouched()


def test_refusals_leave_everything_untouched(rt):
    from upscaler import _lib as L
    lib = rt.lib
    one = A.input_arena(torch.zeros(4096), rt.device, name="operand")
    two = A.input_arena(torch.zeros(4096), rt.device, name="operand 2")
    dm, da = A.output_arena((4096,), torch.float32, rt.device, name="dm"), A.output_arena((4096,), torch.float32, rt.device, name="da")
    good = L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 3, 3, 1, 1, 1)
    bwd = lambda d, u=one.ptr, wf=one.ptr, b=one.ptr, m=one.ptr, dy=one.ptr, dres=two.ptr, dm_=dm.ptr, da_=da.ptr: \
        lib.vcg_conv_in_gate_bf16_bwd(ctypes.byref(d) if d is not None else None, u, wf, b, m, dy, dres, dm_, da_, rt.stream)
    # cin 6, cout 128, k 7, k 4, stride 2, wrong pads, non-square
    for d in (L.ConvDesc(1, 6, 4, 4, 64, 4, 4, 3, 3, 1, 1, 1), L.ConvDesc(1, 3, 4, 4, 128, 4, 4, 3, 3, 1, 1, 1), L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 7, 7, 1, 3, 3),
              L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 4, 4, 1, 2, 2), L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 3, 3, 2, 1, 1), L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 5, 5, 1, 1, 1),
              L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 5, 3, 1, 2, 1)):
        assert bwd(d) == E_UNSUPPORTED
    assert bwd(good, dres=dm.ptr) == E_UNSUPPORTED             # dm == dres
    assert bwd(good, m=dm.ptr) == E_UNSUPPORTED                # dm == m
    assert bwd(good, da_=dm.ptr) == E_UNSUPPORTED              # dm == da
    for kw in (dict(u=None), dict(wf=None), dict(m=None), dict(dy=None), dict(dm_=None), dict(da_=None)):
        assert bwd(good, **kw) == E_NULL
    assert bwd(None) == E_NULL
    # the 3-channel weight gradient: kernel sizes it has no instantiation for, stride, odd width, NULL pointers
    ws = A.workspace_arena(1 << 20, rt.device)
    for d in (L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 7, 7, 1, 3, 3), L.ConvDesc(1, 3, 4, 4, 64, 2, 2, 5, 5, 2, 2, 2), L.ConvDesc(1, 3, 4, 5, 64, 4, 5, 5, 5, 1, 2, 2),
              L.ConvDesc(1, 6, 4, 4, 64, 4, 4, 5, 5, 1, 2, 2)):
        assert lib.vcg_conv3ch_bf16_wgrad_workspace_bytes(ctypes.byref(d)) == 0
        assert lib.vcg_conv3ch_bf16_wgrad(ctypes.byref(d), one.ptr, one.ptr, dm.ptr, da.ptr, ws.ptr, 1 << 20, rt.stream) == E_UNSUPPORTED
    d5 = L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 5, 5, 1, 2, 2)
    assert lib.vcg_conv3ch_bf16_wgrad(ctypes.byref(d5), None, one.ptr, dm.ptr, da.ptr, ws.ptr, 1 << 20, rt.stream) == E_NULL
    assert lib.vcg_conv3ch_bf16_wgrad(ctypes.byref(d5), one.ptr, one.ptr, None, da.ptr, ws.ptr, 1 << 20, rt.stream) == E_NULL
    assert lib.vcg_conv3ch_bf16_wgrad(ctypes.byref(d5), one.ptr, one.ptr, dm.ptr, da.ptr, None, 1 << 20, rt.stream) == E_NULL
    torch.cuda.current_stream().synchronize()
    for a in (one, two, dm, da, ws):
        a.check()
    assert dm.untouched() and da.untouched() and ws.untouched()

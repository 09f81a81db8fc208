"""The memory contract of head/conv on 64 channels (include/vcg.h: vcg_conv9x9_c64to3_bf16_wfrag_bytes, vcg_pack_conv9x9_c64to3_bf16,
vcg_conv9x9_c64to3_bf16_fwd, vcg_conv9x9_c64to3_bf16_fwd_window), as tests/test_abi_upscale_contract_gpu.py checks the 128 / 256-channel window
entry point: every buffer inside a guarded arena (tests/_arena.py) of exactly its stated size -- x [n][h][w][64] bf16, the weight pack of
exactly the queried bytes, y float [n][3][y_h][w] or uint8 [n][y_h][w][3] with no slack.  After the call the guards are intact, the inputs
hold their bytes, the window's rows are written and match the fp64 reference on the same bf16-rounded operands, and every other byte of y
keeps its prefill.  The entry points take no workspace."""
import ctypes

import pytest
import torch

import _arena as A
from conftest import rel_err, report

pytestmark = pytest.mark.gpu
OK, E_SHAPE, E_UNSUPPORTED = 0, -2, -3
TOL_BF16 = 2.0 ** -8


def _r(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _operands(rt, n, h, w):
    """x, kernel and bias on the host; the arenas of x (bf16 NHWC), of the weight pack (made by the pack entry point inside an output arena
    of exactly the queried size, then held in an input arena) and of the bias"""
    g = torch.Generator().manual_seed(64 + h * 10 + w)
    x = torch.randn(n, 64, h, w, generator=g)
    wk = torch.randn(9, 9, 64, 3, generator=g) * (1.0 / 72)
    bias = torch.randn(3, generator=g) * 0.3
    nbytes = rt.lib.vcg_conv9x9_c64to3_bf16_wfrag_bytes()
    assert nbytes == (2304 + 4) * 16
    wa = A.input_arena(wk, rt.device, name="w")
    pk = A.output_arena((nbytes,), torch.uint8, rt.device, name="wfrag")
    assert rt.lib.vcg_pack_conv9x9_c64to3_bf16(wa.ptr, pk.ptr, rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    pk.check()
    wa.check()
    assert torch.equal(wa.payload.cpu(), wk.contiguous().view(-1).view(torch.uint8))
    wf, xb = pk.payload.cpu(), x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    assert bool((wf[-64:] == 0).all())                       # the 64 zero bytes behind the fragments are written too
    arenas = [A.input_arena(t, rt.device, name=nm) for t, nm in ((xb, "x"), (wf, "wfrag"), (bias, "bias"))]
    return x, wk, bias, arenas, (xb, wf, bias)


def _inputs_intact(arenas, tensors):
    for a, t in zip(arenas, tensors):
        a.check()
        assert torch.equal(a.payload.cpu(), t.contiguous().view(-1).view(torch.uint8)), a.name


# n, h, w, (row0, rows, y_row0, y_h): the whole band into an image of its size, and sub-windows that end on the image's last row
CASES = [(1, 9, 70, (0, 9, 0, 9)), (2, 21, 67, (5, 9, 3, 12)), (1, 40, 66, (36, 4, 0, 4)), (2, 1, 1, (0, 1, 0, 1)), (1, 18, 131, (0, 7, 11, 18))]


@pytest.mark.parametrize("n,h,w,win", CASES)
@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_window_contract(rt, n, h, w, win, kind):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    row0, rows, y_row0, y_h = win
    x, wk, bias, arenas, tensors = _operands(rt, n, h, w)
    xa, fa, ba = arenas
    u8 = kind == "u8"
    ya = A.output_arena((n, y_h, w, 3) if u8 else (n, 3, y_h, w), torch.uint8 if u8 else torch.float32, rt.device, name="y")
    assert ya.nbytes == n * y_h * w * 3 * (1 if u8 else 4)
    d = L.ConvDesc(n, 64, h, w, 3, h, w, 9, 9, 1, 4, 4)
    assert rt.lib.vcg_conv9x9_c64to3_bf16_fwd_window(ctypes.byref(d), xa.ptr, fa.ptr, ba.ptr, 1, L.OUT_U8_NHWC if u8 else L.OUT_F32_NCHW, ya.ptr,
                                                     row0, rows, y_row0, y_h, rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    ya.check()
    _inputs_intact(arenas, tensors)
    ref = torch.tanh(K.conv2d(_r(x), _r(wk), bias.double(), 1, "same"))[:, :, row0:row0 + rows]
    inside = torch.zeros(y_h, dtype=torch.bool)
    inside[y_row0:y_row0 + rows] = True
    if u8:
        raw = ya.view(torch.uint8, (n, y_h, w, 3)).cpu()
        got = raw[:, inside].permute(0, 3, 1, 2).double()
        assert bool((raw[:, ~inside] == A.NAN_BYTE).all())                         # nothing outside the window's rows is written
        want = torch.clamp(torch.round((ref + 1) * 127.5), 0, 255)
        # the kernel's fp32 value is within 2^-8 (max-norm) of the reference (the fp32 form below): at most one uint8 step
        step = float((got - want).abs().max())
        report("abi contract vcg_conv9x9_c64to3_bf16_fwd_window u8 %dx%d rows %d+%d: max uint8 step %.0f" % (h, w, row0, rows, step))
        assert step <= 1.0
    else:
        raw = ya.view(torch.float32, (n, 3, y_h, w)).cpu()
        got = raw[:, :, inside].double()
        assert bool((ya.view(torch.uint8, (n, 3, y_h, w * 4)).cpu()[:, :, ~inside] == A.NAN_BYTE).all())
        assert not torch.isnan(got).any()
        e = rel_err(got, ref)
        ew = float(((got - ref).abs() / (ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max())).max())
        report("abi contract vcg_conv9x9_c64to3_bf16_fwd_window f32 %dx%d rows %d+%d: err=%.2e ulp-scaled=%.2f" % (h, w, row0, rows, e, ew))
        assert e < TOL_BF16 and ew < 1.0


@pytest.mark.parametrize("n,h,w", [(2, 1, 1), (1, 9, 70), (2, 21, 67)])
def test_whole_image_contract(rt, n, h, w):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    x, wk, bias, arenas, tensors = _operands(rt, n, h, w)
    xa, fa, ba = arenas
    ya = A.output_arena((n, 3, h, w), torch.float32, rt.device, name="y")
    d = L.ConvDesc(n, 64, h, w, 3, h, w, 9, 9, 1, 4, 4)
    assert rt.lib.vcg_conv9x9_c64to3_bf16_fwd(ctypes.byref(d), xa.ptr, fa.ptr, ba.ptr, 0, ya.ptr, rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    ya.check()
    _inputs_intact(arenas, tensors)
    got = ya.view(torch.float32, (n, 3, h, w)).cpu().double()
    assert not torch.isnan(got).any()
    ref = K.conv2d(_r(x), _r(wk), bias.double(), 1, "same")
    e = rel_err(got, ref)
    ew = float(((got - ref).abs() / (ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max())).max())
    report("abi contract vcg_conv9x9_c64to3_bf16_fwd n=%d %dx%d: err=%.2e ulp-scaled=%.2f" % (n, h, w, e, ew))
    assert e < TOL_BF16 and ew < 1.0


def test_refusals_leave_y_untouched(rt):
    from upscaler import _lib as L
    lib = rt.lib
    one = A.input_arena(torch.zeros(4096), rt.device, name="operand")
    out = A.output_arena((4096,), torch.float32, rt.device, name="out")
    d = L.ConvDesc(1, 64, 8, 8, 3, 8, 8, 9, 9, 1, 4, 4)
    call = lambda desc, kind, row0, rows, y_row0, y_h: lib.vcg_conv9x9_c64to3_bf16_fwd_window(
        ctypes.byref(desc), one.ptr, one.ptr, one.ptr, 1, kind, out.ptr, row0, rows, y_row0, y_h, rt.stream)
    for args in ((0, 0, 0, 8), (-1, 4, 0, 8), (5, 4, 0, 8), (0, 4, -1, 8), (0, 4, 5, 8)):
        assert call(d, L.OUT_U8_NHWC, *args) == E_SHAPE
    assert call(d, 2, 0, 8, 0, 8) == E_UNSUPPORTED
    for bad in (L.ConvDesc(1, 128, 8, 8, 3, 8, 8, 9, 9, 1, 4, 4), L.ConvDesc(1, 256, 8, 8, 3, 8, 8, 9, 9, 1, 4, 4),
                L.ConvDesc(1, 64, 8, 8, 3, 8, 8, 7, 7, 1, 3, 3)):
        assert call(bad, L.OUT_F32_NCHW, 0, 8, 0, 8) == E_UNSUPPORTED
        assert lib.vcg_conv9x9_c64to3_bf16_fwd(ctypes.byref(bad), one.ptr, one.ptr, one.ptr, 1, out.ptr, rt.stream) == E_UNSUPPORTED
    torch.cuda.current_stream().synchronize()
    one.check()
    out.check()
    assert out.untouched()

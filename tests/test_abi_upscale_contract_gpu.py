"""The memory contract of vcg_conv9x9_to3_bf16_fwd_window (include/vcg.h), as tests/test_abi_attention_contract_gpu.py checks the
attention generator's entry points: every buffer inside a guarded arena (tests/_arena.py) of exactly its stated size -- x [n][h][w][cin]
bf16, the weight pack of vcg_conv9x9_to3_bf16_wfrag_bytes(cin) bytes, y float [n][3][y_h][w] or uint8 [n][y_h][w][3] with no slack (a
store wider than a byte running past the last row's last pixel lands in the guard).  After the call the guards are intact, the inputs
hold their bytes, the window's rows are written and match the fp64 reference on the same bf16-rounded operands, and every other byte of y
keeps its prefill.  The entry point takes no workspace."""
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


# n, cin, h, w, (row0, rows, y_row0, y_h): the whole band into an image of its size, and sub-windows that end on the image's last row
CASES = [(1, 256, 9, 70, (0, 9, 0, 9)), (2, 128, 21, 67, (5, 9, 3, 12)), (1, 256, 40, 66, (36, 4, 0, 4)), (2, 128, 1, 1, (0, 1, 0, 1)),
         (1, 256, 18, 131, (0, 7, 11, 18))]


@pytest.mark.parametrize("n,cin,h,w,win", CASES)
@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_window_contract(rt, n, cin, h, w, win, kind):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    row0, rows, y_row0, y_h = win
    g = torch.Generator().manual_seed(cin + h * 10 + w)
    x = torch.randn(n, cin, h, w, generator=g)
    wk = torch.randn(9, 9, cin, 3, generator=g) * (1.0 / (9 * cin ** 0.5))
    bias = torch.randn(3, generator=g) * 0.3
    nbytes = rt.lib.vcg_conv9x9_to3_bf16_wfrag_bytes(cin)
    wa = A.input_arena(wk, rt.device, name="w")
    pk = A.output_arena((nbytes,), torch.uint8, rt.device, name="wfrag")
    assert rt.lib.vcg_pack_conv9x9_to3_bf16(wa.ptr, cin, pk.ptr, rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    pk.check()
    wf, xb = pk.payload.cpu(), x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    xa, fa, ba = (A.input_arena(t, rt.device, name=nm) for t, nm in ((xb, "x"), (wf, "wfrag"), (bias, "bias")))
    u8 = kind == "u8"
    ya = A.output_arena((n, y_h, w, 3) if u8 else (n, 3, y_h, w), torch.uint8 if u8 else torch.float32, rt.device, name="y")
    assert ya.nbytes == n * y_h * w * 3 * (1 if u8 else 4)
    d = L.ConvDesc(n, cin, h, w, 3, h, w, 9, 9, 1, 4, 4)
    assert rt.lib.vcg_conv9x9_to3_bf16_fwd_window(ctypes.byref(d), xa.ptr, fa.ptr, ba.ptr, 1, L.OUT_U8_NHWC if u8 else L.OUT_F32_NCHW, ya.ptr,
                                                  row0, rows, y_row0, y_h, rt.stream) == OK
    torch.cuda.current_stream().synchronize()
    for a in (xa, fa, ba, ya):
        a.check()
    for a, t in ((xa, xb), (fa, wf), (ba, bias)):
        assert torch.equal(a.payload.cpu(), t.contiguous().view(-1).view(torch.uint8)), a.name
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
        report("abi contract vcg_conv9x9_to3_bf16_fwd_window u8 cin%d %dx%d rows %d+%d: max uint8 step %.0f" % (cin, h, w, row0, rows, step))
        assert step <= 1.0
    else:
        raw = ya.view(torch.float32, (n, 3, y_h, w)).cpu()
        got = raw[:, :, inside].double()
        assert bool((ya.view(torch.uint8, (n, 3, y_h, w * 4)).cpu()[:, :, ~inside] == A.NAN_BYTE).all())
        assert not torch.isnan(got).any()
        e = rel_err(got, ref)
        ew = float(((got - ref).abs() / (ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max())).max())
        report("abi contract vcg_conv9x9_to3_bf16_fwd_window f32 cin%d %dx%d rows %d+%d: err=%.2e ulp-scaled=%.2f" % (cin, h, w, row0, rows, e, ew))
        assert e < TOL_BF16 and ew < 1.0


def test_window_refusals_leave_y_untouched(rt):
    from upscaler import _lib as L
    lib = rt.lib
    one = A.input_arena(torch.zeros(4096), rt.device, name="operand")
    out = A.output_arena((4096,), torch.float32, rt.device, name="out")
    d = L.ConvDesc(1, 256, 8, 8, 3, 8, 8, 9, 9, 1, 4, 4)
    call = lambda desc, kind, row0, rows, y_row0, y_h: lib.vcg_conv9x9_to3_bf16_fwd_window(
        ctypes.byref(desc), one.ptr, one.ptr, one.ptr, 1, kind, out.ptr, row0, rows, y_row0, y_h, rt.stream)
    for args in ((0, 0, 0, 8), (-1, 4, 0, 8), (5, 4, 0, 8), (0, 4, -1, 8), (0, 4, 5, 8)):
        assert call(d, L.OUT_U8_NHWC, *args) == E_SHAPE
    assert call(d, 2, 0, 8, 0, 8) == E_UNSUPPORTED
    for bad in (L.ConvDesc(1, 64, 8, 8, 3, 8, 8, 9, 9, 1, 4, 4), L.ConvDesc(1, 256, 8, 8, 3, 8, 8, 7, 7, 1, 3, 3)):
        assert call(bad, L.OUT_F32_NCHW, 0, 8, 0, 8) == E_UNSUPPORTED
    torch.cuda.current_stream().synchronize()
    one.check()
    out.check()
    assert out.untouched()

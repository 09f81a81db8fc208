"""The memory contract of the entry points behind the fp32 predict-pass fusion (include/vcg.h: vcg_conv2d_fwd_affine,
vcg_norm_finalize_batch), in the manner of tests/test_abi_cyclegan_contract_gpu.py: every buffer inside a guarded arena (tests/_arena.py) of
exactly its stated size (the entry points take no workspace).  After the call the guards are intact, the inputs hold their bytes, every output
word is written (no NaN of the prefill survives) and has the bits of the launches it replaces; the shapes the header names as unsupported
return VCG_E_UNSUPPORTED with nothing written."""
import ctypes

import numpy as np
import pytest
import torch

import _arena as A
from conftest import report

pytestmark = pytest.mark.gpu
OK, E_SHAPE, E_UNSUPPORTED = 0, -2, -3
BN_EPS = 1e-3


def _inputs(rt, **tensors):
    arenas = {k: A.input_arena(t.float(), rt.device, name=k) for k, t in tensors.items()}
    return arenas, {k: t.float().contiguous().view(-1).view(torch.uint8) for k, t in tensors.items()}


def _intact(arenas, raw):
    for k, a in arenas.items():
        a.check()
        assert torch.equal(a.payload.cpu(), raw[k]), k


def _affine_operands(rt, cin, cout, k, n, h, w):
    g = torch.Generator().manual_seed(cin + cout * 3 + k + w)
    return _inputs(rt, x=torch.randn(n, cin, h, w, generator=g), w=torch.randn(k, k, cin, cout, generator=g) / np.sqrt(k * k * cin),
                   bias=torch.rand(cout, generator=g) - 0.5, slopes=torch.rand(cout, generator=g) - 0.4, res=torch.randn(n, cout, h, w, generator=g),
                   mmean=torch.rand(cout, generator=g) - 0.5, mvar=torch.rand(cout, generator=g) * 2, gamma=torch.rand(cout, generator=g) + 0.5,
                   beta=torch.rand(cout, generator=g) - 0.7)


@pytest.mark.parametrize("cin,cout,k,n,h,w", [(24, 40, 3, 2, 17, 33), (64, 70, 3, 1, 9, 30), (8, 64, 5, 2, 9, 40)])
def test_finalize_batch_and_affine_forward_contract(rt, cin, cout, k, n, h, w):
    from upscaler import _lib as L
    ar, raw = _affine_operands(rt, cin, cout, k, n, h, w)
    d = L.ConvDesc(n, cin, h, w, cout, h, w, k, k, 1, k // 2, k // 2)
    # two normalisations in one launch: scale, shift [2][cout]
    sc, sh = A.output_arena((2, cout), torch.float32, rt.device, name="scale"), A.output_arena((2, cout), torch.float32, rt.device, name="shift")
    col = lambda key: (ctypes.c_void_p * 2)(ar[key].ptr, ar[key].ptr)
    assert rt.lib.vcg_norm_finalize_batch(col("mmean"), col("mvar"), col("gamma"), col("beta"), 2, cout, BN_EPS, sc.ptr, sh.ptr, rt.stream) == OK
    assert rt.lib.vcg_norm_finalize_batch(col("mmean"), col("mvar"), col("gamma"), col("beta"), 49, cout, BN_EPS, sc.ptr, sh.ptr, rt.stream) == E_SHAPE
    sc.check(); sh.check()
    one_s, one_h, inv = (A.output_arena((cout,), torch.float32, rt.device, name=nm) for nm in ("scale1", "shift1", "invstd"))
    assert rt.lib.vcg_norm_finalize(ar["mmean"].ptr, ar["mvar"].ptr, ar["gamma"].ptr, ar["beta"].ptr, cout, 1, BN_EPS, one_s.ptr, one_h.ptr, inv.ptr,
                                    None, None, 0.0, 0, rt.stream) == OK
    for i in range(2):
        assert torch.equal(sc.view(torch.float32, (2, cout))[i], one_s.view(torch.float32))
        assert torch.equal(sh.view(torch.float32, (2, cout))[i], one_h.view(torch.float32))
    # the three launches
    z, want, got = (A.output_arena((n, cout, h, w), torch.float32, rt.device, name=nm) for nm in ("z", "want", "y"))
    ep = L.Epilogue(ar["bias"].ptr, L.ACT_NONE, 0.0, None, None)
    assert rt.lib.vcg_conv2d_fwd(ctypes.byref(d), ar["x"].ptr, ar["w"].ptr, z.ptr, ctypes.byref(ep), rt.stream) == OK
    assert rt.lib.vcg_norm_act_fwd(z.ptr, n, cout, h * w, one_s.ptr, one_h.ptr, 0, L.ACT_PRELU, 0.0, ar["slopes"].ptr, ar["res"].ptr, want.ptr,
                                   rt.stream) == OK
    ep = L.Epilogue(ar["bias"].ptr, L.ACT_PRELU, 0.0, ar["slopes"].ptr, ar["res"].ptr)
    off = cout * 4                                                 # the second normalisation's slot
    assert rt.lib.vcg_conv2d_fwd_affine(ctypes.byref(d), ar["x"].ptr, ar["w"].ptr, got.ptr, ctypes.byref(ep), sc.ptr + off, sh.ptr + off,
                                        rt.stream) == OK
    for a in (z, want, got, sc, sh):
        a.check()
    _intact(ar, raw)
    y = got.view(torch.float32, (n, cout, h, w))
    assert not torch.isnan(y).any()
    report("abi contract vcg_conv2d_fwd_affine %d->%d k%d %dx%d: equal to the three launches %s" % (cin, cout, k, h, w, torch.equal(y, want.view(torch.float32, (n, cout, h, w)))))
    assert torch.equal(y, want.view(torch.float32, (n, cout, h, w)))


# 9x9 from 3 channels (conv_c3_kernel has no affine stage), stride 2, 4x4, few output channels (the small-M kernel), the statistics shapes' 1x1
@pytest.mark.parametrize("cin,cout,k,stride", [(3, 64, 9, 1), (64, 64, 3, 2), (64, 64, 4, 1), (64, 3, 3, 1), (64, 64, 1, 1), (64, 64, 9, 1)])
def test_affine_forward_unsupported_shapes_write_nothing(rt, cin, cout, k, stride):
    from upscaler import _lib as L
    n, h, w = 1, 12, 40
    oh, ow = (h + stride - 1) // stride, (w + stride - 1) // stride
    ar, raw = _affine_operands(rt, cin, cout, k, n, h, w)
    d = L.ConvDesc(n, cin, h, w, cout, oh, ow, k, k, stride, (k - 1) // 2, (k - 1) // 2)
    y = A.output_arena((n, cout, oh, ow), torch.float32, rt.device, name="y")
    ep = L.Epilogue(ar["bias"].ptr, L.ACT_NONE, 0.0, None, None)
    assert rt.lib.vcg_conv2d_fwd_affine(ctypes.byref(d), ar["x"].ptr, ar["w"].ptr, y.ptr, ctypes.byref(ep), ar["gamma"].ptr, ar["beta"].ptr,
                                        rt.stream) == E_UNSUPPORTED
    y.check()
    assert y.untouched()
    _intact(ar, raw)

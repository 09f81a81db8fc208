"""CPU-only ABI checks of the 5x5 bf16 weight gradient (bf16 training of the reference's default generator, kernel_size 5): the
workspace queries of vcg_conv2d_nhwc_bf16_wgrad / vcg_conv_transpose2d_nhwc_bf16_wgrad serve 5x5 at stride 1 and 2, and keep
refusing what the kernel is not instantiated for.  Pure host logic: no device is touched."""
import ctypes

import pytest

E_UNSUPPORTED = -3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from upscaler import _lib
    return _lib


def _queries(cl):
    return cl.vcg_conv2d_nhwc_bf16_wgrad_workspace_bytes, cl.vcg_conv_transpose2d_nhwc_bf16_wgrad_workspace_bytes


def test_workspace_queries_serve_5x5_at_stride_1_and_2(lib):
    L, cl = lib, lib.load()
    conv, convt = _queries(cl)
    # the trunk layer at the benchmark's shape, and the stride-2 form the transposed stages reduce to
    s1 = L.ConvDesc(8, 64, 256, 256, 64, 256, 256, 5, 5, 1, 2, 2)
    s2 = L.ConvDesc(2, 128, 15, 17, 64, 8, 9, 5, 5, 2, 2, 2)
    # Conv2DTranspose(256, 5, strides 2): 64 -> 256 and 256 -> 256 (both stages of an x4 generator); a stride-1 descriptor of the same
    # kernel takes the stride-1 form of the weight gradient
    t0 = L.ConvDesc(2, 64, 6, 10, 256, 12, 20, 5, 5, 2, 1, 1)
    t1 = L.ConvDesc(1, 256, 5, 7, 256, 10, 14, 5, 5, 2, 1, 1)
    t1s1 = L.ConvDesc(1, 256, 5, 7, 256, 5, 7, 5, 5, 1, 2, 2)
    got = [conv(ctypes.byref(s1)), conv(ctypes.byref(s2)), convt(ctypes.byref(t0)), convt(ctypes.byref(t1)), convt(ctypes.byref(t1s1))]
    assert all(0 < v < (1 << 31) for v in got), got
    # two tap groups of seven waves: 14 dumps of 8192 floats per (ci, co) block pair and slab, plus the bias partials.  One tile:
    small = L.ConvDesc(1, 64, 8, 16, 64, 8, 16, 5, 5, 1, 2, 2)
    assert conv(ctypes.byref(small)) == 14 * 8192 * 4 + 128 * 4


def test_workspace_queries_keep_refusing_unserved_shapes(lib):
    L, cl = lib, lib.load()
    conv, convt = _queries(cl)
    bad = [L.ConvDesc(1, 64, 16, 16, 64, 16, 16, 7, 7, 1, 3, 3),          # 7x7
           L.ConvDesc(1, 64, 16, 16, 64, 6, 6, 5, 5, 3, 2, 2),            # stride 3
           L.ConvDesc(1, 48, 16, 16, 64, 16, 16, 5, 5, 1, 2, 2),          # input channels not a multiple of 64
           L.ConvDesc(1, 64, 16, 16, 96, 16, 16, 5, 5, 1, 2, 2),          # output channels not a multiple of 64
           L.ConvDesc(1, 64, 16, 16, 64, 16, 16, 2, 2, 1, 0, 0)]          # 2x2
    for d in bad:
        assert conv(ctypes.byref(d)) == 0, (d.cin, d.cout, d.kh, d.stride)
    badt = [L.ConvDesc(1, 256, 8, 8, 256, 16, 16, 7, 7, 2, 2, 2), L.ConvDesc(1, 256, 8, 8, 256, 24, 24, 5, 5, 3, 1, 1),
            L.ConvDesc(1, 48, 8, 8, 256, 16, 16, 5, 5, 2, 1, 1), L.ConvDesc(1, 64, 8, 8, 96, 16, 16, 5, 5, 2, 1, 1)]
    for d in badt:
        assert convt(ctypes.byref(d)) == 0, (d.cin, d.cout, d.kh, d.stride)
    # the calls refuse them before any pointer is used
    one = ctypes.c_void_p(16)
    assert cl.vcg_conv2d_nhwc_bf16_wgrad(ctypes.byref(bad[0]), one, one, one, None, one, 1 << 30, None) == E_UNSUPPORTED
    assert cl.vcg_conv_transpose2d_nhwc_bf16_wgrad(ctypes.byref(badt[0]), one, one, one, one, 1 << 30, None) == E_UNSUPPORTED

"""CPU-only ABI checks of the entry points behind the reference-default bf16 inference (kernel_size 5, upscale_factor 4): the
shapes the new kernels do not serve keep returning an error code, checked before anything touches a device."""
import ctypes

import pytest

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from upscaler import _lib
    return _lib


def test_unserved_shapes_keep_their_error_codes(lib):
    L = lib
    cl = L.load()
    one = ctypes.c_void_p(16)                              # any non-null address: never dereferenced by the checks below
    # 5x5 on 128 input channels: not instantiated (as before)
    d = L.ConvDesc(1, 128, 8, 8, 64, 8, 8, 5, 5, 1, 2, 2)
    assert cl.vcg_conv2d_bf16_fwd(ctypes.byref(d), one, one, one, None, None) == E_UNSUPPORTED
    # 5x5 64 -> 64 with epilogue statistics: training statistics stay on the 3x3 kernels
    d = L.ConvDesc(1, 64, 8, 8, 64, 8, 8, 5, 5, 1, 2, 2)
    ep = L.EpilogueBf16(None, None, L.ACT_NONE, 0.0, None, None, one, L.STATS_BATCH)
    assert cl.vcg_conv2d_bf16_fwd(ctypes.byref(d), one, one, one, ctypes.byref(ep), None) == E_UNSUPPORTED
    assert cl.vcg_conv2d_bf16_stats_records(ctypes.byref(d), L.STATS_BATCH) == E_UNSUPPORTED
    assert cl.vcg_conv2d_bf16_stats_records(ctypes.byref(d), L.STATS_INSTANCE) == E_UNSUPPORTED
    # 5x5 with other pads or strides: not the 'same' trunk convolution
    for bad in (L.ConvDesc(1, 64, 8, 8, 64, 8, 8, 5, 5, 1, 1, 1), L.ConvDesc(1, 64, 8, 8, 64, 4, 4, 5, 5, 2, 2, 2)):
        assert cl.vcg_conv2d_bf16_fwd(ctypes.byref(bad), one, one, one, None, None) != 0
    # the transposed convolutions of the k5 / x4 topologies run on the generic entry point; the bf16-epilogue one keeps its contract
    # (3x3 on 64 input channels): these shapes stay refused there
    for dd in (L.ConvDesc(1, 64, 8, 8, 256, 16, 16, 5, 5, 2, 1, 1), L.ConvDesc(1, 256, 8, 8, 256, 16, 16, 5, 5, 2, 1, 1),
               L.ConvDesc(1, 256, 8, 8, 256, 16, 16, 3, 3, 2, 0, 0), L.ConvDesc(1, 256, 8, 8, 256, 16, 16, 7, 7, 2, 2, 2)):
        assert cl.vcg_conv_transpose2d_bf16_fwd(ctypes.byref(dd), one, one, one, None, None) == E_UNSUPPORTED
    # on the generic entry point: a 7x7 transposed convolution and a stride-1 one are not served
    d = L.ConvDesc(1, 256, 8, 8, 256, 16, 16, 7, 7, 2, 2, 2)
    assert cl.vcg_conv_transpose2d_nhwc_bf16_fwd(ctypes.byref(d), one, one, None, 0, 0.0, one, None) == E_UNSUPPORTED
    d = L.ConvDesc(1, 256, 8, 8, 256, 8, 8, 5, 5, 1, 2, 2)
    assert cl.vcg_conv_transpose2d_nhwc_bf16_fwd(ctypes.byref(d), one, one, None, 0, 0.0, one, None) == E_UNSUPPORTED
    # a launch whose output exceeds 4 GiB is an error code, never a wrong result (the engine splits the batch below it):
    # 32 frames of 512 x 512 x 256 bf16 = 4 GiB
    d = L.ConvDesc(32, 256, 256, 256, 256, 512, 512, 5, 5, 2, 1, 1)
    assert cl.vcg_conv_transpose2d_nhwc_bf16_fwd(ctypes.byref(d), one, one, None, 1, 0.2, one, None) == E_SHAPE
    d = L.ConvDesc(16, 256, 256, 256, 256, 512, 512, 5, 5, 2, 1, 1)
    assert cl.vcg_conv_transpose2d_bf16_fwd(ctypes.byref(d), one, one, one, None, None) == E_UNSUPPORTED
    # required pointers
    d = L.ConvDesc(1, 64, 8, 8, 64, 8, 8, 5, 5, 1, 2, 2)
    assert cl.vcg_conv2d_bf16_fwd(ctypes.byref(d), one, None, one, None, None) == E_NULL

"""CPU-only checks of what bf16 training of make_generator_cyclegan adds: the argument checks of vcg_conv2d_nhwc_bf16_dgrad_add
and of vcg_conv9x9_to3_bf16_wgrad at 64 channels (include/vcg.h) return their error codes before anything touches a device, and the layer
classes and the factory refuse the shapes they do not serve."""
import ctypes

import pytest

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from upscaler import _lib
    return _lib


def _desc(L, cin=256, cout=256, k=3, stride=1, h=9, w=20, n=2):
    oh, ow = -(-h // stride), -(-w // stride)
    return L.ConvDesc(n, cin, h, w, cout, oh, ow, k, k, stride, k // 2, k // 2)


def test_dgrad_add_null_pointers(lib):
    L = lib
    cl = L.load()
    one, two, three, four = (ctypes.c_void_p(v) for v in (256, 512, 768, 1024))          # non-null addresses the checks never dereference
    d = ctypes.byref(_desc(L))
    for args in ((None, one, two, three, four), (d, None, two, three, four), (d, one, None, three, four), (d, one, two, None, four),
                 (d, one, two, three, None)):
        assert cl.vcg_conv2d_nhwc_bf16_dgrad_add(*args, None) == E_NULL


def test_dgrad_add_shapes(lib):
    L = lib
    cl = L.load()
    one, two, three, four = (ctypes.c_void_p(v) for v in (256, 512, 768, 1024))
    call = lambda d, res=three, dx=four: cl.vcg_conv2d_nhwc_bf16_dgrad_add(ctypes.byref(d), one, two, res, dx, None)
    assert call(L.ConvDesc(0, 256, 9, 20, 256, 9, 20, 3, 3, 1, 1, 1)) == E_SHAPE                 # empty batch
    assert call(L.ConvDesc(2, 256, 9, 20, 256, 8, 20, 3, 3, 1, 1, 1)) == E_SHAPE                 # a stride-1 'same' layer keeps its size
    assert call(_desc(L, stride=2)) == E_UNSUPPORTED
    for cin, cout in ((32, 64), (64, 32), (96, 64), (64, 160)):                                  # multiples of 16 / 32, not of 64
        assert call(_desc(L, cin=cin, cout=cout)) == E_UNSUPPORTED
    assert call(_desc(L, k=5)) == E_UNSUPPORTED
    assert call(L.ConvDesc(2, 64, 9, 20, 64, 9, 20, 3, 3, 1, 0, 0)) == E_UNSUPPORTED             # 'valid' pads
    assert call(_desc(L), res=four, dx=four) == E_UNSUPPORTED                                    # the residual may not be dx itself


def test_head_conv_wgrad_accepts_64_channels(lib):
    """vcg_conv9x9_to3_bf16_wgrad at cin = 64: a workspace query of its own, VCG_E_WORKSPACE one byte below it, VCG_E_UNSUPPORTED at an odd
    width; other channel counts are refused by the query (0) and by the call"""
    L = lib
    cl = L.load()
    one = ctypes.c_void_p(256)
    E_WORKSPACE = -4
    desc = lambda cin, w=20: L.ConvDesc(2, cin, 9, w, 3, 9, w, 9, 9, 1, 4, 4)
    d = desc(64)
    need = cl.vcg_conv9x9_to3_bf16_wgrad_workspace_bytes(ctypes.byref(d))
    # 256 workgroups x 2 row tiles x (11 column tiles x 16 x 64) floats of register dumps + the bf16 [n][h][w][4] copy of dz + alignment slack
    assert need == 256 * 2 * 11 * 16 * 64 * 4 + 2 * 9 * 20 * 8 + 256
    assert need < cl.vcg_conv9x9_to3_bf16_wgrad_workspace_bytes(ctypes.byref(desc(256)))
    assert cl.vcg_conv9x9_to3_bf16_wgrad(ctypes.byref(d), one, one, one, one, need - 1, None) == E_WORKSPACE
    for arg in range(4):
        ptrs = [one] * 4
        ptrs[arg] = None
        assert cl.vcg_conv9x9_to3_bf16_wgrad(ctypes.byref(d), *ptrs, need, None) == E_NULL
    odd = desc(64, 21)
    assert cl.vcg_conv9x9_to3_bf16_wgrad(ctypes.byref(odd), one, one, one, one, 1 << 30, None) == E_UNSUPPORTED
    for cin in (32, 128):
        assert cl.vcg_conv9x9_to3_bf16_wgrad_workspace_bytes(ctypes.byref(desc(cin))) == 0
        assert cl.vcg_conv9x9_to3_bf16_wgrad(ctypes.byref(desc(cin)), one, one, one, one, 1 << 30, None) == E_UNSUPPORTED


def test_layers_refuse_what_they_do_not_serve():
    from upscaler import _engine as E
    for args in ((3, 64, 5), (3, 128, 9), (1, 64, 9)):
        with pytest.raises(NotImplementedError):
            E.StemConv9x9Bf16("s", *args)
    for args in ((256, 3, 9), (64, 1, 9), (64, 3, 5)):
        with pytest.raises(NotImplementedError):
            E.HeadConv9x9C64Bf16("h", *args)
    E.ConvTBf16("t", 128, 64, 3)                                   # the 256 -> 128 -> 64 stages
    E.ConvTBf16("t", 256, 128, 3)
    with pytest.raises(NotImplementedError):
        E.ConvTBf16("t", 128, 64, 5)


def test_factory_keyword_and_refusals_before_a_device_is_needed():
    from upscaler import _graph
    import inspect
    sig = inspect.signature(_graph.make_generator_cyclegan)
    assert sig.parameters["dtype"].default == "fp32"
    for kw in (dict(filters=32), dict(n_downsample=3), dict(kernel_size=7), dict(kernel_size=5), dict(norm=None), dict(upscale_factor=8)):
        with pytest.raises(NotImplementedError, match="filters=64"):
            _graph.make_generator_cyclegan((64, 64, 3), res_block_num=1, dtype="bf16", **kw)
    with pytest.raises(NotImplementedError, match="filters=64"):
        _graph.make_generator_cyclegan((64, 64, 4), res_block_num=1, dtype="bf16")
    with pytest.raises(ValueError):
        _graph.make_generator_cyclegan((64, 64, 3), res_block_num=1, dtype="fp16")

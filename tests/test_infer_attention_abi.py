"""CPU-only ABI checks of the attention generator's entry points (include/vcg.h): the size queries answer for the shapes that are served and
with 0 for the others, and unsupported descriptors, null pointers and y == m return their error codes before anything touches a device."""
import ctypes

import pytest

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from upscaler import _lib
    return _lib


def test_size_queries(lib):
    cl = lib.load()
    # [channel block][source x kernel row x group of 4 kernel columns][64 channels][2 halves] x 16 bytes
    assert cl.vcg_conv_in_gate_bf16_wfrag_bytes(3, 3, 3, 64) == 3 * 2048
    assert cl.vcg_conv_in_gate_bf16_wfrag_bytes(3, 5, 5, 64) == 10 * 2048
    assert cl.vcg_conv_in_gate_bf16_wfrag_bytes(6, 5, 5, 128) == 2 * 20 * 2048
    assert cl.vcg_conv_in_gate_bf16_wfrag_bytes(6, 3, 3, 512) == 8 * 6 * 2048
    for cin, k, cout in ((4, 3, 64), (3, 7, 64), (3, 4, 64), (6, 5, 96), (3, 5, 1024), (9, 3, 64), (3, 5, 0)):
        assert cl.vcg_conv_in_gate_bf16_wfrag_bytes(cin, k, k, cout) == 0
    assert cl.vcg_conv_in_gate_bf16_wfrag_bytes(3, 5, 3, 64) == 0
    assert cl.vcg_conv9x9_to3_bf16_wfrag_bytes(256) == lib.FINAL9X9_WFRAG_BYTES
    assert cl.vcg_conv9x9_to3_bf16_wfrag_bytes(128) == (2 * 9 * 4 * 64 + 4) * 16
    for cin in (0, 64, 192, 512):
        assert cl.vcg_conv9x9_to3_bf16_wfrag_bytes(cin) == 0


def test_unsupported_shapes_return_error_codes(lib):
    L = lib
    cl = L.load()
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)          # non-null addresses: never dereferenced by the checks below
    for cin, k, cout in ((4, 3, 64), (3, 7, 64), (3, 4, 64), (6, 5, 96), (3, 5, 1024)):
        assert cl.vcg_pack_conv_in_gate_bf16(one, cin, k, k, cout, two, None) == E_UNSUPPORTED
        d = L.ConvDesc(1, cin, 4, 4, cout, 4, 4, k, k, 1, k // 2, k // 2)
        assert cl.vcg_conv_in_gate_bf16_fwd(ctypes.byref(d), one, one, one, one, two, None) == E_UNSUPPORTED
    for d in (L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 3, 3, 2, 1, 1), L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 5, 5, 1, 1, 1), L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 5, 3, 1, 2, 1)):
        assert cl.vcg_conv_in_gate_bf16_fwd(ctypes.byref(d), one, one, one, one, two, None) == E_UNSUPPORTED
    d = L.ConvDesc(1, 3, 4, 4, 64, 4, 4, 3, 3, 1, 1, 1)
    assert cl.vcg_conv_in_gate_bf16_fwd(ctypes.byref(d), one, one, one, two, two, None) == E_UNSUPPORTED          # y is m
    assert cl.vcg_conv_in_gate_bf16_fwd(ctypes.byref(d), one, one, one, None, two, None) == E_NULL
    assert cl.vcg_conv_in_gate_bf16_fwd(ctypes.byref(L.ConvDesc(1, 3, 4, 4, 64, 2, 2, 3, 3, 1, 1, 1)), one, one, one, one, two, None) == E_SHAPE
    for cin in (64, 192, 512):
        assert cl.vcg_pack_conv9x9_to3_bf16(one, cin, two, None) == E_UNSUPPORTED
        d = L.ConvDesc(1, cin, 4, 4, 3, 4, 4, 9, 9, 1, 4, 4)
        assert cl.vcg_conv9x9_to3_bf16_fwd(ctypes.byref(d), one, one, one, 1, two, None) == E_UNSUPPORTED
    for d in (L.ConvDesc(1, 3, 2, 2, 128, 6, 6, 4, 4, 3, 0, 0), L.ConvDesc(1, 3, 2, 2, 128, 4, 4, 5, 5, 2, 0, 0), L.ConvDesc(1, 6, 2, 2, 128, 4, 4, 3, 3, 2, 0, 0),
              L.ConvDesc(1, 3, 2, 2, 128, 4, 4, 3, 3, 2, 1, 1), L.ConvDesc(1, 3, 2, 2, 100, 4, 4, 3, 3, 2, 0, 0), L.ConvDesc(1, 3, 2, 2, 256, 8, 8, 5, 5, 4, 0, 0)):
        assert cl.vcg_input_convt_add_bf16(ctypes.byref(d), one, one, one, two, None) == E_UNSUPPORTED
    assert cl.vcg_input_convt_add_bf16(ctypes.byref(L.ConvDesc(1, 3, 2, 2, 128, 5, 4, 3, 3, 2, 0, 0)), one, one, one, two, None) == E_SHAPE
    assert cl.vcg_input_convt_add_bf16(ctypes.byref(L.ConvDesc(1, 3, 2, 2, 128, 4, 4, 3, 3, 2, 0, 0)), one, one, one, None, None) == E_NULL


def test_engine_refuses_before_touching_a_device_what_it_does_not_serve():
    """the attribute make_upscaler_attention leaves on its model is what the engine keys on (checked without building a model: needs a device)"""
    from upscaler import _infer

    class Fake:
        graph = object()
        attention_generator = {"kernel_size": 5, "filters": 32, "upscale_factor": 4, "res_block_num": 1, "norm": "batch", "channels": 3}

    with pytest.raises(NotImplementedError, match="filters=64"):
        _infer.Bf16AttentionGenerator(Fake())
    with pytest.raises(TypeError):
        _infer.Bf16AttentionGenerator(object())

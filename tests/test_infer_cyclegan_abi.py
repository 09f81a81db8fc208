"""CPU-only ABI checks of head/conv on 64 channels (include/vcg.h: vcg_conv9x9_c64to3_bf16_*), the entry points make_generator_cyclegan's
bf16 inference adds: the size query's value, and null pointers, unsupported descriptors and windows outside the band return their error codes
before anything touches a device."""
import ctypes

import pytest

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from upscaler import _lib
    return _lib


def _desc(L, cin=64, k=9, h=12, w=20, n=1):
    return L.ConvDesc(n, cin, h, w, 3, h, w, k, k, 1, k // 2, k // 2)


def test_size_query(lib):
    cl = lib.load()
    # [9 kx][4 k-steps][64 lanes] fragments of 16 bytes for the one 64-channel chunk + 64 zero bytes
    assert cl.vcg_conv9x9_c64to3_bf16_wfrag_bytes() == (2304 + 4) * 16
    assert cl.vcg_conv9x9_c64to3_bf16_wfrag_bytes() * 2 - 64 == cl.vcg_conv9x9_to3_bf16_wfrag_bytes(128)
    assert cl.vcg_conv9x9_to3_bf16_wfrag_bytes(64) == 0          # the 128 / 256 entry points stay as they were


def test_null_pointers(lib):
    L = lib
    cl = L.load()
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)          # non-null addresses: never dereferenced by the checks below
    assert cl.vcg_pack_conv9x9_c64to3_bf16(None, two, None) == E_NULL
    assert cl.vcg_pack_conv9x9_c64to3_bf16(one, None, None) == E_NULL
    d = ctypes.byref(_desc(L))
    for args in ((None, one, one, one, 1, two), (d, None, one, one, 1, two), (d, one, None, one, 1, two), (d, one, one, one, 1, None)):
        assert cl.vcg_conv9x9_c64to3_bf16_fwd(*args, None) == E_NULL
        a = args[:5] + (L.OUT_F32_NCHW, args[5], 0, 12, 0, 12)
        assert cl.vcg_conv9x9_c64to3_bf16_fwd_window(*a, None) == E_NULL


def test_unsupported_descriptors(lib):
    L = lib
    cl = L.load()
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)
    bad = [_desc(L, cin=cin) for cin in (3, 128, 256)] + [_desc(L, k=k) for k in (3, 5, 7)]
    bad.append(L.ConvDesc(1, 64, 12, 20, 3, 12, 20, 9, 9, 2, 4, 4))          # stride 2
    bad.append(L.ConvDesc(1, 64, 12, 20, 64, 12, 20, 9, 9, 1, 4, 4))         # 64 output channels
    for d in bad:
        assert cl.vcg_conv9x9_c64to3_bf16_fwd(ctypes.byref(d), one, one, one, 1, two, None) == E_UNSUPPORTED
        for kind in (L.OUT_F32_NCHW, L.OUT_U8_NHWC):
            assert cl.vcg_conv9x9_c64to3_bf16_fwd_window(ctypes.byref(d), one, one, one, 1, kind, two, 0, 12, 0, 12, None) == E_UNSUPPORTED
    d = _desc(L)
    for kind in (-1, 2, 7):
        assert cl.vcg_conv9x9_c64to3_bf16_fwd_window(ctypes.byref(d), one, one, one, 1, kind, two, 0, 12, 0, 12, None) == E_UNSUPPORTED
    # an image whose (h + 8) * w * 128 bytes (+ 64 KiB) do not fit 32-bit offsets: this layer has the descriptor form alone
    big = _desc(L, h=4096, w=8192)
    assert (4096 + 8) * 8192 * 128 + 65536 > 0xFFFFFFE0
    assert cl.vcg_conv9x9_c64to3_bf16_fwd(ctypes.byref(big), one, one, one, 1, two, None) == E_UNSUPPORTED
    assert cl.vcg_conv9x9_c64to3_bf16_fwd_window(ctypes.byref(big), one, one, one, 1, L.OUT_U8_NHWC, two, 0, 8, 0, 8, None) == E_UNSUPPORTED
    # output size differing from the input's
    assert cl.vcg_conv9x9_c64to3_bf16_fwd(ctypes.byref(L.ConvDesc(1, 64, 12, 20, 3, 6, 10, 9, 9, 1, 4, 4)), one, one, one, 1, two, None) == E_SHAPE


def test_windows_outside_the_band(lib):
    L = lib
    cl = L.load()
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)
    d = _desc(L)          # 12 rows
    for row0, rows, y_row0, y_h in ((0, 0, 0, 12), (-1, 4, 0, 12), (9, 4, 0, 12), (0, 13, 0, 13), (0, 4, -1, 12), (0, 4, 9, 12), (0, 12, 0, 11),
                                    (2 ** 31 - 1, 2, 0, 12)):
        for kind in (L.OUT_F32_NCHW, L.OUT_U8_NHWC):
            assert cl.vcg_conv9x9_c64to3_bf16_fwd_window(ctypes.byref(d), one, one, one, 1, kind, two, row0, rows, y_row0, y_h, None) == E_SHAPE


def test_engine_refuses_before_touching_a_device_what_it_does_not_serve():
    """the attribute make_generator_cyclegan leaves on its model is what the engine keys on (checked without building a model: needs a device)"""
    from upscaler import _infer

    def fake(**kw):
        class Fake:
            graph = object()
            cyclegan_generator = dict({"filters": 64, "n_downsample": 2, "res_block_num": 1, "upscale_factor": 1, "norm": "instance",
                                       "kernel_size": 3, "channels": 3}, **kw)
        return Fake()

    for kw in ({"filters": 32}, {"n_downsample": 3}, {"channels": 1}, {"kernel_size": 7}, {"upscale_factor": 8}, {"norm": None}):
        with pytest.raises(NotImplementedError, match="filters=64"):
            _infer.Bf16CycleGanGenerator(fake(**kw))
    with pytest.raises(TypeError):
        _infer.Bf16CycleGanGenerator(object())

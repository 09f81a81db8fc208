"""CPU-only ABI checks of the entry points the bf16 VGG19 perceptual loss adds (include/vcg.h: vcg_maxpool2x2_nhwc_bf16_fwd,
vcg_maxpool2x2_relu_nhwc_bf16_bwd, vcg_feature_loss_bf16_ws_bytes, vcg_feature_loss_bf16): they exist, the size query answers, and
null pointers, unserved shapes and a short workspace return their documented codes before anything touches a device or a pointer (the
addresses below are never dereferenced; no GPU is present where this runs).  The model refuses what the kernels do not serve at
construction, and the loss classes' dtype keyword is checked, without a device."""
import ctypes

import pytest

E_NULL, E_SHAPE, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4
ONE, TWO, THREE = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)          # non-null, 16-byte aligned addresses
ODD = ctypes.c_void_p(4096 + 8)                                                                    # not 16-byte aligned


@pytest.fixture(scope="module")
def cl():
    import __graft_entry__ as g
    g.build()
    from upscaler import _lib
    return _lib.load()


def test_entry_points_exist_and_are_declared(cl):
    from upscaler import _lib
    for name in ("vcg_maxpool2x2_nhwc_bf16_fwd", "vcg_maxpool2x2_relu_nhwc_bf16_bwd", "vcg_feature_loss_bf16_ws_bytes", "vcg_feature_loss_bf16"):
        assert name in _lib.SIGNATURES and hasattr(cl, name), name


def test_pool_forward_refusals(cl):
    f = cl.vcg_maxpool2x2_nhwc_bf16_fwd
    assert f(None, TWO, 1, 4, 4, 8, None) == E_NULL and f(ONE, None, 1, 4, 4, 8, None) == E_NULL
    for n, h, w, c in ((0, 4, 4, 8), (1, 1, 4, 8), (1, 4, 1, 8), (1, 0, 4, 8), (1, 4, -2, 8), (1, 4, 4, 0), (-1, 4, 4, 8)):
        assert f(ONE, TWO, n, h, w, c, None) == E_SHAPE, (n, h, w, c)
    for c in (1, 4, 12, 65):
        assert f(ONE, TWO, 1, 4, 4, c, None) == E_UNSUPPORTED, c
    assert f(ODD, TWO, 1, 4, 4, 8, None) == E_UNSUPPORTED and f(ONE, ODD, 1, 4, 4, 8, None) == E_UNSUPPORTED


def test_pool_backward_refusals(cl):
    f = cl.vcg_maxpool2x2_relu_nhwc_bf16_bwd
    assert f(None, TWO, THREE, 1, 4, 4, 8, None) == E_NULL
    assert f(ONE, None, THREE, 1, 4, 4, 8, None) == E_NULL
    assert f(ONE, TWO, None, 1, 4, 4, 8, None) == E_NULL
    for n, h, w, c in ((0, 4, 4, 8), (1, 1, 4, 8), (1, 4, 1, 8), (1, 4, 4, 0), (1, -3, 4, 8)):
        assert f(ONE, TWO, THREE, n, h, w, c, None) == E_SHAPE, (n, h, w, c)
    for c in (3, 12, 100):
        assert f(ONE, TWO, THREE, 1, 5, 7, c, None) == E_UNSUPPORTED, c
    assert f(ONE, TWO, ODD, 1, 4, 4, 8, None) == E_UNSUPPORTED


def test_feature_loss_size_query_and_refusals(cl):
    q, f = cl.vcg_feature_loss_bf16_ws_bytes, cl.vcg_feature_loss_bf16
    assert q(0) == 0
    assert q(1) == q(7) == q(2048) == 16                       # one workgroup: four waves' partials
    assert q(2055) == 16 and q(2056) == 32 and q(8 * 256 * 1024) == q(1 << 40) == 1024 * 16          # the grid stops growing at 1024 workgroups
    call = lambda t=ONE, p=TWO, count=64, kind=0, out=THREE, dz=THREE, ws=ONE, wsn=16: f(t, p, count, kind, 1.0, out, dz, ws, wsn, None)
    for kw in ({"t": None}, {"p": None}, {"out": None}, {"dz": None}, {"ws": None}):
        assert call(**kw) == E_NULL, kw
    assert call(count=0) == E_SHAPE
    assert call(kind=2) == E_UNSUPPORTED and call(kind=-1) == E_UNSUPPORTED
    assert call(t=ODD) == E_UNSUPPORTED and call(p=ODD) == E_UNSUPPORTED and call(dz=ODD) == E_UNSUPPORTED
    assert call(wsn=15) == E_WORKSPACE and call(count=2056, wsn=31) == E_WORKSPACE and call(wsn=0) == E_WORKSPACE


def test_model_and_loss_classes_refuse_without_a_device():
    from upscaler import model as PM
    assert "3 channels" in PM.VGG19Features.VGG_BF16_SERVED and "16" in PM.VGG19Features.VGG_BF16_SERVED
    for shape in ((64, 64, 4), (8, 8, 3), (64, 15, 3), (64, 64, 1)):
        with pytest.raises(NotImplementedError, match="VGG19Features\\(dtype='bf16'\\) serves"):
            PM.VGG19Features(shape, "random", dtype="bf16")
        with pytest.raises(NotImplementedError, match="VGG19Features\\(dtype='bf16'\\) serves"):
            PM.VGG_MSE_LOSS(shape, 0.1, vgg19="random", dtype="bf16")
    with pytest.raises(ValueError):
        PM.VGG19Features((64, 64, 3), "random", dtype="fp16")
    for cls in (PM.VGG_LOSS, PM.VGG_MSE_LOSS, PM.VGG_MAE_LOSS):
        with pytest.raises(ValueError):
            cls((64, 64, 3), vgg19="random", dtype="half")
        with pytest.raises(RuntimeError):                    # as before: no weights named
            cls((64, 64, 3), dtype="bf16")

"""CPU-only checks of what the bf16 tail of make_upscaler_attention adds: every new size query and every refusal of the new entry points
(include/vcg.h) answers before anything touches a device or a pointer, the old entries still refuse the tail's shapes, the index arithmetic
of vcg_input_convt_add_bf16_bwd is the gradient of Conv2DTranspose(s+1, strides s, 'same'), and the new layer classes and the factory's
tail_dtype keyword refuse what they do not serve."""
import ctypes
import inspect

import pytest
import torch

E_NULL, E_SHAPE, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from upscaler import _lib
    return _lib


ONE, TWO, THREE, FOUR, FIVE = (ctypes.c_void_p(v) for v in (256, 512, 768, 1024, 1280))      # non-null addresses the checks never dereference


def _gate(L, cin=6, cout=128, k=3, h=9, w=20, n=2, stride=1, pad=None):
    pad = k // 2 if pad is None else pad
    return L.ConvDesc(n, cin, h, w, cout, h, w, k, k, stride, pad, pad)


def test_up_gate_bwd_refusals(lib):
    L, cl = lib, lib.load()
    call = lambda d, u=ONE, wf=ONE, b=ONE, m=TWO, dy=ONE, dres=THREE, dm=FOUR, da=FIVE: \
        cl.vcg_conv_in_gate_up_bf16_bwd(ctypes.byref(d) if d is not None else None, u, wf, b, m, dy, dres, dm, da, None)
    good = _gate(L)
    for kw in (dict(u=None), dict(wf=None), dict(m=None), dict(dy=None), dict(dm=None), dict(da=None)):
        assert call(good, **kw) == E_NULL
    assert call(None) == E_NULL
    assert call(_gate(L, n=0)) == E_SHAPE
    assert call(L.ConvDesc(2, 6, 9, 20, 128, 8, 20, 3, 3, 1, 1, 1)) == E_SHAPE
    # cin 3 (the residual blocks' entry), cout 256 / 32, k 7 / 4, stride 2, wrong pads, non-square
    for d in (_gate(L, cin=3), _gate(L, cin=3, cout=64), _gate(L, cout=256), _gate(L, cout=32), _gate(L, k=7), _gate(L, k=4), _gate(L, stride=2),
              _gate(L, k=5, pad=1), L.ConvDesc(2, 6, 9, 20, 128, 9, 20, 5, 3, 1, 2, 1)):
        assert call(d) == E_UNSUPPORTED
    assert call(good, dres=FOUR) == E_UNSUPPORTED            # dm == dres
    assert call(good, m=FOUR) == E_UNSUPPORTED               # dm == m
    assert call(good, da=FOUR) == E_UNSUPPORTED              # dm == da
    # the residual blocks' entry still refuses the up-sampling gates' shapes
    old = lambda d: cl.vcg_conv_in_gate_bf16_bwd(ctypes.byref(d), ONE, ONE, ONE, TWO, ONE, THREE, FOUR, FIVE, None)
    assert old(_gate(L, cin=6, cout=64)) == E_UNSUPPORTED and old(_gate(L, cin=3, cout=128)) == E_UNSUPPORTED


def test_up_gate_wgrad_queries_and_refusals(lib):
    L, cl = lib, lib.load()
    q = lambda d: cl.vcg_conv_in_gate_up_bf16_wgrad_ws_bytes(ctypes.byref(d))
    call = lambda d, n, u=ONE, da=ONE, dw=ONE, db=ONE, ws=ONE: cl.vcg_conv_in_gate_up_bf16_wgrad(ctypes.byref(d), u, da, dw, db, ws, n, None)
    for cout in (64, 128):
        for k in (3, 5):
            d = _gate(L, cout=cout, k=k)
            d3 = _gate(L, cin=3, cout=cout, k=k)
            need = q(d)
            # one 3-channel source at a time through the one frame slot: the workspace of the 3-channel entry at the same shape
            assert need > 0 and need == cl.vcg_conv3ch_bf16_wgrad_workspace_bytes(ctypes.byref(d3))
            assert call(d, need - 1) == E_WORKSPACE
            for kw in (dict(u=None), dict(da=None), dict(dw=None), dict(ws=None)):
                assert call(d, need, **kw) == E_NULL
    for d in (_gate(L, w=21), _gate(L, cin=3), _gate(L, cout=256), _gate(L, cout=192), _gate(L, k=9, pad=4), _gate(L, k=4), _gate(L, stride=2),
              _gate(L, k=5, pad=1)):
        assert q(d) == 0
        assert call(d, 1 << 30) == E_UNSUPPORTED
    assert q(_gate(L, n=0)) == 0 and call(_gate(L, n=0), 1 << 30) == E_SHAPE
    assert cl.vcg_conv_in_gate_up_bf16_wgrad_ws_bytes(None) == 0
    # the 3-channel entry still refuses cin 6
    assert cl.vcg_conv3ch_bf16_wgrad_workspace_bytes(ctypes.byref(_gate(L, cin=6, cout=64, k=5))) == 0
    assert cl.vcg_conv3ch_bf16_wgrad(ctypes.byref(_gate(L, cin=6, cout=64, k=5)), ONE, ONE, ONE, ONE, ONE, 1 << 30, None) == E_UNSUPPORTED


def test_final_conv_c128_wgrad_queries_and_refusals(lib):
    L, cl = lib, lib.load()
    desc = lambda cin, w=20: L.ConvDesc(2, cin, 9, w, 3, 9, w, 9, 9, 1, 4, 4)
    d = desc(128)
    need = cl.vcg_conv9x9_c128to3_bf16_wgrad_ws_bytes(ctypes.byref(d))
    # 256 workgroups x 4 row tiles x (11 column tiles x 16 x 64) floats of register dumps + the bf16 [n][h][w][4] copy of dz + alignment slack
    assert need == 256 * 4 * 11 * 16 * 64 * 4 + 2 * 9 * 20 * 8 + 256
    assert cl.vcg_conv9x9_c128to3_bf16_wgrad(ctypes.byref(d), ONE, ONE, ONE, ONE, need - 1, None) == E_WORKSPACE
    for arg in range(4):
        ptrs = [ONE] * 4
        ptrs[arg] = None
        assert cl.vcg_conv9x9_c128to3_bf16_wgrad(ctypes.byref(d), *ptrs, need, None) == E_NULL
    assert cl.vcg_conv9x9_c128to3_bf16_wgrad(ctypes.byref(desc(128, 21)), ONE, ONE, ONE, ONE, 1 << 30, None) == E_UNSUPPORTED
    assert cl.vcg_conv9x9_c128to3_bf16_wgrad(ctypes.byref(L.ConvDesc(2, 128, 9, 20, 3, 9, 20, 5, 5, 1, 2, 2)), ONE, ONE, ONE, ONE, 1 << 30, None) == E_UNSUPPORTED
    assert cl.vcg_conv9x9_c128to3_bf16_wgrad(ctypes.byref(L.ConvDesc(0, 128, 9, 20, 3, 9, 20, 9, 9, 1, 4, 4)), ONE, ONE, ONE, ONE, 1 << 30, None) == E_SHAPE
    for cin in (64, 256, 32):
        assert cl.vcg_conv9x9_c128to3_bf16_wgrad_ws_bytes(ctypes.byref(desc(cin))) == 0
        assert cl.vcg_conv9x9_c128to3_bf16_wgrad(ctypes.byref(desc(cin)), ONE, ONE, ONE, ONE, 1 << 30, None) == E_UNSUPPORTED
    # the 64 / 256 entry still refuses 128
    assert cl.vcg_conv9x9_to3_bf16_wgrad_workspace_bytes(ctypes.byref(d)) == 0
    assert cl.vcg_conv9x9_to3_bf16_wgrad(ctypes.byref(d), ONE, ONE, ONE, ONE, 1 << 30, None) == E_UNSUPPORTED


def _add_input(L, s=4, cout=128, h=5, w=7, n=2, cin=3, k=None, oh=None, pad=0):
    k = s + 1 if k is None else k
    return L.ConvDesc(n, cin, h, w, cout, s * h if oh is None else oh, s * w, k, k, s, pad, pad)


def test_add_input_entries_queries_and_refusals(lib):
    L, cl = lib, lib.load()
    to = lambda d, x=ONE, w=ONE, b=ONE, yi=TWO, yo=THREE: cl.vcg_input_convt_add_bf16_to(ctypes.byref(d) if d is not None else None, x, w, b, yi, yo, None)
    q = lambda d: cl.vcg_input_convt_add_bf16_bwd_ws_bytes(ctypes.byref(d))
    bwd = lambda d, n, x=ONE, dy=ONE, ya=TWO, dz=THREE, dw=FOUR, ba=FIVE, bc=FIVE, ws=ONE: \
        cl.vcg_input_convt_add_bf16_bwd(ctypes.byref(d) if d is not None else None, x, dy, ya, 0.2, dz, dw, ba, bc, ws, n, None)
    bad_shape = (_add_input(L, n=0), _add_input(L, oh=19))
    unsupported = (_add_input(L, s=3), _add_input(L, s=8), _add_input(L, cin=6), _add_input(L, k=4), _add_input(L, pad=1), _add_input(L, cout=12))
    for kw in (dict(x=None), dict(w=None), dict(yi=None), dict(yo=None)):
        assert to(_add_input(L), **kw) == E_NULL
    assert to(None) == E_NULL
    for d in bad_shape:
        assert to(d) == E_SHAPE and q(d) == 0 and bwd(d, 1 << 30) == E_SHAPE
    for d in unsupported:
        assert to(d) == E_UNSUPPORTED and q(d) == 0 and bwd(d, 1 << 30) == E_UNSUPPORTED
    # the workspace: [workgroups x teams][4 taps x 8 channels x 3 + 2 x 8 sums][units], units = s^2 cout / 8, teams = 256 / units
    for s, cout, h, w, n in ((2, 128, 5, 7, 2), (4, 128, 5, 7, 2), (4, 64, 9, 12, 1), (2, 64, 64, 64, 8)):
        d = _add_input(L, s=s, cout=cout, h=h, w=w, n=n)
        units = s * s * cout // 8
        tiles = n * -(-h // 4) * -(-w // 8)
        need = q(d)
        assert need == min(tiles, 512) * (256 // units) * 112 * units * 4
        assert bwd(d, need - 1) == E_WORKSPACE
        for kw in (dict(x=None), dict(dy=None), dict(ya=None), dict(dz=None), dict(dw=None), dict(ws=None)):
            assert bwd(d, need, **kw) == E_NULL
        assert bwd(d, need, dz=ONE) == E_UNSUPPORTED             # dz == dY
        assert bwd(d, need, dz=TWO) == E_UNSUPPORTED             # dz == y_act
    # more than 256 units: the forward serves the shape, the backward does not
    wide = _add_input(L, s=4, cout=136)
    assert q(wide) == 0 and bwd(wide, 1 << 30) == E_UNSUPPORTED
    assert bwd(None, 0) == E_NULL and cl.vcg_input_convt_add_bf16_bwd_ws_bytes(None) == 0


def _add_input_dw_by_phases(a, dy, s):
    """dw (s+1, s+1, cout, 3) accumulated as vcg_input_convt_add_bf16_bwd accumulates it: output pixel o = s i + t feeds tap t of input pixel
    i and, where t == 0, tap s of input pixel i - 1 (zero outside the image) -- per (phase, slot), then placed as its reduction places them"""
    n, _, h, w = a.shape
    cout = dy.shape[1]
    ap = torch.zeros(n, 3, h + 1, w + 1, dtype=a.dtype)
    ap[:, :, 1:, 1:] = a                                          # the halo: row above, column to the left
    dw = torch.zeros(s + 1, s + 1, cout, 3, dtype=a.dtype)
    for ty in range(s):
        for tx in range(s):
            g = dy[:, :, ty::s, tx::s]                            # [n, cout, h, w]: the output pixels of this phase
            for slot in range(4):
                up, left = slot & 1, slot >> 1
                if (up and ty) or (left and tx):
                    continue
                src = ap[:, :, 1 - up:1 - up + h, 1 - left:1 - left + w]
                dw[s if up else ty, s if left else tx] += torch.einsum("nchw,nihw->ci", g, src)
    return dw


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("h,w", [(3, 5), (4, 4)])
def test_add_input_bwd_index_arithmetic(s, h, w):
    from oracle import keras_ops as K
    g = torch.Generator().manual_seed(10 * s + h)
    a = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64)
    dy = torch.randn(2, 8, s * h, s * w, generator=g, dtype=torch.float64)
    wr = torch.zeros(s + 1, s + 1, 8, 3, dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad((K.conv2d_transpose_same(a, wr, None, s) * dy).sum(), [wr])
    got = _add_input_dw_by_phases(a, dy, s)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float(ref[s, s].abs().max()) > 0 and float(ref[s, 0].abs().max()) > 0


def test_new_layers_refuse_what_they_do_not_serve():
    from upscaler import _engine as E
    for args in ((3, 64, 3), (6, 256, 3), (6, 32, 5), (6, 128, 7)):
        with pytest.raises(NotImplementedError):
            E.UpGateConvBf16("g", *args)
    for args in ((64, 128, 3), (64, 128, 5), (128, 128, 3), (128, 128, 5)):
        E.UpConvTBf16("t", *args)
    for args in ((256, 128, 3), (64, 64, 3), (64, 256, 5), (128, 128, 4)):
        with pytest.raises(NotImplementedError):
            E.UpConvTBf16("t", *args)
    with pytest.raises(NotImplementedError):
        E.UpConvTBf16("t", 64, 128, 3, act=0)
    for args in ((6, 128, 2), (3, 128, 3), (3, 12, 2), (3, 136, 4)):
        with pytest.raises(NotImplementedError):
            E.ToAddInputBf16("a", *args)
    for args in ((256, 3, 9), (64, 3, 9), (128, 1, 9), (128, 3, 5)):
        with pytest.raises(NotImplementedError):
            E.FinalConv9x9C128Bf16("f", *args)
    for cout in (64, 128):
        for k in (3, 5):
            E.UpGateConvBf16("g", 6, cout, k)
    E.ToAddInputBf16("a", 3, 128, 2)
    E.ToAddInputBf16("a", 3, 128, 4)
    E.FinalConv9x9C128Bf16("f", 128, 3, 9)
    # the classes they stand next to refuse what they refused
    with pytest.raises(NotImplementedError):
        E.ConvTBf16("t", 128, 64, 5)
    with pytest.raises(NotImplementedError):
        E.GateConvBf16("g", 6, 64, 3)
    with pytest.raises(NotImplementedError):
        E.GateConvBf16("g", 3, 128, 3)
    assert E.FinalConv9x9Bf16.WGRAD == E.HeadConv9x9C64Bf16.WGRAD == "vcg_conv9x9_to3_bf16_wgrad"


def test_tail_dtype_keyword_and_refusals_before_a_device_is_needed():
    from upscaler import _graph
    sig = inspect.signature(_graph.make_upscaler_attention)
    assert sig.parameters["tail_dtype"].default == "fp32" and sig.parameters["trunk_dtype"].default == "fp32"
    assert "filters=64" in _graph.ATTENTION_BF16_SERVED and "bf16+tail" in _graph.ATTENTION_BF16_SERVED and "tail_dtype='bf16'" in _graph.ATTENTION_BF16_SERVED
    for bad in ("fp16", "bf16+tail", None):
        with pytest.raises(ValueError):
            _graph.make_upscaler_attention((32, 48, 3), res_block_num=1, trunk_dtype="bf16", tail_dtype=bad)
    for trunk in ("fp32",):
        with pytest.raises(NotImplementedError, match="filters=64"):
            _graph.make_upscaler_attention((32, 48, 3), res_block_num=1, trunk_dtype=trunk, tail_dtype="bf16")
    with pytest.raises(NotImplementedError, match="filters=64"):
        _graph.make_upscaler_attention((32, 48, 3), res_block_num=1, tail_dtype="bf16")          # the default trunk is fp32
    for kw in (dict(filters=32), dict(norm="instance"), dict(kernel_size=7), dict(upscale_factor=8)):
        with pytest.raises(NotImplementedError, match="filters=64"):
            _graph.make_upscaler_attention((32, 48, 3), res_block_num=1, trunk_dtype="bf16", tail_dtype="bf16", **kw)
    with pytest.raises(NotImplementedError, match="filters=64"):
        _graph.make_upscaler_attention((32, 48, 4), res_block_num=1, trunk_dtype="bf16", tail_dtype="bf16")
    with pytest.raises(NotImplementedError, match="bf16\\+tail"):
        _graph.make_upscaler_attention((32, 48, 3), res_block_num=1, trunk_dtype="bf16+tail", tail_dtype="bf16")

"""CPU-only ABI checks of the entry points bf16 inference of make_upscaler_incep_resnet adds (include/vcg.h: vcg_incep_padded_channels,
vcg_incep_frag_bf16_bytes, vcg_pack_incep_frag_bf16, vcg_incep_fold, vcg_incep_head_bf16_fwd, vcg_conv2d_nhwc_bf16_fwd_epilogue,
vcg_incep_join_bf16_fwd): the size queries' values, and null pointers and unserved descriptors return their documented codes before
anything touches a device; the engine refuses unserved configurations the same way."""
import ctypes

import pytest

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
ONE, TWO = ctypes.c_void_p(4096), ctypes.c_void_p(8192)          # non-null addresses: never dereferenced by the checks below


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from upscaler import _lib
    return _lib


def test_size_queries(lib):
    cl = lib.load()
    assert [cl.vcg_incep_padded_channels(c) for c in (1, 19, 25, 32, 33, 48, 64, 0, -5)] == [32, 32, 32, 32, 64, 64, 64, 0, 0]
    assert cl.vcg_incep_frag_bf16_bytes(1, 64, 19) == 64 * 32 * 2
    assert cl.vcg_incep_frag_bf16_bytes(7, 19, 25) == 7 * 32 * 32 * 2
    assert cl.vcg_incep_frag_bf16_bytes(9, 32, 48) == 9 * 32 * 64 * 2
    assert cl.vcg_incep_frag_bf16_bytes(25, 48, 64) == 25 * 64 * 64 * 2
    # an unpadded layer's fragments are the generic kernels'
    assert cl.vcg_incep_frag_bf16_bytes(9, 64, 64) == cl.vcg_conv_frag_bf16_bytes(9, 64, 64)
    assert cl.vcg_incep_frag_bf16_bytes(0, 64, 64) == 0 and cl.vcg_incep_frag_bf16_bytes(9, -1, 64) == 0


def test_pack_and_fold_refusals(lib):
    cl = lib.load()
    assert cl.vcg_pack_incep_frag_bf16(None, 1, 64, 32, 0, 64, TWO, None) == E_NULL
    assert cl.vcg_pack_incep_frag_bf16(ONE, 1, 64, 32, 0, 64, None, None) == E_NULL
    for taps, cin_total, cout, k0, kcount in ((0, 64, 32, 0, 64), (1, 64, 0, 0, 64), (1, 64, 32, -1, 32), (1, 64, 32, 33, 32), (1, 64, 32, 0, 0)):
        assert cl.vcg_pack_incep_frag_bf16(ONE, taps, cin_total, cout, k0, kcount, TWO, None) == E_SHAPE
    for taps, cin_total, cout, k0, kcount in ((26, 64, 32, 0, 64), (1, 64, 65, 0, 64), (1, 128, 64, 0, 128)):
        assert cl.vcg_pack_incep_frag_bf16(ONE, taps, cin_total, cout, k0, kcount, TWO, None) == E_UNSUPPORTED
    fold = lambda bias, mean, var, alpha, c, sc, sh, ao: cl.vcg_incep_fold(bias, mean, var, ONE, ONE, alpha, c, 1e-3, sc, sh, ao, None)
    assert fold(ONE, ONE, ONE, ONE, 19, None, TWO, TWO) == E_NULL
    assert fold(ONE, ONE, ONE, ONE, 19, TWO, None, TWO) == E_NULL
    assert fold(ONE, ONE, None, ONE, 19, TWO, TWO, TWO) == E_NULL          # moving_mean without moving_var
    assert fold(ONE, None, ONE, ONE, 19, TWO, TWO, TWO) == E_NULL
    assert fold(ONE, ONE, ONE, ONE, 19, TWO, TWO, None) == E_NULL          # alpha without alpha_out
    assert fold(ONE, ONE, ONE, None, 19, TWO, TWO, TWO) == E_NULL
    assert fold(ONE, ONE, ONE, ONE, 0, TWO, TWO, TWO) == E_SHAPE
    assert fold(ONE, ONE, ONE, ONE, 65, TWO, TWO, TWO) == E_UNSUPPORTED


def _paths(L, n, **null):
    arr = (L.IncepHeadPath * n)()
    for i in range(n):
        arr[i] = L.IncepHeadPath(*[None if f in null else 4096 for f, _ in L.IncepHeadPath._fields_])
    return arr


def test_head_refusals(lib):
    L = lib
    cl = L.load()
    desc = lambda n=1, h=4, w=4, cin=64, npaths=3, cout=(32, 32, 32): L.IncepHeadDesc(n, h, w, cin, npaths, (ctypes.c_int32 * 3)(*cout))
    call = lambda d, m, p: cl.vcg_incep_head_bf16_fwd(ctypes.byref(d) if d is not None else None, m, p, None)
    assert call(None, ONE, _paths(L, 3)) == E_NULL
    assert call(desc(), None, _paths(L, 3)) == E_NULL
    assert call(desc(), ONE, None) == E_NULL
    for field, _ in L.IncepHeadPath._fields_:
        if field != "out_alpha":          # optional: no activation
            assert call(desc(), ONE, _paths(L, 3, **{field: 1})) == E_NULL, field
    for d in (desc(n=0), desc(h=0), desc(w=-1), desc(cout=(32, 0, 32)), desc(n=1, h=8192, w=4096)):          # 2^25 pixels x 128 bytes = 4 GiB
        assert call(d, ONE, _paths(L, 3)) == E_SHAPE
    for d in (desc(cin=32), desc(cin=128), desc(npaths=0), desc(npaths=4), desc(cout=(32, 33, 32)), desc(cout=(64, 32, 32))):
        assert call(d, ONE, _paths(L, 3)) == E_UNSUPPORTED


def test_epilogue_conv_refusals(lib):
    L = lib
    cl = L.load()
    desc = lambda cin=32, cout=48, kh=3, kw=3, stride=1, h=6, w=6, oh=None, ow=None, pt=None, pl=None: L.ConvDesc(
        1, cin, h, w, cout, h if oh is None else oh, w if ow is None else ow, kh, kw, stride, kh // 2 if pt is None else pt, kw // 2 if pl is None else pl)
    epi = lambda scale=4096, shift=4096, act=L.ACT_PRELU, alpha=4096, res=None, mode=0: L.EpilogueBf16(scale, shift, act, 0.0, alpha, res, None, mode)
    call = lambda d, x, wf, y, ep: cl.vcg_conv2d_nhwc_bf16_fwd_epilogue(ctypes.byref(d) if d is not None else None, x, wf, y,
                                                                       ctypes.byref(ep) if ep is not None else None, None)
    assert call(None, ONE, ONE, TWO, epi()) == E_NULL and call(desc(), ONE, ONE, TWO, None) == E_NULL
    assert call(desc(), None, ONE, TWO, epi()) == E_NULL and call(desc(), ONE, None, TWO, epi()) == E_NULL
    assert call(desc(), ONE, ONE, None, epi()) == E_NULL
    assert call(desc(), ONE, ONE, TWO, epi(scale=None)) == E_NULL and call(desc(), ONE, ONE, TWO, epi(shift=None)) == E_NULL
    assert call(desc(), ONE, ONE, TWO, epi(alpha=None)) == E_NULL          # PReLU without its slopes
    for d in (desc(h=0), desc(cin=0), desc(oh=3), desc(ow=12), desc(pt=0), desc(pl=2), desc(kh=1, kw=7, cin=19, cout=25, pl=0)):
        assert call(d, ONE, ONE, TWO, epi()) == E_SHAPE
    bad = [desc(stride=2), desc(kh=7, kw=7), desc(kh=4, kw=4), desc(kh=1, kw=1), desc(kh=3, kw=5), desc(kh=1, kw=9), desc(cin=65), desc(cout=96),
           desc(kh=1, kw=7, cin=48, cout=32), desc(kh=7, kw=1, cin=25, cout=48)]
    for d in bad:
        assert call(d, ONE, ONE, TWO, epi()) == E_UNSUPPORTED
    assert call(desc(), ONE, ONE, TWO, epi(act=L.ACT_LRELU)) == E_UNSUPPORTED
    assert call(desc(), ONE, ONE, TWO, epi(act=L.ACT_TANH)) == E_UNSUPPORTED
    assert call(desc(), ONE, ONE, TWO, epi(res=4096)) == E_UNSUPPORTED
    assert call(desc(), ONE, ONE, TWO, epi(mode=L.STATS_BATCH)) == E_UNSUPPORTED


def test_join_refusals(lib):
    L = lib
    cl = L.load()
    desc = lambda n=1, h=4, w=4, cout=64, nsrc=3, cin=(32, 32, 64): L.IncepJoinDesc(n, h, w, cout, nsrc, (ctypes.c_int32 * 3)(*cin))
    ptrs = lambda *v: (ctypes.c_void_p * 3)(*v)
    z, wf = ptrs(4096, 4096, 4096), ptrs(4096, 4096, 4096)
    call = lambda d, z_, wf_, bias, m, y: cl.vcg_incep_join_bf16_fwd(ctypes.byref(d) if d is not None else None, z_, wf_, bias, m, y, None)
    assert call(None, z, wf, ONE, ONE, TWO) == E_NULL
    assert call(desc(), None, wf, ONE, ONE, TWO) == E_NULL and call(desc(), z, None, ONE, ONE, TWO) == E_NULL
    assert call(desc(), z, wf, None, ONE, TWO) == E_NULL and call(desc(), z, wf, ONE, None, TWO) == E_NULL
    assert call(desc(), z, wf, ONE, ONE, None) == E_NULL
    assert call(desc(), ptrs(4096, None, 4096), wf, ONE, ONE, TWO) == E_NULL
    assert call(desc(), z, ptrs(4096, 4096, None), ONE, ONE, TWO) == E_NULL
    for d in (desc(n=0), desc(w=0), desc(cin=(32, 0, 64)), desc(h=8192, w=4096)):
        assert call(d, z, wf, ONE, ONE, TWO) == E_SHAPE
    for d in (desc(cout=32), desc(nsrc=0), desc(nsrc=4), desc(cin=(32, 32, 65))):
        assert call(d, z, wf, ONE, ONE, TWO) == E_UNSUPPORTED
    assert call(desc(), ptrs(4096, 8192, 4096), wf, ONE, ONE, TWO) == E_UNSUPPORTED          # y is one of the sources


def test_engine_refuses_before_touching_a_device_what_it_does_not_serve():
    """the attribute make_upscaler_incep_resnet leaves on its model is what the engine keys on (checked without building a model: needs a device)"""
    from upscaler import _infer

    def fake(**kw):
        class Fake:
            graph = object()
            incep_resnet_generator = dict({"filters": 64, "upscale_factor": 4, "channels": 3, "a_block_type": "3path", "a_block_num": 1,
                                           "a_block_kernel": 3, "b_block_type": "2path", "b_block_num": 1, "b_block_kernel": 7,
                                           "c_block_type": "2path", "c_block_num": 1, "c_block_kernel": 3}, **kw)
        return Fake()

    for kw in ({"filters": 32}, {"channels": 1}, {"upscale_factor": 1}, {"upscale_factor": 3}, {"a_block_kernel": 7}, {"b_block_kernel": 9},
               {"c_block_kernel": 7}, {"a_block_type": "4path"}, {"b_block_type": "3path"}):          # (3-path with the 2-path default kernel 7)
        with pytest.raises(NotImplementedError, match="filters=64"):
            _infer.Bf16IncepResnetGenerator(fake(**kw))
    assert "filters=64" in _infer.Bf16IncepResnetGenerator.SERVED
    with pytest.raises(TypeError):
        _infer.Bf16IncepResnetGenerator(object())

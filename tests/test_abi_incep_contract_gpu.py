"""The memory contract of the entry points bf16 inference of make_upscaler_incep_resnet adds (include/vcg.h: vcg_pack_incep_frag_bf16,
vcg_incep_fold, vcg_incep_head_bf16_fwd, vcg_conv2d_nhwc_bf16_fwd_epilogue, vcg_incep_join_bf16_fwd), as
tests/test_abi_cyclegan_contract_gpu.py checks head/conv's: every buffer inside a guarded arena (tests/_arena.py) of exactly its stated size
-- tensors [n][h][w][padded channels] bf16, packed kernels of exactly vcg_incep_frag_bf16_bytes, epilogue vectors of exactly
vcg_incep_padded_channels floats, no slack anywhere.  After the calls the guards are intact, the inputs hold their bytes, every byte of
every output is written (no NaN of the prefill survives, padded channels are zero) and the values match the fp64 reference.  None of the
entry points takes a workspace.  Refused calls write nothing."""
import ctypes

import pytest
import torch

import _arena as A
import _incep_kernel_calls as C
from conftest import rel_err

pytestmark = pytest.mark.gpu
E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3


@pytest.mark.parametrize("btype,k,shape", [("3path", 3, (2, 5, 7)), ("3path", 5, (1, 9, 33)), ("2path", 7, (1, 9, 33)), ("2path", 3, (3, 1, 1))])
def test_block_in_exact_size_arenas(rt, btype, k, shape):
    n, h, w = shape
    res, dev = C.run_block(rt, btype, k, n, h, w, seed=1)          # run_block ends with Device.check(): guards and input bytes
    sizes = {a.name: a.nbytes for a in dev.outputs}
    assert sizes["y join"] == n * h * w * 64 * 2 and sizes["y a/1"] == n * h * w * 32 * 2
    if btype == "3path":
        assert sizes["y c/2"] == n * h * w * 64 * 2 and sizes["y b/2"] == n * h * w * 32 * 2          # 48 channels are stored on 64
    else:
        assert sizes["y b/1"] == sizes["y b/2"] == sizes["y b/3"] == n * h * w * 32 * 2                # 19, 25 and 32 on 32
    assert sizes["scale"] in (128, 256) and sizes["wfrag"] > 0
    for a in dev.outputs:
        assert not a.untouched(), a.name
        if a.dtype != torch.uint8:
            assert not torch.isnan(a.view(a.dtype).float()).any(), a.name
    for what, got, ref in res:
        assert rel_err(got, ref) < C.TOL_BF16 and C.ulp_scaled(got, ref) < 1.0, what


def test_join_in_place_on_the_block_input(rt):
    """y may be m (documented): the same bytes as with a separate output"""
    from upscaler import _lib as L
    n, h, w = 1, 9, 33
    wt = C.block_weights("2path", 3, 4)
    g = torch.Generator().manual_seed(9)
    m = C.to_nhwc_bf16(torch.randn(n, 64, h, w, generator=g))
    za, zb = (C.to_nhwc_bf16(torch.randn(n, 32, h, w, generator=g)) for _ in range(2))
    dev = C.Device(rt)
    ma, srcs = dev.put(m, "m"), [dev.put(za, "za"), dev.put(zb, "zb")]
    y = C.run_join(dev, wt, "2path", 3, srcs, ma, n, h, w)
    dev.check()
    io = A.output_arena((n, h, w, 64), torch.bfloat16, rt.device, name="m = y")
    io.payload.copy_(ma.payload)
    name = C.block_spec("2path", 3)[0]
    wfs = [dev.pack(wt[name + "/final/1x1/kernel"], k0, 32) for k0 in (0, 32)]
    jd = L.IncepJoinDesc(n, h, w, 64, 2, (ctypes.c_int32 * 3)(32, 32, 0))
    z = (ctypes.c_void_p * 2)(*[a.ptr for a in srcs])
    wf = (ctypes.c_void_p * 2)(*[a.ptr for a in wfs])
    bias = dev.put(wt[name + "/final/1x1/bias"], "bias")
    assert rt.lib.vcg_incep_join_bf16_fwd(ctypes.byref(jd), z, wf, bias.ptr, io.ptr, io.ptr, rt.stream) == 0
    io.check()
    assert torch.equal(io.payload.cpu(), y.payload.cpu())


def test_refusals_leave_the_outputs_untouched(rt):
    from upscaler import _lib as L
    lib = rt.lib
    one = A.input_arena(torch.zeros(65536), rt.device, name="operand")
    out = A.output_arena((65536,), torch.float32, rt.device, name="out")
    # pack / fold
    assert lib.vcg_pack_incep_frag_bf16(one.ptr, 26, 64, 32, 0, 64, out.ptr, rt.stream) == E_UNSUPPORTED
    assert lib.vcg_pack_incep_frag_bf16(one.ptr, 1, 64, 32, 40, 32, out.ptr, rt.stream) == E_SHAPE
    assert lib.vcg_incep_fold(one.ptr, one.ptr, one.ptr, None, None, None, 65, 1e-3, out.ptr, out.ptr, None, rt.stream) == E_UNSUPPORTED
    assert lib.vcg_incep_fold(one.ptr, one.ptr, None, None, None, None, 32, 1e-3, out.ptr, out.ptr, None, rt.stream) == E_NULL
    # head
    paths = (L.IncepHeadPath * 3)(*[L.IncepHeadPath(one.ptr, one.ptr, one.ptr, one.ptr, one.ptr, one.ptr, None, out.ptr) for _ in range(3)])
    for d in (L.IncepHeadDesc(1, 4, 4, 32, 3, (ctypes.c_int32 * 3)(32, 32, 32)), L.IncepHeadDesc(1, 4, 4, 64, 4, (ctypes.c_int32 * 3)(32, 32, 32)),
              L.IncepHeadDesc(1, 4, 4, 64, 3, (ctypes.c_int32 * 3)(32, 48, 32))):
        assert lib.vcg_incep_head_bf16_fwd(ctypes.byref(d), one.ptr, paths, rt.stream) == E_UNSUPPORTED
    assert lib.vcg_incep_head_bf16_fwd(ctypes.byref(L.IncepHeadDesc(0, 4, 4, 64, 3, (ctypes.c_int32 * 3)(32, 32, 32))), one.ptr, paths, rt.stream) == E_SHAPE
    # the layers between head and join
    ep = L.EpilogueBf16(one.ptr, one.ptr, L.ACT_PRELU, 0.0, one.ptr, None, None, 0)
    for d in (L.ConvDesc(1, 32, 4, 4, 32, 4, 4, 7, 7, 1, 3, 3), L.ConvDesc(1, 32, 4, 4, 32, 2, 2, 3, 3, 2, 1, 1), L.ConvDesc(1, 128, 4, 4, 64, 4, 4, 3, 3, 1, 1, 1),
              L.ConvDesc(1, 64, 4, 4, 64, 4, 4, 1, 7, 1, 0, 3)):
        rc = lib.vcg_conv2d_nhwc_bf16_fwd_epilogue(ctypes.byref(d), one.ptr, one.ptr, out.ptr, ctypes.byref(ep), rt.stream)
        assert rc in (E_UNSUPPORTED, E_SHAPE), rc
    ep_res = L.EpilogueBf16(one.ptr, one.ptr, L.ACT_NONE, 0.0, None, one.ptr, None, 0)
    d = L.ConvDesc(1, 32, 4, 4, 32, 4, 4, 3, 3, 1, 1, 1)
    assert lib.vcg_conv2d_nhwc_bf16_fwd_epilogue(ctypes.byref(d), one.ptr, one.ptr, out.ptr, ctypes.byref(ep_res), rt.stream) == E_UNSUPPORTED
    # join
    z = (ctypes.c_void_p * 3)(one.ptr, one.ptr, one.ptr)
    for jd in (L.IncepJoinDesc(1, 4, 4, 32, 3, (ctypes.c_int32 * 3)(32, 32, 64)), L.IncepJoinDesc(1, 4, 4, 64, 3, (ctypes.c_int32 * 3)(32, 32, 128))):
        assert lib.vcg_incep_join_bf16_fwd(ctypes.byref(jd), z, z, one.ptr, one.ptr, out.ptr, rt.stream) == E_UNSUPPORTED
    jd = L.IncepJoinDesc(1, 4, 4, 64, 2, (ctypes.c_int32 * 3)(32, 32, 0))
    zy = (ctypes.c_void_p * 2)(one.ptr, out.ptr)
    assert lib.vcg_incep_join_bf16_fwd(ctypes.byref(jd), zy, z, one.ptr, one.ptr, out.ptr, rt.stream) == E_UNSUPPORTED
    torch.cuda.current_stream().synchronize()
    one.check()
    out.check()
    assert out.untouched()

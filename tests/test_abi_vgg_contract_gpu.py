"""The memory contract of the entry points the bf16 VGG19 perceptual loss adds (include/vcg.h: vcg_maxpool2x2_nhwc_bf16_fwd,
vcg_maxpool2x2_relu_nhwc_bf16_bwd, vcg_feature_loss_bf16), as tests/test_abi_incep_contract_gpu.py checks the inception entries': every
buffer inside a guarded arena (tests/_arena.py) of exactly its stated size, the loss kernel's workspace of exactly
vcg_feature_loss_bf16_ws_bytes, no slack anywhere.  After the calls the guards are intact, the inputs hold their bytes, every byte
of every output is written (no NaN of the prefill survives) and the values are the reference's.  Refused calls write nothing."""
import pytest
import torch

import _arena as A
import _vgg_bf16_emulation as V

pytestmark = pytest.mark.gpu
E_NULL, E_SHAPE, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4


def _bf16_of(arena):
    return arena.view(torch.bfloat16, arena.shape).cpu()


@pytest.mark.parametrize("n,h,w,c", [(2, 5, 7, 8), (1, 16, 18, 24), (1, 2, 2, 8)])
def test_pooling_in_exact_size_arenas(rt, n, h, w, c):
    g = torch.Generator().manual_seed(n * h + w)
    x = torch.randn(n, h, w, c, generator=g).to(torch.bfloat16)
    dy = torch.randn(n, h // 2, w // 2, c, generator=g).to(torch.bfloat16)
    xa, dya = A.input_arena(x, rt.device, "x"), A.input_arena(dy, rt.device, "dy")
    ya = A.output_arena((n, h // 2, w // 2, c), torch.bfloat16, rt.device, "y")
    dza = A.output_arena((n, h, w, c), torch.bfloat16, rt.device, "dz")
    assert ya.nbytes == n * (h // 2) * (w // 2) * c * 2 and dza.nbytes == n * h * w * c * 2
    assert rt.lib.vcg_maxpool2x2_nhwc_bf16_fwd(xa.ptr, ya.ptr, n, h, w, c, rt.stream) == 0
    assert rt.lib.vcg_maxpool2x2_relu_nhwc_bf16_bwd(xa.ptr, dya.ptr, dza.ptr, n, h, w, c, rt.stream) == 0
    for a in (xa, dya, ya, dza):
        a.check()
    assert torch.equal(_bf16_of(xa).view(torch.int16), x.view(torch.int16)) and torch.equal(_bf16_of(dya).view(torch.int16), dy.view(torch.int16))
    y, dz = _bf16_of(ya), _bf16_of(dza)
    assert not torch.isnan(y.float()).any() and not torch.isnan(dz.float()).any()          # every element written, nothing read from a guard
    xr = x.float().permute(0, 3, 1, 2).contiguous()
    yr, idx = torch.nn.functional.max_pool2d(xr, 2, 2, return_indices=True)
    dzr = torch.nn.functional.max_unpool2d(dy.float().permute(0, 3, 1, 2).contiguous(), idx, 2, 2, output_size=(h, w)) * (xr > 0)
    assert torch.equal(y.float(), yr.permute(0, 2, 3, 1)) and torch.equal(dz.float(), dzr.permute(0, 2, 3, 1))


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("count", [3, 2048 + 8, 8 * 256 * 5 + 1])
def test_feature_loss_in_exact_size_arenas(rt, kind, count):
    g = torch.Generator().manual_seed(count)
    t = torch.relu(torch.randn(count, generator=g)).to(torch.bfloat16)
    p = (torch.relu(torch.randn(count, generator=g)) + 0.125).to(torch.bfloat16)
    p[1::5] = 0.0
    ta, pa = A.input_arena(t, rt.device, "f_true"), A.input_arena(p, rt.device, "f_pred")
    out = A.output_arena((1,), torch.float32, rt.device, "loss")
    dza = A.output_arena((count,), torch.bfloat16, rt.device, "dz_pred")
    need = rt.lib.vcg_feature_loss_bf16_ws_bytes(count)
    assert need == 16 * min(max((count // 8 + 255) // 256, 1), 1024)
    ws = A.workspace_arena(need, rt.device, fill=A.NAN_BYTE)          # stale partials would show as NaN in the value
    assert rt.lib.vcg_feature_loss_bf16(ta.ptr, pa.ptr, count, kind, 2.0, out.ptr, dza.ptr, ws.ptr, need, rt.stream) == 0
    for a in (ta, pa, out, dza, ws):
        a.check()
    assert torch.equal(_bf16_of(ta).view(torch.int16), t.view(torch.int16)) and torch.equal(_bf16_of(pa).view(torch.int16), p.view(torch.int16))
    name = "mse" if kind == 0 else "mae"
    val, dz = float(out.view(torch.float32)[0].item()), _bf16_of(dza).double()
    ref, gref = V.loss_value(t, p, name), V.loss_grad(t, p, name, 2.0, round_grads=False)
    assert not torch.isnan(dz).any()
    assert abs(val - ref) <= 1e-5 * ref
    assert bool(((dz - gref).abs() <= 1.01 * 2.0 ** -8 * gref.abs()).all())
    # one byte short: refused, nothing written
    out2 = A.output_arena((1,), torch.float32, rt.device, "loss (refused)")
    dz2 = A.output_arena((count,), torch.bfloat16, rt.device, "dz_pred (refused)")
    assert rt.lib.vcg_feature_loss_bf16(ta.ptr, pa.ptr, count, kind, 2.0, out2.ptr, dz2.ptr, ws.ptr, need - 1, rt.stream) == E_WORKSPACE
    torch.cuda.current_stream().synchronize()
    assert out2.untouched() and dz2.untouched()


def test_refusals_leave_the_outputs_untouched(rt):
    lib = rt.lib
    one = A.input_arena(torch.zeros(4096, dtype=torch.bfloat16), rt.device, name="operand")
    out = A.output_arena((4096,), torch.bfloat16, rt.device, name="out")
    ws = A.workspace_arena(16, rt.device)
    assert lib.vcg_maxpool2x2_nhwc_bf16_fwd(one.ptr, out.ptr, 1, 4, 4, 12, rt.stream) == E_UNSUPPORTED
    assert lib.vcg_maxpool2x2_nhwc_bf16_fwd(one.ptr, out.ptr, 1, 1, 4, 8, rt.stream) == E_SHAPE
    assert lib.vcg_maxpool2x2_nhwc_bf16_fwd(one.ptr, out.ptr + 2, 1, 4, 4, 8, rt.stream) == E_UNSUPPORTED
    assert lib.vcg_maxpool2x2_nhwc_bf16_fwd(None, out.ptr, 1, 4, 4, 8, rt.stream) == E_NULL
    assert lib.vcg_maxpool2x2_relu_nhwc_bf16_bwd(one.ptr, one.ptr, out.ptr, 1, 4, 1, 8, rt.stream) == E_SHAPE
    assert lib.vcg_maxpool2x2_relu_nhwc_bf16_bwd(one.ptr, one.ptr, out.ptr, 1, 4, 4, 20, rt.stream) == E_UNSUPPORTED
    assert lib.vcg_maxpool2x2_relu_nhwc_bf16_bwd(one.ptr, None, out.ptr, 1, 4, 4, 8, rt.stream) == E_NULL
    assert lib.vcg_feature_loss_bf16(one.ptr, one.ptr, 0, 0, 1.0, out.ptr, out.ptr, ws.ptr, 16, rt.stream) == E_SHAPE
    assert lib.vcg_feature_loss_bf16(one.ptr, one.ptr, 64, 5, 1.0, out.ptr, out.ptr, ws.ptr, 16, rt.stream) == E_UNSUPPORTED
    assert lib.vcg_feature_loss_bf16(one.ptr, one.ptr, 64, 0, 1.0, out.ptr, out.ptr, ws.ptr, 12, rt.stream) == E_WORKSPACE
    assert lib.vcg_feature_loss_bf16(one.ptr, one.ptr, 64, 0, 1.0, None, out.ptr, ws.ptr, 16, rt.stream) == E_NULL
    torch.cuda.current_stream().synchronize()
    for a in (one, out, ws):
        a.check()
    assert out.untouched() and ws.untouched()

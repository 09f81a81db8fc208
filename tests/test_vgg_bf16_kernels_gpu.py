"""The three bandwidth kernels of the bf16 VGG19 perceptual loss (include/vcg.h: vcg_maxpool2x2_nhwc_bf16_fwd,
vcg_maxpool2x2_relu_nhwc_bf16_bwd, vcg_feature_loss_bf16), each launch against the exact function of its own inputs:
  * pooling forward and backward select and copy stored values, so they are compared BIT FOR BIT with torch on the bf16 values -- with planted
    ties (equal positive values among them), all-zero windows, negative maxima and odd heights / widths;
  * the loss value to 1e-5 relative of the fp64 mean, the gradient within one bf16 rounding of the fp64 gradient (|dz - g| <= 2^-8 |g|: half
    an ulp of 2^-7 relative to the binade's lower end, the unit roundoff of round-to-nearest on 8 significant bits; times 1.01 for the fp32
    arithmetic in front of the rounding), and exactly zero
    where f_pred is not positive -- with p == t and p == 0 elements, for both kinds, at counts that are no multiple of 8, of the workgroup's
    2048 elements, and beyond the 1024-workgroup grid's span (the grid-stride loop)."""
import pytest
import torch

import _vgg_bf16_emulation as V

pytestmark = pytest.mark.gpu


def _pool_case(n, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g).to(torch.bfloat16)
    x[0, 0:2, 0:2, :] = 0.0                                  # an all-zero window: no gradient (the maximum is not > 0)
    if h >= 4 and w >= 4:
        x[0, 2:4, 0:2, :] = 0.75                             # four equal positive values: the first takes the gradient
        x[0, 0:2, 2:4, :] = -0.5                             # a negative maximum, tied: pooled but masked
        x[0, 2, 2, :], x[0, 2, 3, :], x[0, 3, 2, :], x[0, 3, 3, :] = 0.25, 1.5, 1.5, -2.0          # a tie of the last two candidates
        x[-1, -2:, -2:, 0::3] = 2.0                          # ties in the last complete (or cut) window
    else:
        x[0, :, :, 4:] = 1.25                                # the only window: all-zero in channels 0-3, four equal positive values in the rest
    return x


@pytest.mark.parametrize("n,h,w,c", [(2, 5, 8, 16), (1, 33, 47, 64), (1, 2, 2, 8)])
def test_pool_forward_and_backward_bit_exact(rt, n, h, w, c):
    from upscaler import _engine as E
    x = _pool_case(n, h, w, c, h * w)
    xr = x.float().permute(0, 3, 1, 2).contiguous()
    yr, idx = torch.nn.functional.max_pool2d(xr, 2, 2, return_indices=True)
    dy = torch.randn(n, h // 2, w // 2, c, generator=torch.Generator().manual_seed(7)).to(torch.bfloat16)
    dzr = torch.nn.functional.max_unpool2d(dy.float().permute(0, 3, 1, 2).contiguous(), idx, 2, 2, output_size=(h, w)) * (xr > 0)
    xd, dyd = x.to(rt.device), dy.to(rt.device)
    y = E.maxpool2x2_nhwc_bf16(rt, xd)
    dz = E.maxpool2x2_relu_nhwc_bf16_bwd(rt, xd, dyd)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (n, h // 2, w // 2, c)
    assert torch.equal(y.cpu().view(torch.int16), yr.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous().view(torch.int16))
    got = dz.cpu().float()
    assert torch.equal(got, dzr.permute(0, 2, 3, 1))
    assert not (got[:, 2 * (h // 2):] != 0).any() and not (got[:, :, 2 * (w // 2):] != 0).any()
    zc = slice(None) if h >= 4 and w >= 4 else slice(0, 4)
    assert not (got[0, 0:2, 0:2, zc] != 0).any()             # the all-zero window
    if h >= 4 and w >= 4:
        assert torch.equal(got[0, 2, 0], dy[0, 1, 0].float()) and not (got[0, 2:4, 0:2].reshape(4, c)[1:] != 0).any()
        assert not (got[0, 0:2, 2:4] != 0).any()
        assert torch.equal(got[0, 2, 3], dy[0, 1, 1].float()) and not (got[0, 3, 2] != 0).any()
    # a second launch into a buffer full of NaNs: every element is written
    dz2 = torch.full_like(dz, float("nan"))
    from upscaler import _lib as L
    L.check(rt.lib.vcg_maxpool2x2_relu_nhwc_bf16_bwd(xd.data_ptr(), dyd.data_ptr(), dz2.data_ptr(), n, h, w, c, rt.stream), "bwd")
    assert torch.equal(dz2.cpu().view(torch.int16), dz.cpu().view(torch.int16))


@pytest.mark.parametrize("kind", ["mse", "mae"])
@pytest.mark.parametrize("count", [13, 8 * 256 * 3 + 5, 2048 * 1024 + 8 * 300 + 3])
def test_feature_loss_value_and_gradient(rt, kind, count):
    from upscaler import _engine as E
    g = torch.Generator().manual_seed(count % 1000)
    t = torch.relu(torch.randn(count, generator=g)).to(torch.bfloat16)
    p = torch.relu(torch.randn(count, generator=g)).to(torch.bfloat16)            # half of the elements are p == 0 (and many t == 0)
    p[::7] = t[::7]                                                                # p == t elements (sign(0) = 0 for the MAE)
    p[3::11] = -p[3::11]                                                           # negative values: masked as well
    scale = 3.0
    val, dz = E.feature_loss_bf16(rt, t.to(rt.device), p.to(rt.device), kind, scale)
    ref = V.loss_value(t, p, kind)
    gref = V.loss_grad(t, p, kind, scale, round_grads=False)
    got = dz.cpu().double()
    rel = abs(float(val.item()) - ref) / ref
    err = (got - gref).abs()
    worst = float((err / gref.abs().clamp_min(1e-300))[gref != 0].max())
    print("feature loss %s count=%d: value rel err %.2e, gradient worst |dz - g| / |g| = %.3e (2^-8 = %.3e)" % (kind, count, rel, worst, 2.0 ** -8))
    assert rel < 1e-5
    assert bool((err <= 1.01 * 2.0 ** -8 * gref.abs()).all())
    assert bool((got[p.float() <= 0] == 0).all()) and bool((got[gref == 0] == 0).all())
    assert int((gref != 0).sum()) > count // 8                                     # the check above is not vacuous
    # deterministic: a second launch gives the same bits
    val2, dz2 = E.feature_loss_bf16(rt, t.to(rt.device), p.to(rt.device), kind, scale)
    assert float(val2.item()) == float(val.item()) and torch.equal(dz2.view(torch.int16), dz.view(torch.int16))

"""The kernels bf16 inference of make_upscaler_incep_resnet adds (include/vcg.h: vcg_incep_head_bf16_fwd, vcg_conv2d_nhwc_bf16_fwd_epilogue,
vcg_incep_join_bf16_fwd, with vcg_pack_incep_frag_bf16 and vcg_incep_fold): each launch of a block against the fp64 function of its own
bf16-rounded inputs (tests/_incep_bf16_emulation.py), with the bars of tests/test_infer_cyclegan_bf16_gpu.py -- max-norm relative error
< 2^-8 and the ulp-scaled element-wise check < 1.

Block parameters exercise both PReLU branches (BatchNormalization scales of both signs, negative shifts, slopes in 0.05 .. 0.4).  Shapes
n x h x w: 2x5x7 (inside one 32-pixel tile, odd), 1x9x33 (one row / column past an 8x32 tile; more than one workgroup of 128 pixels), 3x1x1;
1x7 and 7x1 also at 1x5x5 (extent shorter than the kernel); 1xk / kx1 with k = 3, 5 at one shape each; the 48 -> 64 layer also at 2x32x256,
the smallest size at which the generic kernels take their LDS-tiled form (64 tile-groups).  Head path sets (32, 32, 32) and (32, 19), join
sources (32, 32, 64) and (32, 32).  Every output buffer is pre-filled with NaN bytes: padded channels must read back as exact zeros, and
every launch but the head consumes a padded tensor the device wrote, so a NaN left in the padding would show downstream."""
import pytest
import torch

import _incep_bf16_emulation as EM
import _incep_kernel_calls as C
from conftest import rel_err, report

pytestmark = pytest.mark.gpu

SHAPES = [(2, 5, 7), (1, 9, 33), (3, 1, 1)]
CASES = [("3path", 3, s) for s in SHAPES] + [("3path", 5, s) for s in SHAPES] + [("2path", 7, s) for s in SHAPES + [(1, 5, 5)]] \
    + [("2path", 3, (2, 5, 7)), ("2path", 5, (1, 9, 33))]


@pytest.mark.parametrize("btype,k,shape", CASES, ids=["%s-k%d-%dx%dx%d" % ((b, k) + s) for b, k, s in CASES])
def test_block_launch_by_launch(rt, btype, k, shape):
    n, h, w = shape
    res, _ = C.run_block(rt, btype, k, n, h, w)
    assert [r[0].split()[0] for r in res] == (["head"] * 3 + ["mid"] * 3 if btype == "3path" else ["head"] * 2 + ["mid"] * 2) + ["join"]
    for what, got, ref in res:
        assert got.shape == ref.shape, what
        assert float(ref.min()) < 0 < float(ref.max()), what
        e, ew = rel_err(got, ref), C.ulp_scaled(got, ref)
        report("bf16 incep %s k%d n=%d %dx%d %s: err=%.2e ulp-scaled=%.2f" % (btype, k, n, h, w, what, e, ew))
        assert e < C.TOL_BF16 and ew < 1.0, (what, e, ew)


def test_both_prelu_branches_are_exercised():
    """the parameters of the cases above: scales of both signs, negative shifts, slopes inside 0.05 .. 0.4 (no device needed, but the
    statement belongs to this file's cases)"""
    for btype, k in (("3path", 3), ("2path", 7)):
        w = C.block_weights(btype, k, 1000 * k + (7 if btype == "3path" else 0))
        for name, v in w.items():
            if name.endswith("/gamma"):
                assert float(v.min()) < 0 < float(v.max()), name
            elif name.endswith("/beta"):
                assert float(v.min()) < -0.3, name
            elif name.endswith("/alpha"):
                assert 0.05 <= float(v.min()) and float(v.max()) <= 0.4, name


@pytest.mark.parametrize("k", [3, 5])
def test_c3_on_the_tiled_kernel(rt, k):
    """c/3 (48 -> 64 on 64 stored channels) at 2x32x256: 64 groups of 8x32-pixel tiles, where the generic kernels switch to their LDS-tiled
    form; x has zeros in its padded channels, as c/2 stores them"""
    n, h, w = 2, 32, 256
    wt = C.block_weights("3path", k, 50 + k)
    w64 = {kk: v.double() for kk, v in wt.items()}
    name = C.block_spec("3path", k)[0]
    x = torch.randn(n, 48, h, w, generator=torch.Generator().manual_seed(k))
    dev = C.Device(rt)
    xb = C.to_nhwc_bf16(x, 64)
    y, _ = C.run_mid(dev, wt, "3path", k, "c/3", dev.put(xb, "x"), n, h, w)
    got = C.stored(y, n, h, w, 64)
    dev.check()
    with torch.no_grad():
        ref = EM.f_mid(w64, name, "c/3", k, k, None, xb[..., :48].float().permute(0, 3, 1, 2).double())
    e, ew = rel_err(got, ref), C.ulp_scaled(got, ref)
    report("bf16 incep c/3 %dx%d 48->64 n=%d %dx%d (tiled kernel): err=%.2e ulp-scaled=%.2f" % (k, k, n, h, w, e, ew))
    assert e < C.TOL_BF16 and ew < 1.0


def test_head_reads_the_block_input_once_for_all_paths(rt):
    """the same block input through the 3-path and the 2-path head: path a/1 of both, given the same parameters, is the same tensor bit for
    bit (the paths of a launch do not disturb one another)"""
    n, h, w = 1, 9, 33
    w3 = C.block_weights("3path", 3, 1)
    n3, n2 = C.block_spec("3path", 3)[0], C.block_spec("2path", 3)[0]
    w2 = C.block_weights("2path", 3, 2)
    for key in list(w3):
        if key.startswith(n3 + "/a/1/"):
            w2[n2 + key[len(n3):]] = w3[key]
    m = C.to_nhwc_bf16(torch.randn(n, 64, h, w, generator=torch.Generator().manual_seed(3)))
    dev = C.Device(rt)
    ma = dev.put(m, "m")
    o3 = C.run_head(dev, w3, "3path", 3, ma, n, h, w)
    o2 = C.run_head(dev, w2, "2path", 3, ma, n, h, w)
    dev.check()
    assert torch.equal(o3["a/1"].payload.cpu(), o2["a/1"].payload.cpu())
    assert not torch.equal(o3["b/1"].payload.cpu(), o2["b/1"].payload.cpu())

"""The fp32 weight-gradient kernel's tile loop (csrc/conv_wgrad.hip) at the smallest shapes where every workgroup walks
several pixel tiles, crosses a row end and an image boundary inside its slab, has ragged right / bottom edges and channel
counts that are no multiple of the block.  tiles per workgroup (make_plan's formulas): trunk 3, 4x4 stride 1 3,
stride 2 2, 5x5 3, 9x9 swapped 1, convT 5.

Reference: the fp64 oracle.  dw / dx under test_kernels_gpu.TOL.  The bias gradient is a plain fp32 sum of dy = randn + 3
(a real sum, not noise); its bound is max(2 x the parent commit's error, 1e-6) on the same case -- PARENT_DB_ERR, from
profiles/wgrad_f32_tileloop_parity.txt.  The factor 2 would allow a different but equally long fp32 summation order; the
kernel keeps the parent's order (one chain per channel, pixel after pixel), so the errors are the parent's."""
import numpy as np
import pytest
import torch

from conftest import rel_err, report

pytestmark = pytest.mark.gpu
TOL = 1e-3           # the file-wide bound of tests/test_kernels_gpu.py

# kind, cin, cout, k, stride, padding, n, h, w
CASES = {
    "trunk3x3": ("conv", 64, 64, 3, 1, "same", 3, 70, 150),
    "k4s1_big": ("conv", 40, 72, 4, 1, 1, 3, 41, 71),
    "k3s2": ("conv", 64, 128, 3, 2, "same", 4, 63, 95),
    "k5": ("conv", 64, 64, 5, 1, "same", 2, 70, 150),
    "k9_swapped": ("conv", 64, 3, 9, 1, "same", 2, 40, 150),
    "convT": ("convT", 64, 256, 3, 2, "same", 3, 35, 75),
}
# db error of the parent commit's kernel on the same case (profiles/wgrad_f32_tileloop_parity.txt)
PARENT_DB_ERR = {
    "trunk3x3": 1.244e-07,
    "k4s1_big": 8.935e-08,
    "k3s2": 1.437e-07,
    "k5": 7.860e-08,
    "k9_swapped": 6.217e-08,
    "convT": 1.122e-07,
}

_REF = {}


def _case(rt, name):
    """layer, parameter store, device inputs and the fp64 reference of one case: computed once, shared, never written to"""
    if name in _REF:
        return _REF[name]
    from upscaler import _engine as E
    from oracle import keras_ops as K
    from test_kernels_gpu import _standalone
    kind, cin, cout, k, stride, padding, n, h, w = CASES[name]
    layer = E.Conv2D("c", cin, cout, k, stride, padding) if kind == "conv" else E.ConvT2D("c", cin, cout, k)
    ps, wd = _standalone(rt, layer, seed=cin + cout + k)
    g = torch.Generator().manual_seed(17)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    wk = wd["c/kernel"].clone().requires_grad_(True)
    bk = wd["c/bias"].clone().requires_grad_(True)
    yr = K.conv2d(xr, wk, bk, stride, padding) if kind == "conv" else K.conv2d_transpose_same(xr, wk, bk, 2)
    dy = torch.randn(*yr.shape, generator=g, dtype=torch.float64) + 3.0
    (yr * dy).sum().backward()
    _REF[name] = (layer, ps, x.float().to(rt.device), dy.float().to(rt.device),
                  xr.grad.detach(), wk.grad.detach(), bk.grad.detach())
    return _REF[name]


def _run(layer, ps, xd, dyd):
    _, ctx = layer.forward(xd)
    dx = layer.backward(ctx, dyd, True, True, 0)
    return dx, ps.grad("c/kernel").clone(), ps.grad("c/bias").clone()


@pytest.mark.parametrize("name", list(CASES))
def test_wgrad_tile_loop(rt, name):
    layer, ps, xd, dyd, dx_ref, dw_ref, db_ref = _case(rt, name)
    dx, dw, db = _run(layer, ps, xd, dyd)
    e_dx, e_dw, e_db = rel_err(dx, dx_ref), rel_err(dw, dw_ref), rel_err(db, db_ref)
    report("wgrad tile loop %-10s dx=%.3e dw=%.3e db=%.3e (parent db=%.3e)" % (name, e_dx, e_dw, e_db, PARENT_DB_ERR[name]))
    assert e_dx < TOL and e_dw < TOL
    assert e_db <= max(2.0 * PARENT_DB_ERR[name], 1e-6), (e_db, PARENT_DB_ERR[name])


def test_wgrad_tile_loop_is_deterministic(rt):
    layer, ps, xd, dyd = _case(rt, "trunk3x3")[:4]
    _, dw1, db1 = _run(layer, ps, xd, dyd)
    _, dw2, db2 = _run(layer, ps, xd, dyd)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)

"""The persistent flat-K kernel for layers with three or fewer input channels (csrc/conv_fwd.hip: conv_c3_kernel).  A
workgroup keeps one 64-channel block, stages its weights once and walks spatial tiles with the input tile double-buffered;
the launch has min(tiles, 2 x CU count) workgroups, rounded down to a multiple of the channel blocks.  So the shapes here are
the smallest at which that can go wrong: a workgroup that walks three or four tiles (both input buffers reused) with a
ragged number of tiles per workgroup, fewer tiles than workgroups, every instantiation at ragged edges with cin = 3 and
cin = 1 and cout no multiple of 64, flipped taps (the data gradient), and an input whose neighbours in memory are NaN.

Reference: the fp64 oracle (oracle.keras_ops) under TOL = 1e-3, the file-wide bound of tests/test_kernels_gpu.py (the
kernels are exact fp32 FMA chains: errors of about 1e-6 are what is seen)."""
import pytest
import torch

from conftest import rel_err, report

pytestmark = pytest.mark.gpu
TOL = 1e-3           # the file-wide bound of tests/test_kernels_gpu.py

# cin, cout, k, stride, padding, n, h, w, epilogue ("lrelu_res" = bias + LeakyReLU(0.2) + residual, None = bias)
CASES = {
    # the tile loop: on 256 CUs 512 workgroups; 2 x 31 x 12 = 744 spatial tiles on 256 workgroups per channel block (dgrad, 70 = 64 + 6
    # channels: 3 tiles for some, 2 for the others) and 4 x 32 x 13 = 1664 tiles on 512 workgroups (forward: 4 and 3), both edges ragged
    "loop_dgrad": (70, 3, 9, 1, "same", 2, 245, 371, None),
    "loop_fwd": (3, 64, 9, 1, "same", 4, 250, 400, "lrelu_res"),
    # fewer tiles than 2 x CU count: 2 spatial tiles, 2 channel blocks
    "few_fwd": (3, 70, 9, 1, "same", 1, 9, 13, None),
    "few_dgrad": (70, 3, 9, 1, "same", 1, 9, 13, None),
    # every instantiation at ragged edges
    "k3_c1": (1, 70, 3, 1, "same", 2, 13, 45, None),
    "k5_c3": (3, 70, 5, 1, "same", 2, 20, 40, "lrelu_res"),
    "k9_c1": (1, 70, 9, 1, "same", 2, 20, 45, None),
    "k4s2_c3": (3, 70, 4, 2, 1, 2, 37, 50, None),
    "k4s2_c1": (1, 130, 4, 2, 1, 1, 19, 70, None),
    "k5_flip": (70, 3, 5, 1, "same", 2, 20, 40, None),       # data gradient: <5,5,1> with flipped taps, 3 -> 70
    "k3_flip_c1": (70, 1, 3, 1, "same", 2, 13, 45, None),    # data gradient: <3,3,1>, one input channel
}
FWD = ["loop_fwd", "few_fwd", "k3_c1", "k5_c3", "k9_c1", "k4s2_c3", "k4s2_c1"]
DGRAD = ["loop_dgrad", "few_dgrad", "k5_flip", "k3_flip_c1"]
LOOPING = {"loop_fwd": "fwd", "loop_dgrad": "dgrad"}

_REF = {}


def _case(rt, name):
    """layer, parameters, device inputs and the fp64 reference of one case: computed once, shared, never written to"""
    if name in _REF:
        return _REF[name]
    from upscaler import _engine as E, _lib as L
    from oracle import keras_ops as K
    from test_kernels_gpu import _standalone
    cin, cout, k, stride, padding, n, h, w, epi = CASES[name]
    act, alpha = (L.ACT_LRELU, 0.2) if epi == "lrelu_res" else (L.ACT_NONE, 0.0)
    layer = E.Conv2D("c", cin, cout, k, stride, padding, act, alpha)
    ps, wd = _standalone(rt, layer, seed=cin + cout + k)
    g = torch.Generator().manual_seed(29)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    dev = lambda t: t.float().to(rt.device)
    c = dict(layer=layer, ps=ps, x=dev(x), epi=epi)
    if name in DGRAD:
        xr = x.clone().requires_grad_(True)
        zr = K.conv2d(xr, wd["c/kernel"], wd["c/bias"], stride, padding)
        dy = torch.randn(*zr.shape, generator=g, dtype=torch.float64)
        skip = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
        (dx,) = torch.autograd.grad((zr * dy).sum(), xr)
        c.update(dy=dev(dy), skip=dev(skip), dx_ref=dx + skip)
    else:
        with torch.no_grad():
            zr = K.conv2d(x, wd["c/kernel"], wd["c/bias"], stride, padding)
            res = torch.randn(*zr.shape, generator=g, dtype=torch.float64)
            c.update(res=dev(res), y_ref=K.leaky_relu(zr, 0.2) + res if epi == "lrelu_res" else zr)
    _REF[name] = c
    return c


def _forward(c, x=None):
    x = c["x"] if x is None else x
    return c["layer"].forward(x, residual=c["res"] if c["epi"] == "lrelu_res" else None)[0]


def _dgrad(c):
    layer = c["layer"]
    ctx = (c["x"], None, layer.desc(*[c["x"].shape[i] for i in (0, 2, 3)]))
    return layer.backward(ctx, c["dy"], True, False, 0, dx_residual=c["skip"])


def _tiles_per_workgroup(cus, n, oh, ow, cout):
    """(busiest, idlest): spatial tiles of the workgroups of one channel block under the kernel's grid rule"""
    co_blocks = -(-cout // 64)
    spatial = n * -(-oh // 8) * -(-ow // 32)
    tiles = spatial * co_blocks
    grid = min(tiles, 2 * cus)
    grid = max(grid - grid % co_blocks, co_blocks)
    per_block = grid // co_blocks
    return -(-spatial // per_block), spatial // per_block


@pytest.mark.parametrize("name", sorted(LOOPING))
def test_looping_cases_really_loop(name):
    """a condition of the tests below, not a measurement: on this device the busiest workgroup walks at least three tiles
    (both input buffers are reused) and the tiles do not divide evenly over the workgroups"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cin, cout, _, _, _, n, h, w, _ = CASES[name]
    busiest, idlest = _tiles_per_workgroup(cus, n, h, w, cout if LOOPING[name] == "fwd" else cin)
    report("conv c3 persistent %-10s CUs=%d tiles per workgroup: busiest %d, idlest %d" % (name, cus, busiest, idlest))
    assert busiest >= 3 and busiest != idlest, (cus, busiest, idlest)


@pytest.mark.parametrize("name", FWD)
def test_c3_forward(rt, name):
    c = _case(rt, name)
    e = rel_err(_forward(c), c["y_ref"])
    report("conv c3 persistent fwd   %-10s %.3e" % (name, e))
    assert e < TOL


@pytest.mark.parametrize("name", DGRAD)
def test_c3_dgrad(rt, name):
    """the stride-1 data gradient runs the same kernel with flipped taps, the skip gradient is the launch's residual"""
    c = _case(rt, name)
    e = rel_err(_dgrad(c), c["dx_ref"])
    report("conv c3 persistent dgrad %-10s %.3e" % (name, e))
    assert e < TOL


@pytest.mark.parametrize("name", ["k9_c1", "k4s2_c3", "loop_fwd"])
def test_c3_input_between_nan_neighbours(rt, name):
    """the input as a view into a larger buffer that is NaN on both sides of it (laid out as tests/_arena.py lays out its
    input arenas: 64 KiB guards of 0xFF bytes): padding and ragged edges must read zeros, never a neighbour -- a zero weight
    does not cancel a NaN -- so the result is finite and bit-equal to the plain run"""
    c = _case(rt, name)
    x = c["x"]
    guard = 64 * 1024
    raw = torch.full((2 * guard + x.numel() * 4,), 0xFF, dtype=torch.uint8, device=x.device)
    view = raw[guard:guard + x.numel() * 4].view(torch.float32).view(*x.shape)
    view.copy_(x)
    assert bool(torch.isnan(raw[:guard].view(torch.float32)).all()) and bool(torch.isnan(raw[-guard:].view(torch.float32)).all())
    y = _forward(c, view)
    assert bool(torch.isfinite(y).all())
    assert torch.equal(y, _forward(c))


def test_c3_tile_loop_is_deterministic(rt):
    c = _case(rt, "loop_dgrad")
    a, b = _dgrad(c), _dgrad(c)
    assert a.data_ptr() != b.data_ptr()
    assert torch.equal(a, b)

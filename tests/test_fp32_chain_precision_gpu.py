"""Every fp32 contraction kernel held to the accuracy of an fp32 accumulation chain, output by output (tests/_chain_error.py):
rho(kernel) <= 4 * rho_seq, where rho = max_i |y_i - y64_i| / (2^-24 * T_i), T_i the random-walk scale of output i from the fp64 oracle
on the squared operands, and rho_seq the same figure of the strictly sequential fp32 chain on the CPU, computed here on the same
data.  The max-norm bound of the other files (1e-3 of the tensor's maximum) passes a convolution on tf32-cut operands and an error
of 1e-4 * max in one border pixel (tests/test_chain_error_cpu.py shows both); this one does not.

Forward (K = cin*kh*kw), data gradient (plain; K = cout * taps), weight gradient and bias gradient (K = n*oh*ow), each against its own
T and its own reference chain; bias, no activation; inputs and parameters fp32-exact.  The shapes are the smallest that reach each
instantiation.  One line per check goes to the report: case, check, rho, rho_seq, K, the kernel that serves it;
profiles/fp32_chain_precision.txt is that table from an MI355X.

Known weakness: the bias gradient of a layer with 1 - 3 output channels is a maximum over 1 - 3 numbers, so its rho_seq is one draw of a
rounding error (0.03 for smallm_16to1_k4, which vcg_channel_sum meets with 0.04).  A legitimate reordering of that sum can miss 4 * rho_seq
by chance; the checks with hundreds of outputs and more cannot."""
import pytest
import torch

import _chain_error as C
from conftest import report

pytestmark = pytest.mark.gpu
CHECKS = ("fwd", "dx", "dw", "db")
TILED = "conv_fwd_kernel<%s>"
WG = "wgrad_kernel"

# name: (cin, cout, k, stride, padding, n, h, w), {check: the kernel the engine routes it to}
CONV_CASES = {
    "trunk_64to64_k3": ((64, 64, 3, 1, "same", 2, 16, 32), dict(fwd=TILED % "3,3,1,8,1", dx=TILED % "3,3,1,8,1" + " flipped")),
    "k3_5to70_w75": ((5, 70, 3, 1, "same", 2, 13, 75), dict(fwd=TILED % "3,3,1,8,2", dx=TILED % "3,3,1,8,2" + " flipped")),
    "k3_5to70_w30": ((5, 70, 3, 1, "same", 2, 13, 30), dict(fwd=TILED % "3,3,1,8,1", dx=TILED % "3,3,1,8,1" + " flipped")),
    "k3s2_12to70": ((12, 70, 3, 2, "same", 2, 13, 37), dict(fwd=TILED % "3,3,2,8,1", dx="convt_kernel<3>")),
    "k4s1_40to72": ((40, 72, 4, 1, 1, 2, 21, 37), dict(fwd=TILED % "4,4,1,8,1", dx=TILED % "4,4,1,8,1" + " flipped")),
    "k4s2_12to130": ((12, 130, 4, 2, 1, 2, 37, 50), dict(fwd=TILED % "4,4,2,4,1", dx="convt_kernel<4>")),
    "k5_12to70": ((12, 70, 5, 1, "same", 2, 20, 40), dict(fwd=TILED % "5,5,1,8,1", dx=TILED % "5,5,1,8,1" + " flipped")),
    "k1x7_19to25": ((19, 25, (1, 7), 1, "same", 2, 13, 45), dict(fwd=TILED % "1,7,1,8,1", dx=TILED % "1,7,1,8,1" + " flipped")),
    "k7x1_25to32": ((25, 32, (7, 1), 1, "same", 2, 13, 45), dict(fwd=TILED % "7,1,1,8,1", dx=TILED % "7,1,1,8,1" + " flipped")),
    "k1x1_64to19": ((64, 19, (1, 1), 1, "same", 2, 13, 45), dict(fwd=TILED % "1,1,1,8,1", dx=TILED % "1,1,1,8,1")),
    # conv_c3_kernel: forward of the first, data gradient (flipped taps, 3 -> 70) of the second; the other direction of each is the
    # small-M kernel's (3 * 9 <= 32 rows), the first one's weight gradient the 3-channel orientation (cin <= 3 as the B operand)
    "c3_3to70_k9": ((3, 70, 9, 1, "same", 2, 20, 45), dict(fwd="conv_c3_kernel<9,9,1>", dx="conv_smallm_kernel<9,9,8> flipped (not conv_c3)")),
    "c3_70to3_k9": ((70, 3, 9, 1, "same", 2, 20, 45), dict(fwd="conv_smallm_kernel<9,9,8> (not conv_c3)", dx="conv_c3_kernel<9,9,1> flipped",
                                                             dw=WG + " swapped orientation (cout <= 3)")),
    "smallm_256to3_k9": ((256, 3, 9, 1, "same", 1, 12, 70), dict(fwd="conv_smallm_kernel<9,9,8>", dx="conv_c3_kernel<9,9,1> flipped",
                                                                  dw=WG + " swapped orientation (cout <= 3)")),
    "smallm_64to3_k9": ((64, 3, 9, 1, "same", 2, 9, 50), dict(fwd="conv_smallm_kernel<9,9,8>", dx="conv_c3_kernel<9,9,1> flipped",
                                                               dw=WG + " swapped orientation (cout <= 3)")),
    "smallm_16to1_k4": ((16, 1, 4, 1, 1, 2, 8, 70), dict(fwd="conv_smallm_kernel<4,4,8> (cin < 64: not the cout=1 reduction)",
                                                          dx=TILED % "4,4,1,8,1" + " flipped (no conv_c3<4,4,1>)", dw=WG + " swapped orientation (cout <= 3)")),
    "cout1_512to1_k4": ((512, 1, 4, 1, 1, 1, 10, 10), dict(fwd="conv_cout1_kernel<4>", dx=TILED % "4,4,1,8,1" + " flipped (no conv_c3<4,4,1>)",
                                                            dw=WG + " swapped orientation (cout <= 3)")),
    "rowchain_256to3_k9_w64": ((256, 3, 9, 1, "same", 1, 12, 64), dict(fwd="conv9x9_rowchain_f32_kernel", dx="conv_c3_kernel<9,9,1> flipped",
                                                                       dw=WG + " swapped orientation (cout <= 3)")),
}
# name: (cin, cout, k, n, h, w)
CONVT_CASES = {
    "convT_70to12_k3": ((70, 12, 3, 2, 7, 19), dict(fwd="convt_kernel<3>", dx=TILED % "3,3,2,8,1")),
    "convT_64to256_k3": ((64, 256, 3, 1, 8, 32), dict(fwd="convt_kernel<3>", dx=TILED % "3,3,2,8,1")),
    "convT_64to256_k5": ((64, 256, 5, 1, 9, 33), dict(fwd="convt_kernel<5>", dx=TILED % "5,5,2,4,1")),
    "convT_128to64_k3": ((128, 64, 3, 2, 12, 20), dict(fwd="convt_kernel<3>", dx=TILED % "3,3,2,8,1")),
}
# name: (batch, cin, cout)
DENSE_CASES = {"dense_2x77to130": (2, 77, 130), "dense_3x1024to32": (3, 1024, 32), "dense_8x32to1": (8, 32, 1)}

_REF = {}


def _rand(g, *shape):
    return C.f32_exact(torch.randn(*shape, generator=g, dtype=torch.float64))


def _case(rt, name):
    """the fp64 results, T, K and reference chains of one case and the kernels' four results: computed once, shared, never written to"""
    if name in _REF:
        return _REF[name]
    from upscaler import _engine as E
    from test_kernels_gpu import _standalone
    dev = lambda t: t.float().to(rt.device)
    g = torch.Generator().manual_seed(29)
    if name in CONV_CASES:
        (cin, cout, k, stride, padding, n, h, w), served = CONV_CASES[name]
        layer = E.Conv2D("c", cin, cout, k, stride, padding)
        ps, wd = _standalone(rt, layer, seed=cin + cout + h)
        oh, ow, _, _ = layer.out_hw(h, w)
        x, dy = _rand(g, n, cin, h, w), _rand(g, n, cout, oh, ow)
        checks = C.conv_checks(x, wd["c/kernel"], wd["c/bias"], dy, stride, padding)
        y, ctx = layer.forward(dev(x))
    elif name in CONVT_CASES:
        (cin, cout, k, n, h, w), served = CONVT_CASES[name]
        layer = E.ConvT2D("c", cin, cout, k)
        ps, wd = _standalone(rt, layer, seed=cin + cout + h)
        x, dy = _rand(g, n, cin, h, w), _rand(g, n, cout, 2 * h, 2 * w)
        checks = C.convt_checks(x, wd["c/kernel"], wd["c/bias"], dy)
        y, ctx = layer.forward(dev(x))
    else:
        b, cin, cout = DENSE_CASES[name]
        served = dict(fwd="dense_fwd_kernel", dx="dense_dgrad_kernel", dw="dense_wgrad_kernel", db="dense_dbias_kernel")
        layer = E.Dense("c", cin, cout)
        ps, wd = _standalone(rt, layer, seed=cin + cout + b)
        x, dy = _rand(g, b, cin), _rand(g, b, cout)
        checks = C.dense_checks(x, wd["c/kernel"], wd["c/bias"], dy)
        y, ctx = layer.forward(dev(x))
    dx = layer.backward(ctx, dev(dy), True, True, 0)
    got = dict(fwd=y.cpu(), dx=dx.cpu(), dw=ps.grad("c/kernel").cpu().clone(), db=ps.grad("c/bias").cpu().clone())
    # the weight gradient's normal orientation sums the bias gradient from its staged dy tiles; the others leave it to vcg_channel_sum
    own_db = name in CONV_CASES and "dw" not in served
    served = dict(dict(dw=WG, db=WG + " (bias chain)" if own_db else "channel_sum"), **served)
    _REF[name] = dict(checks=checks, got=got, served=served)
    return _REF[name]


@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("name", list(CONV_CASES) + list(CONVT_CASES) + list(DENSE_CASES))
def test_fp32_kernel_is_as_accurate_as_an_fp32_chain(rt, name, check):
    c = _case(rt, name)
    ref, got = c["checks"][check], c["got"][check]
    r = C.rho(got.view(ref["y64"].shape), ref["y64"], ref["t"])
    report("fp32 chain %-24s %-3s rho=%7.2f rho_seq=%5.2f K=%-5d %s" % (name, check, r, ref["rho_seq"], ref["k"], c["served"][check]))
    assert ref["rho_seq"] <= ref["sane"], "the reference chain is no fp32 chain of this contraction: %.3g" % ref["rho_seq"]
    assert r <= C.FACTOR * ref["rho_seq"], (r, ref["rho_seq"])

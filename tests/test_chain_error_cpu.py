"""Self-test of the fp32-chain metric (tests/_chain_error.py), torch on the CPU only: what it must pass, what it must fail.

Passes: torch's own blocked fp32 conv2d / matmul, the reference chain in a permuted order.  Fails: operands cut to tf32's 10
mantissa bits (every shape), a split-bf16 product of three terms (the shapes with K <= 600), and an fp32 result with 1e-4 * max|y|
added to ONE low-energy output -- which the suite's max-norm bound of 1e-3 lets through, as it does the tf32 results.  Also pinned:
K from the tensors of ones, and the gathers behind the gradient / transposed / dense reference chains (each is an fp32 chain of the
fp64 oracle's own result: rho_seq of the size the theory gives)."""
import pytest
import torch
import torch.nn.functional as F

import _chain_error as C
from conftest import rel_err

# cin, cout, k, n, h, w: stride 1, 'same'.  K = cin*k*k = 576, 45, 243, 300, 5184
SHAPES = {"64to64_k3": (64, 64, 3, 2, 16, 32), "5to70_k3": (5, 70, 3, 2, 13, 30), "3to64_k9": (3, 64, 9, 1, 16, 40),
          "12to70_k5": (12, 70, 5, 2, 20, 40), "64to3_k9": (64, 3, 9, 2, 9, 50)}
SMALL_K = [s for s, v in SHAPES.items() if v[0] * v[2] * v[2] <= 600]
_DATA = {}


def _data(name):
    """operands, fp64 result, T, K and the reference chain of one shape: computed once, shared, never written to"""
    if name in _DATA:
        return _DATA[name]
    from oracle import keras_ops as K
    cin, cout, k, n, h, w = SHAPES[name]
    g = torch.Generator().manual_seed(cin * 1000 + cout + k)
    x = C.f32_exact(torch.randn(n, cin, h, w, generator=g, dtype=torch.float64))
    wk = C.f32_exact(torch.randn(k, k, cin, cout, generator=g, dtype=torch.float64))
    b = C.f32_exact(torch.randn(cout, generator=g, dtype=torch.float64))
    op = lambda a, ww: K.conv2d(a, ww, None, 1, "same")
    y64 = op(x, wk) + b.view(1, -1, 1, 1)
    t, kmap = C.scale(op, x, wk, b.view(1, -1, 1, 1))
    pads = C.conv_pads(h, w, k, k, 1, "same")
    seq = C.conv_fwd_chain(x, wk, b, 1, pads)
    _DATA[name] = dict(x=x, w=wk, b=b, y64=y64, t=t, kmap=kmap, pads=pads, rho_seq=C.rho(seq, y64, t))
    return _DATA[name]


def _torch_conv(x, w_hwio, b, pads):
    pt, pb, pl, pr = pads
    return F.conv2d(F.pad(x.float(), (pl, pr, pt, pb)), w_hwio.float().permute(3, 2, 0, 1).contiguous(), None if b is None else b.float())


@pytest.mark.parametrize("name", list(SHAPES))
def test_reference_chain_is_an_fp32_chain(name):
    d = _data(name)
    assert 0.5 < d["rho_seq"] <= C.RHO_SEQ_SANE, d["rho_seq"]


@pytest.mark.parametrize("name", list(SHAPES))
def test_torch_fp32_conv_meets_the_condition(name):
    d = _data(name)
    r = C.rho(_torch_conv(d["x"], d["w"], d["b"], d["pads"]), d["y64"], d["t"])
    assert C.meets(r, d["rho_seq"]), (r, d["rho_seq"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_permuted_chain_meets_the_condition(name):
    d = _data(name)
    cin, cout, k = SHAPES[name][:3]
    order = torch.randperm(cin * k * k, generator=torch.Generator().manual_seed(5)).tolist()
    r = C.rho(C.conv_fwd_chain(d["x"], d["w"], d["b"], 1, d["pads"], order), d["y64"], d["t"])
    assert C.meets(r, d["rho_seq"]), (r, d["rho_seq"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_tf32_operands_fail_the_condition_and_pass_the_max_norm_bound(name):
    d = _data(name)
    y = _torch_conv(C.cut_mantissa(d["x"], 10), C.cut_mantissa(d["w"], 10), d["b"], d["pads"])
    r = C.rho(y, d["y64"], d["t"])
    assert not C.meets(r, d["rho_seq"]) and r > 100 * d["rho_seq"], (r, d["rho_seq"])
    assert rel_err(y, d["y64"]) < 1e-3                       # the bound of tests/test_kernels_gpu.py does not see it


@pytest.mark.parametrize("name", SMALL_K)
def test_three_term_bf16_split_fails_the_condition(name):
    d = _data(name)
    xh, xl = C.bf16_split(d["x"])
    wh, wl = C.bf16_split(d["w"])
    y = _torch_conv(xh, wh, d["b"], d["pads"]) + (_torch_conv(xh, wl, None, d["pads"]) + _torch_conv(xl, wh, None, d["pads"]))
    r = C.rho(y, d["y64"], d["t"])
    assert not C.meets(r, d["rho_seq"]), (r, d["rho_seq"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_low_energy_output_off_by_1e_4_of_the_maximum_fails(name):
    """the other blind spot: a corner pixel of a low-energy channel"""
    from oracle import keras_ops as K
    d = _data(name)
    wk = d["w"].clone()
    wk[..., 1] *= 2.0 ** -6                                   # channel 1: 1/64 of the others' energy, exactly
    b = d["b"].clone()
    b[1] *= 2.0 ** -6
    op = lambda a, ww: K.conv2d(a, ww, None, 1, "same")
    y64 = op(d["x"], wk) + b.view(1, -1, 1, 1)
    t, _ = C.scale(op, d["x"], wk, b.view(1, -1, 1, 1))
    rho_seq = C.rho(C.conv_fwd_chain(d["x"], wk, b, 1, d["pads"]), y64, t)
    y = _torch_conv(d["x"], wk, b, d["pads"])
    assert C.meets(C.rho(y, y64, t), rho_seq)
    i = int(t.argmin())                                       # the smallest T: a border pixel of the low-energy channel
    n, co, h, w = t.shape
    assert (i // (h * w)) % co == 1
    y.view(-1)[i] += 1e-4 * float(y64.abs().max())
    r = C.rho(y, y64, t)
    assert not C.meets(r, rho_seq), (r, rho_seq)
    assert rel_err(y, y64) < 1e-3


@pytest.mark.parametrize("name", list(SHAPES))
def test_k_counts_the_taps_inside_the_image(name):
    cin, cout, k, n, h, w = SHAPES[name]
    km = _data(name)["kmap"]
    r = k // 2                                                # odd k, 'same': the window of output (oy, ox) starts at (oy - r, ox - r)
    assert bool((km[:, :, r:h - r, r:w - r] == cin * k * k).all())
    for oy, ox in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        rows = len([1 for ky in range(k) if 0 <= oy - r + ky < h])
        cols = len([1 for kx in range(k) if 0 <= ox - r + kx < w])
        assert rows < k and cols < k
        assert bool((km[:, :, oy, ox] == cin * rows * cols).all())
    assert float(km[0, 0, 0, 0]) == cin * (r + 1) ** 2


def test_torch_fp32_matmul_meets_the_condition():
    g = torch.Generator().manual_seed(3)
    x = C.f32_exact(torch.randn(3, 1024, generator=g, dtype=torch.float64))
    w = C.f32_exact(torch.randn(1024, 32, generator=g, dtype=torch.float64))
    b = C.f32_exact(torch.randn(32, generator=g, dtype=torch.float64))
    dy = C.f32_exact(torch.randn(3, 32, generator=g, dtype=torch.float64))
    ch = C.dense_checks(x, w, b, dy)
    got = {"fwd": x.float() @ w.float() + b.float(), "dx": dy.float() @ w.float().t(), "dw": x.float().t() @ dy.float(), "db": dy.float().sum(0)}
    for name, c in ch.items():
        assert c["rho_seq"] <= c["sane"], (name, c["rho_seq"])
        assert C.meets(C.rho(got[name], c["y64"], c["t"]), c["rho_seq"], c["sane"]), name
    assert ch["fwd"]["k"] == 1024 and ch["dx"]["k"] == 32 and ch["dw"]["k"] == 3 and ch["db"]["k"] == 3
    y = C.cut_mantissa(x, 10) @ C.cut_mantissa(w, 10) + b.float()
    assert not C.meets(C.rho(y, ch["fwd"]["y64"], ch["fwd"]["t"]), ch["fwd"]["rho_seq"])


# cin, cout, k, stride, padding, n, h, w: a stride, an explicit padding, a kernel that is no square, odd sizes
GRAD_CASES = [(5, 7, 3, 2, "same", 2, 9, 11), (6, 5, 4, 2, 1, 2, 10, 13), (4, 6, (1, 7), 1, "same", 1, 5, 12), (3, 9, 5, 1, "same", 2, 7, 8)]


@pytest.mark.parametrize("cin,cout,k,stride,padding,n,h,w", GRAD_CASES)
def test_gradient_chains_are_fp32_chains_of_the_oracle(cin, cout, k, stride, padding, n, h, w):
    """a wrong gather (tap, stride, padding, flip) is an error of the size of the result: rho_seq of 1e6, not of 3"""
    kh, kw = (k, k) if isinstance(k, int) else k
    g = torch.Generator().manual_seed(cin + cout)
    x = C.f32_exact(torch.randn(n, cin, h, w, generator=g, dtype=torch.float64))
    wk = C.f32_exact(torch.randn(kh, kw, cin, cout, generator=g, dtype=torch.float64))
    b = C.f32_exact(torch.randn(cout, generator=g, dtype=torch.float64))
    pads = C.conv_pads(h, w, kh, kw, stride, padding)
    oh, ow = C._out_hw(h, w, kh, kw, stride, pads)
    dy = C.f32_exact(torch.randn(n, cout, oh, ow, generator=g, dtype=torch.float64))
    ch = C.conv_checks(x, wk, b, dy, stride, padding)
    for name, c in ch.items():
        assert c["rho_seq"] <= c["sane"], (name, c["rho_seq"])
    assert ch["fwd"]["k"] == cin * kh * kw and ch["db"]["k"] == n * oh * ow and ch["dw"]["k"] <= n * oh * ow
    assert ch["dx"]["k"] <= cout * kh * kw
    # torch's autograd in fp32 meets the condition on all four
    xr, wr, br = (t.float().requires_grad_(True) for t in (x, wk, b))
    pt, pb, pl, pr = pads
    y = F.conv2d(F.pad(xr, (pl, pr, pt, pb)), wr.permute(3, 2, 0, 1), br, stride=stride)
    y.backward(dy.float())
    for name, got in (("fwd", y), ("dx", xr.grad), ("dw", wr.grad), ("db", br.grad)):
        assert C.meets(C.rho(got, ch[name]["y64"], ch[name]["t"]), ch[name]["rho_seq"], ch[name]["sane"]), name
    # and on tf32-cut operands it misses it on the three gradients (the forward pass: above): each check's T is of the size of its own chain's error, not above it
    xr, wr, br = (C.cut_mantissa(t, 10).requires_grad_(True) for t in (x, wk, b))
    F.conv2d(F.pad(xr, (pl, pr, pt, pb)), wr.permute(3, 2, 0, 1), br, stride=stride).backward(C.cut_mantissa(dy, 10))
    for name, got in (("dx", xr.grad), ("dw", wr.grad), ("db", br.grad)):
        assert not C.meets(C.rho(got, ch[name]["y64"], ch[name]["t"]), ch[name]["rho_seq"], ch[name]["sane"]), name


@pytest.mark.parametrize("cin,cout,k,n,h,w", [(5, 6, 3, 2, 4, 7), (4, 3, 5, 1, 5, 6), (3, 5, 4, 1, 3, 5)])
def test_transposed_chains_are_fp32_chains_of_the_oracle(cin, cout, k, n, h, w):
    g = torch.Generator().manual_seed(cin + cout + k)
    x = C.f32_exact(torch.randn(n, cin, h, w, generator=g, dtype=torch.float64))
    wk = C.f32_exact(torch.randn(k, k, cout, cin, generator=g, dtype=torch.float64))
    b = C.f32_exact(torch.randn(cout, generator=g, dtype=torch.float64))
    dy = C.f32_exact(torch.randn(n, cout, 2 * h, 2 * w, generator=g, dtype=torch.float64))
    ch = C.convt_checks(x, wk, b, dy)
    for name, c in ch.items():
        assert c["rho_seq"] <= c["sane"], (name, c["rho_seq"])
    assert ch["dx"]["k"] == cout * k * k and ch["dw"]["k"] <= n * h * w and ch["db"]["k"] == n * 4 * h * w
    assert ch["fwd"]["k"] == cin * ((k + 1) // 2) ** 2          # the phase with the most taps

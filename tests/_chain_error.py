"""Element-wise accuracy of an fp32 contraction against what an fp32 accumulation chain can deliver.  Plain helper (torch on the CPU
only) of tests/test_chain_error_cpu.py and tests/test_fp32_chain_precision_gpu.py.

The setting: y_i = sum_{j<K} a_ij * b_ij (+ bias_i) with fp32-representable operands -- a convolution, its data / weight / bias
gradient, a transposed convolution, a dense layer.

  random-walk scale   T_i = sqrt(K_i * sum_j (a_ij b_ij)^2 + bias_i^2), in fp64 from the SAME operation on the squared operands
                      (conv2d(x^2, w^2), ...); K_i, the number of terms output i really has, from the operation on tensors of ones,
                      so a border output carries its own smaller K.  A chain's partial sums are of size sqrt(k) * |term|, each add
                      rounds by at most u times that: the error of an fp32 chain is a random walk of size ~ u * T_i / sqrt(6).
  metric              rho(y) = max_i |y_i - y64_i| / (u * T_i),  u = 2^-24, y64 the fp64 result.  Scale-free: every output is held
                      to its own scale, not to the tensor's maximum.
  reference chain     the contraction on the CPU as a strictly sequential fp32 chain: one accumulator per output, started from
                      the bias, one rounded product added after another over all K terms in index order (chain_matmul over the
                      im2col matrix).  Terms that fall into the padding are exact zeros and leave the chain as it is.
  condition           rho(kernel) <= FACTOR * rho_seq, rho_seq measured in the same test on the same data.  FACTOR = 4: other
                      fp32 orders moved the maximum over 1e3 - 1e5 outputs by at most 1.4x (-> 2x), and a matrix instruction may add
                      its two or four products before the accumulator (-> another 2x).

Measured on the CPU (tests/test_chain_error_cpu.py holds these as assertions; profiles/fp32_chain_precision.txt has the table): the
sequential chain 1.9 - 3.9, operands rounded to tf32's 10 mantissa bits 400 - 3400, a 3-term bf16 split 15 - 65 for K <= 600."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
FACTOR = 4.0
# The reference chain itself (without a bias; rho_seq_sane adds the bias' share): each of its K adds rounds by at most u * |partial sum| and a partial sum after k terms is ~ sqrt(k) *
# rms term, so its error is a random walk with sigma ~ u * T / sqrt(6) = 0.41 u T; the maximum of 1e3 - 1e6 such outputs lies at 3.5 - 5
# sigma = 1.4 - 2.1 (3.2 is the largest seen with independent normal data).  8 is twice that: a reference chain past it is not an fp32
# chain of THIS contraction (a wrong gather, a wrong oracle), and FACTOR times it would bound nothing.
RHO_SEQ_SANE = 8.0


def f32_exact(t):
    """fp64 tensor whose values are fp32-representable"""
    return t.float().double()


def scale(op, a, b, bias=None):
    """T of the bilinear operation ``op`` (fp64 tensors in, fp64 tensor out) on operands a, b: (T, K), both shaped like op(a, b).
    bias: a tensor that broadcasts against the output."""
    k = op(torch.ones_like(a), torch.ones_like(b)).round()
    s = op(a * a, b * b)
    t2 = k * s
    if bias is not None:
        t2 = t2 + (bias * bias).expand_as(t2)
    return t2.clamp_min(0).sqrt(), k


def rho(y, y64, t):
    """max_i |y_i - y64_i| / (u T_i); an output with T_i = 0 has no terms and must be exact"""
    y = y.detach().cpu().double()
    assert y.shape == y64.shape == t.shape, (y.shape, y64.shape, t.shape)
    err = (y - y64).abs()
    r = torch.where(t > 0, err / (U * t.clamp_min(1e-300)), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


def rho_seq_sane(t, k, bias=None):
    """what rho_seq of a correct reference chain stays under.  A chain that starts from a bias carries |bias| in every partial sum, but
    T counts the bias once: its K adds round by ~ 0.4 u |bias| each, a walk of 0.4 sqrt(K) u |bias|, 4.5 sigma of it for the maximum
    -> 2 sqrt(K) |bias| / T on top of RHO_SEQ_SANE.  (A wrong gather is off by the size of the result: rho ~ 1 / (u sqrt(K)) > 1e5.)"""
    if bias is None:
        return RHO_SEQ_SANE
    return RHO_SEQ_SANE + float((2.0 * k.sqrt() * bias.abs() / t.clamp_min(1e-300)).max())


def meets(rho_y, rho_seq, sane=RHO_SEQ_SANE):
    return rho_seq <= sane and rho_y <= FACTOR * rho_seq


def chain_matmul(w, c, bias=None, order=None):
    """out[..., m, l] = bias[m] + sum_j w[m, j] * c[..., j, l] as sequential fp32 chains: the product is rounded to fp32, then added to
    the accumulator (two tensor operations: nothing fuses them).  order: the sequence of j (default 0 .. K-1)."""
    w, c = w.float(), c.float()
    m, k = w.shape
    assert c.shape[-2] == k
    wk = w.t().contiguous().unsqueeze(-1)                      # [K, M, 1]
    ck = c.movedim(-2, 0).contiguous().unsqueeze(-2)           # [K, ..., 1, L]
    acc = torch.zeros(c.shape[:-2] + (m, c.shape[-1]), dtype=torch.float32)
    if bias is not None:
        acc += bias.float().view(m, 1)
    for j in (range(k) if order is None else order):
        acc += wk[j] * ck[j]
    return acc


def chain_sum(v, order=None):
    """sequential fp32 sum over the last axis"""
    v = v.float()
    acc = torch.zeros(v.shape[:-1], dtype=torch.float32)
    for j in (range(v.shape[-1]) if order is None else order):
        acc += v[..., j]
    return acc


# ---- gathers of a convolution: x [n, cin, h, w], w_hwio (kh, kw, cin, cout), pads (top, bottom, left, right), dy [n, cout, oh, ow] ----
def conv_pads(h, w, kh, kw, stride, padding):
    """(top, bottom, left, right) of oracle.keras_ops.conv2d's padding argument"""
    from oracle.keras_ops import same_pads
    if padding == "same":
        _, pt, pb = same_pads(h, kh, stride)
        _, pl, pr = same_pads(w, kw, stride)
        return pt, pb, pl, pr
    p = 0 if padding == "valid" else int(padding)
    return p, p, p, p


def _cols(x, kh, kw, stride, pads):
    pt, pb, pl, pr = pads
    return F.unfold(F.pad(x, (pl, pr, pt, pb)), (kh, kw), stride=stride)          # [n, cin*kh*kw, oh*ow], K in (cin, ky, kx) order


def _out_hw(h, w, kh, kw, stride, pads):
    pt, pb, pl, pr = pads
    return (h + pt + pb - kh) // stride + 1, (w + pl + pr - kw) // stride + 1


def conv_fwd_chain(x, w_hwio, bias, stride, pads, order=None):
    """K = cin*kh*kw"""
    kh, kw, cin, cout = w_hwio.shape
    n, _, h, w = x.shape
    oh, ow = _out_hw(h, w, kh, kw, stride, pads)
    wm = w_hwio.permute(3, 2, 0, 1).reshape(cout, -1)
    return chain_matmul(wm, _cols(x.float(), kh, kw, stride, pads), bias, order).view(n, cout, oh, ow)


def conv_dgrad_chain(dy, w_hwio, stride, pads, h, w, bias=None, order=None):
    """dx[ci, iy, ix] = sum_{co, ky, kx} dy[co, (iy + top - ky) / s, (ix + left - kx) / s] * w[ky, kx, ci, co]: the stride-1 correlation of
    the zero-dilated dy with the flipped kernel.  K = cout*kh*kw, the terms between the strides and in the padding being zeros.
    bias [cin]: for the transposed convolution's forward pass, which is this sum."""
    kh, kw, cin, cout = w_hwio.shape
    n, _, oh, ow = dy.shape
    pt, _, pl, _ = pads
    dh, dw = (oh - 1) * stride + 1, (ow - 1) * stride + 1
    d = torch.zeros(n, cout, dh, dw, dtype=torch.float32)
    d[:, :, ::stride, ::stride] = dy.float()
    d = F.pad(d, (kw - 1 - pl, w + pl - dw, kh - 1 - pt, h + pt - dh))            # -> [h + kh - 1, w + kw - 1]
    wm = w_hwio.flip(0, 1).permute(2, 3, 0, 1).reshape(cin, -1)
    return chain_matmul(wm, F.unfold(d, (kh, kw)), bias, order).view(n, cin, h, w)


def conv_wgrad_chain(x, dy, kh, kw, stride, pads, order=None):
    """dw[ky, kx, ci, co] = sum_{n, oy, ox} x[n, ci, oy*s - top + ky, ox*s - left + kx] * dy[n, co, oy, ox].  K = n*oh*ow"""
    n, cin = x.shape[:2]
    cout = dy.shape[1]
    cols = _cols(x.float(), kh, kw, stride, pads).permute(1, 0, 2).reshape(cin * kh * kw, -1)        # [M, n*L]
    d = dy.float().permute(0, 2, 3, 1).reshape(-1, cout)                                              # [n*L, cout]
    return chain_matmul(cols, d, None, order).view(cin, kh, kw, cout).permute(1, 2, 0, 3).contiguous()


# ---- the checks of one layer: {name: dict(y64, t, k, seq, rho_seq)}, everything a kernel's result is held against ----
def vjp(fn, shape, dy):
    """gradient of <fn(p), dy> with respect to p for a LINEAR fn of an fp64 tensor of ``shape`` (so the point does not matter)"""
    p = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(fn(p), p, dy)[0]


def _check(op, a, b, seq, bias=None):
    y64 = op(a, b)
    if bias is not None:
        y64 = y64 + bias
    t, k = scale(op, a, b, bias)
    return dict(y64=y64, t=t, k=int(k.max()), rho_seq=rho(seq, y64, t), sane=rho_seq_sane(t, k, bias))


def _bias_check(dy, dims):
    """db[c] = sum over the batch and the pixels of dy[:, c]: the 'product' is dy * 1, K the number of summands"""
    op = lambda d, one: (d * one).sum(dims)
    moved = dy.movedim(1, 0).reshape(dy.shape[1], -1)
    return _check(op, dy, torch.ones_like(dy), chain_sum(moved))


def conv_checks(x, w_hwio, b, dy, stride, padding):
    """forward, data gradient, weight gradient and bias gradient of oracle.keras_ops.conv2d (fp64, fp32-exact operands)"""
    from oracle import keras_ops as K
    kh, kw = w_hwio.shape[:2]
    n, _, h, w = x.shape
    pads = conv_pads(h, w, kh, kw, stride, padding)
    fwd = lambda a, ww: K.conv2d(a, ww, None, stride, padding)
    dgr = lambda d, ww: vjp(lambda p: fwd(p, ww), x.shape, d)
    wgr = lambda a, d: vjp(lambda p: fwd(a, p), w_hwio.shape, d)
    return {"fwd": _check(fwd, x, w_hwio, conv_fwd_chain(x, w_hwio, b, stride, pads), b.view(1, -1, 1, 1)),
            "dx": _check(dgr, dy, w_hwio, conv_dgrad_chain(dy, w_hwio, stride, pads, h, w)),
            "dw": _check(wgr, x, dy, conv_wgrad_chain(x, dy, kh, kw, stride, pads)),
            "db": _bias_check(dy, (0, 2, 3))}


def convt_checks(x, w_hwoi, b, dy):
    """the same four of oracle.keras_ops.conv2d_transpose_same (stride 2).  It is the data gradient of the stride-2 convolution
    [cout, 2h, 2w] -> [cin, h, w] whose HWIO kernel w_hwoi is, cropped as TF's SAME pads that convolution: its forward chain is that
    convolution's data-gradient chain (K = cin * the taps of the output's phase), its data gradient that convolution's forward chain
    (K = cout*k*k), its weight gradient that convolution's with x and dy exchanged (K = n*h*w)."""
    from oracle import keras_ops as K
    k = w_hwoi.shape[0]
    n, _, h, w = x.shape
    ct = max(k - 2, 0) // 2
    pads = (ct, k - 2 - ct, ct, k - 2 - ct)
    fwd = lambda a, ww: K.conv2d_transpose_same(a, ww, None, 2)
    dgr = lambda d, ww: vjp(lambda p: fwd(p, ww), x.shape, d)
    wgr = lambda a, d: vjp(lambda p: fwd(a, p), w_hwoi.shape, d)
    return {"fwd": _check(fwd, x, w_hwoi, conv_dgrad_chain(x, w_hwoi, 2, pads, 2 * h, 2 * w, b), b.view(1, -1, 1, 1)),
            "dx": _check(dgr, dy, w_hwoi, conv_fwd_chain(dy, w_hwoi, None, 2, pads)),
            "dw": _check(wgr, x, dy, conv_wgrad_chain(dy, x, k, k, 2, pads)),
            "db": _bias_check(dy, (0, 2, 3))}


def dense_checks(x, w_io, b, dy):
    """y = x @ w + b (K = cin), dx = dy @ w^T (K = cout), dw = x^T @ dy and db = sum dy (K = batch)"""
    return {"fwd": _check(lambda a, ww: a @ ww, x, w_io, chain_matmul(w_io.t(), x.t(), b).t(), b.view(1, -1)),
            "dx": _check(lambda d, ww: d @ ww.t(), dy, w_io, chain_matmul(w_io, dy.t()).t()),
            "dw": _check(lambda a, d: a.t() @ d, x, dy, chain_matmul(x.t(), dy)),
            "db": _bias_check(dy, (0,))}


# ---- degraded arithmetic, for the self-test of the metric ----
def cut_mantissa(t, bits):
    """fp32 values rounded to ``bits`` explicit mantissa bits (10: tf32, 7: bf16), round to nearest even; as fp32"""
    t = t.float().contiguous()
    i = t.abs().view(torch.int32).to(torch.int64)
    drop = 23 - bits
    i = (i + ((1 << (drop - 1)) - 1) + ((i >> drop) & 1)) & ~((1 << drop) - 1)
    return torch.copysign(i.to(torch.int32).view(torch.float32), t)


def bf16_split(t):
    """t ~ hi + lo, two bf16-representable fp32 tensors: what a split-bf16 matrix path feeds its instructions.  Its three product
    terms are hi*hi + hi*lo + lo*hi; lo*lo (2^-16 of the product) and what hi + lo misses of t (2^-17) are dropped."""
    t = t.float()
    hi = cut_mantissa(t, 7)
    return hi, cut_mantissa(t - hi, 7)

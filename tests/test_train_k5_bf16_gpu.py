"""bf16 TRAINING of the reference's default generator (make_upscaler_orig with kernel_size=5, upscale_factor=4; reference model.py:267):
the 5x5 bf16 weight gradient (bf16_gwgrad.hip: two tap groups per block pair) straight through the C ABI, the layers built on it
(E.Conv5x5Bf16, E.ConvTBf16), the model in both bf16 modes against the storage-emulating fp64 oracle, the captured train step, and the
learning-phase-0 pass against the inference engine."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err, report

pytestmark = pytest.mark.gpu
TOL_BF16 = 2.0 ** -8
E_WORKSPACE = -4


def _bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _nhwc_bf16(rt, x_nchw):
    """host fp32 NCHW -> device bf16 NHWC (torch's round-to-nearest-even, as the product's conversion kernel)"""
    return x_nchw.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(rt.device)


def _nchw_f64(y_nhwc_bf16):
    return y_nhwc_bf16.cpu().double().permute(0, 3, 1, 2)


def _sync_check(rc, what):
    from upscaler import _lib as L
    L.check(rc, what)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# (a) vcg_conv2d_nhwc_bf16_wgrad, 5x5
# ---------------------------------------------------------------------------------------------------------------
WGRAD_CASES = [
    # cin, cout, stride, n, h, w ('same' padding)
    (64, 64, 1, 1, 5, 7),              # smaller than one tile; every tap partly out of image
    (64, 64, 1, 2, 9, 20),             # ragged in both directions; two column tiles
    (64, 128, 1, 3, 17, 33),           # several tiles, images and co blocks
    (128, 64, 1, 1, 8, 16),            # exactly one tile; two ci blocks
    (64, 64, 2, 1, 8, 8),              # stride 2, even size; TF-SAME pads (1, 2)
    (128, 64, 2, 2, 15, 17),           # stride 2, odd size; pads (2, 2); de-interleaved halo with unequal halves
    (64, 64, 1, 8, 40, 48),            # 120 tiles, every slab of both tap groups busy
    (128, 128, 1, 16, 17, 33),         # 4 block pairs x 2 tap groups leave 32 slabs for 144 ragged tiles: 4-5 tiles per workgroup, the ring wraps
    (128, 128, 2, 4, 64, 48),          # stride 2: 64 tiles of 4 x 16 on 32 slabs, two tiles per workgroup
]


@pytest.mark.parametrize("cin,cout,stride,n,h,w", WGRAD_CASES)
def test_conv5x5_bf16_wgrad_abi(rt, cin, cout, stride, n, h, w):
    """dW and dbias of a 5x5 'same' convolution from bf16 NHWC x and dy against fp64 autograd on the same bf16-rounded operands, to
    1e-4 max-norm (the bound of test_generic_conv_bf16_fwd_dgrad_wgrad), and bit-identical on a second call."""
    from oracle import keras_ops as K
    from upscaler import _engine as E, _lib as L
    k = 5
    oh, pt, _ = E.same_pads(h, k, stride)
    ow, pl, _ = E.same_pads(w, k, stride)
    g = torch.Generator().manual_seed(cin + 3 * cout + 7 * stride + h)
    x = torch.randn(n, cin, h, w, generator=g)
    dy = torch.randn(n, cout, oh, ow, generator=g)
    wr = torch.zeros(k, k, cin, cout, dtype=torch.float64, requires_grad=True)
    br = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    yr = K.conv2d(_bf16_round(x), wr, br, stride, "same")
    assert tuple(yr.shape) == (n, cout, oh, ow)
    (yr * _bf16_round(dy)).sum().backward()

    d = L.ConvDesc(n, cin, h, w, cout, oh, ow, k, k, stride, pt, pl)
    need = rt.lib.vcg_conv2d_nhwc_bf16_wgrad_workspace_bytes(ctypes.byref(d))
    assert need > 0
    xd, dyd = _nhwc_bf16(rt, x), _nhwc_bf16(rt, dy)
    ws = torch.empty(need, dtype=torch.uint8, device=rt.device)
    out = []
    for _ in range(2):
        dw = torch.full((k, k, cin, cout), float("nan"), device=rt.device)
        db = torch.full((cout,), float("nan"), device=rt.device)
        _sync_check(rt.lib.vcg_conv2d_nhwc_bf16_wgrad(ctypes.byref(d), xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), need,
                                                      rt.stream), "vcg_conv2d_nhwc_bf16_wgrad")
        out.append((dw, db))
    e_dw, e_db = rel_err(out[0][0], wr.grad), rel_err(out[0][1], br.grad)
    report("5x5 bf16 wgrad %d->%d s%d n=%d %dx%d: dw=%.2e dbias=%.2e (workspace %d bytes)" % (cin, cout, stride, n, h, w, e_dw, e_db, need))
    assert e_dw < 1e-4 and e_db < 1e-4
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---------------------------------------------------------------------------------------------------------------
# (b) vcg_conv_transpose2d_nhwc_bf16_wgrad, 5x5; (c) E.ConvTBf16 on the same data
# ---------------------------------------------------------------------------------------------------------------
CT_CASES = [(64, 256, 2, 6, 10), (256, 256, 1, 5, 7)]          # cin, cout, n, h, w: the two up-sampling stages of an x4 generator
_ct_cache = {}


def _ct_data(cin, cout, n, h, w, k=5):
    """operands and the fp64 autograd reference of Conv2DTranspose(cout, 5, strides 2, 'same') + LeakyReLU(0.2), computed once"""
    key = (cin, cout, n, h, w, k)
    if key not in _ct_cache:
        from oracle import keras_ops as K
        g = torch.Generator().manual_seed(11 * cin + cout + h)
        x = torch.randn(n, cin, h, w, generator=g)
        wk = torch.randn(k, k, cout, cin, generator=g) * (0.5 / (k * cin ** 0.5))
        bias = torch.randn(cout, generator=g) * 0.3
        dz = torch.randn(n, cout, 2 * h, 2 * w, generator=g)
        xr = _bf16_round(x).requires_grad_(True)
        wr = _bf16_round(wk).requires_grad_(True)
        br = bias.double().requires_grad_(True)
        z = K.conv2d_transpose_same(xr, wr, br, 2)
        gx, gw, gb = torch.autograd.grad((z * _bf16_round(dz)).sum(), [xr, wr, br])
        _ct_cache[key] = dict(x=x, wk=wk, bias=bias, dz=dz, y=K.leaky_relu(z.detach(), 0.2), gx=gx, gw=gw, gb=gb)
    return _ct_cache[key]


@pytest.mark.parametrize("cin,cout,n,h,w", CT_CASES)
def test_conv_transpose5x5_bf16_wgrad_abi(rt, cin, cout, n, h, w):
    """dW of Conv2DTranspose(5, strides 2) against fp64 autograd of K.conv2d_transpose_same to 1e-4; one byte of workspace less is
    VCG_E_WORKSPACE with dw untouched."""
    from upscaler import _lib as L
    D = _ct_data(cin, cout, n, h, w)
    d = L.ConvDesc(n, cin, h, w, cout, 2 * h, 2 * w, 5, 5, 2, 1, 1)
    need = rt.lib.vcg_conv_transpose2d_nhwc_bf16_wgrad_workspace_bytes(ctypes.byref(d))
    assert need > 0
    xd, dzd = _nhwc_bf16(rt, D["x"]), _nhwc_bf16(rt, D["dz"])
    ws = torch.empty(need, dtype=torch.uint8, device=rt.device)
    dw = torch.full((5, 5, cout, cin), float("nan"), device=rt.device)
    rc = rt.lib.vcg_conv_transpose2d_nhwc_bf16_wgrad(ctypes.byref(d), xd.data_ptr(), dzd.data_ptr(), dw.data_ptr(), ws.data_ptr(), need - 1, rt.stream)
    torch.cuda.synchronize()
    assert rc == E_WORKSPACE and bool(torch.isnan(dw).all())
    _sync_check(rt.lib.vcg_conv_transpose2d_nhwc_bf16_wgrad(ctypes.byref(d), xd.data_ptr(), dzd.data_ptr(), dw.data_ptr(), ws.data_ptr(), need, rt.stream),
                "vcg_conv_transpose2d_nhwc_bf16_wgrad")
    e = rel_err(dw, D["gw"])
    report("5x5 bf16 convT wgrad %d->%d n=%d %dx%d: dw=%.2e (workspace %d bytes)" % (cin, cout, n, h, w, e, need))
    assert e < 1e-4


def _bind(rt, layer, weights):
    from upscaler import _engine as E
    ps = E.ParamStore()
    layer.declare(ps)
    ps.materialize(rt)
    layer.bind(rt, ps)
    ps.set_weights({k: v.numpy() for k, v in weights.items()})
    return ps


@pytest.mark.parametrize("cin,cout,n,h,w", CT_CASES)
def test_conv_transpose_bf16_layer(rt, cin, cout, n, h, w):
    """E.ConvTBf16: forward (+ bias + LeakyReLU) and data gradient to 2^-8 (stored in bf16), kernel / bias gradient to 1e-4; with
    input_lrelu_slope the data gradient carries the derivative of the LeakyReLU that produced the layer's input."""
    from upscaler import _engine as E, _lib as L
    D = _ct_data(cin, cout, n, h, w)
    layer = E.ConvTBf16("t", cin, cout, 5, L.ACT_LRELU, 0.2)
    ps = _bind(rt, layer, {"t/kernel": D["wk"], "t/bias": D["bias"]})
    xd = _nhwc_bf16(rt, D["x"])
    y, ctx = layer.forward(xd)
    e_y = rel_err(_nchw_f64(y), D["y"])
    dzd = _nhwc_bf16(rt, D["dz"])
    dx = layer.backward(ctx, dzd, True, True, 0)
    e_dx = rel_err(_nchw_f64(dx), D["gx"])
    e_dw, e_db = rel_err(ps.grad("t/kernel"), D["gw"]), rel_err(ps.grad("t/bias"), D["gb"])
    # the input read as a LeakyReLU(0.2) output: dx *= (x > 0 ? 1 : 0.2); the mask multiplies the stored (bf16) gradient
    dxm = layer.backward(ctx, dzd, True, False, 0, input_lrelu_slope=0.2)
    xr = _bf16_round(D["x"])
    dxf = dx.cpu().float().permute(0, 3, 1, 2)
    want = torch.where(xr > 0, dxf, (dxf * 0.2).to(torch.bfloat16).float())          # fp32 product, one rounding
    assert torch.equal(dxm.cpu().float().permute(0, 3, 1, 2), want)
    report("bf16 convT layer 5x5 %d->%d n=%d %dx%d: fwd=%.2e dgrad=%.2e wgrad=%.2e dbias=%.2e" % (cin, cout, n, h, w, e_y, e_dx, e_dw, e_db))
    assert e_y < TOL_BF16 and e_dx < TOL_BF16
    assert e_dw < 1e-4 and e_db < 1e-4


@pytest.mark.parametrize("k,cin", [(4, 64), (5, 128), (3, 32)])
def test_conv_transpose_bf16_layer_refuses_other_shapes(k, cin):
    from upscaler import _engine as E
    with pytest.raises(NotImplementedError):
        E.ConvTBf16("t", cin, 256, k)


# ---------------------------------------------------------------------------------------------------------------
# (c) E.Conv5x5Bf16
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(2, 9, 20), (1, 5, 7), (3, 40, 72)])
def test_conv5x5_bf16_trunk_layer(rt, n, h, w):
    """forward, forward with the statistics epilogue (or its fall-back), and backward WITH dx_residual: dx = conv data gradient +
    residual, added in fp32 before the one rounding to bf16 -- against fp64 autograd on the bf16-rounded operands to 2^-8; dw / dbias to 1e-4"""
    from oracle import keras_ops as K
    from upscaler import _engine as E
    g = torch.Generator().manual_seed(100 + h)
    wk = torch.randn(5, 5, 64, 64, generator=g) * (2.0 / (25 * 64)) ** 0.5
    bk = torch.randn(64, generator=g) * 0.1
    x, res = torch.randn(n, 64, h, w, generator=g), torch.randn(n, 64, h, w, generator=g)
    dy = torch.randn(n, 64, h, w, generator=g)
    layer = E.Conv5x5Bf16("c")
    ps = _bind(rt, layer, {"c/kernel": wk, "c/bias": bk})
    xr = _bf16_round(x).requires_grad_(True)
    wr = _bf16_round(wk).requires_grad_(True)
    br = bk.double().requires_grad_(True)
    yr = K.conv2d(xr, wr, br, 1, "same")
    (yr * _bf16_round(dy)).sum().backward()
    dx_ref = xr.grad + _bf16_round(res)

    xd = _nhwc_bf16(rt, x)
    y, ctx = layer.forward(xd)
    ys, ctxs, stats = layer.forward_stats(xd, False)
    assert torch.equal(y, ys)                                  # the statistics form stores the same output
    e_y = rel_err(_nchw_f64(y), yr)
    dx = layer.backward(ctx, _nhwc_bf16(rt, dy), True, True, 0, dx_residual=_nhwc_bf16(rt, res))
    e_dx = rel_err(_nchw_f64(dx), dx_ref)
    dx0 = layer.backward(ctxs, _nhwc_bf16(rt, dy), True, False, 0)
    e_dx0 = rel_err(_nchw_f64(dx0), xr.grad)
    e_dw, e_db = rel_err(ps.grad("c/kernel"), wr.grad), rel_err(ps.grad("c/bias"), br.grad)
    if stats is not None:                                      # per-tile partials: their sum is the channel sum of the stored output
        buf, nrec = stats
        s = buf.view(nrec, 2, 64).double().sum(0).cpu()
        yd = y.cpu().double().reshape(-1, 64)
        assert rel_err(s[0], yd.sum(0)) < 1e-5 and rel_err(s[1], (yd * yd).sum(0)) < 1e-5
    report("bf16 5x5 trunk layer n=%d %dx%d: fwd=%.2e dgrad+res=%.2e dgrad=%.2e wgrad=%.2e dbias=%.2e stats=%s"
           % (n, h, w, e_y, e_dx, e_dx0, e_dw, e_db, "epilogue" if stats is not None else "separate pass"))
    assert e_y < TOL_BF16 and e_dx < TOL_BF16 and e_dx0 < TOL_BF16
    assert e_dw < 1e-4 and e_db < 1e-4


# ---------------------------------------------------------------------------------------------------------------
# (d) the model
# ---------------------------------------------------------------------------------------------------------------
def _randomize_bn(G, seed):
    """non-trivial BatchNormalization statistics / affine parameters / PReLU slopes, as after training"""
    rng = np.random.RandomState(seed)
    w = G.get_weights_dict()
    for k, v in w.items():
        if k.endswith("/gamma"):
            w[k] = rng.uniform(0.7, 1.3, v.shape).astype(np.float32)
        elif k.endswith(("/beta", "/moving_mean", "/bias")):
            w[k] = rng.uniform(-0.2, 0.2, v.shape).astype(np.float32)
        elif k.endswith("/moving_variance"):
            w[k] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif k.endswith("/alpha"):
            w[k] = rng.uniform(0.0, 0.3, v.shape).astype(np.float32)
    G.set_weights_dict(w)
    return w


@pytest.mark.parametrize("k,factor,mode", [(5, 4, "bf16+tail"), (5, 2, "bf16"), (3, 4, "bf16+tail"), (5, 2, "bf16+tail")])
def test_k5_x4_generator_training_forward_and_gradients(rt, k, factor, mode):
    """Training-mode forward, MSE loss, every parameter gradient and the moving statistics against the fp64 oracle evaluated with the same
    storage roundings (the yardstick of test_bf16_trunk_generator_training_forward_and_gradients): per tensor
    max(1e-2, 2.5 x that tensor's fp32-vs-fp64 distance under the same emulation) in relative L2.  Numerically-zero gradients are
    excluded by that test's floor; here they may only be the trunk's conv biases in front of a BatchNormalization."""
    from oracle import models as M
    from upscaler import model as PM, _engine as E
    res, n, h, w = 2, 2, 12, 20
    G = PM.make_upscaler_orig((factor * h, factor * w, 3), kernel_size=k, upscale_factor=factor, res_block_num=res, seed=7, trunk_dtype=mode)
    wd = _randomize_bn(G, 5)
    x = (np.random.RandomState(1).randint(0, 256, (n, h, w, 3)) / 127.5 - 1).astype(np.float32)
    t = (np.random.RandomState(2).randint(0, 256, (n, factor * h, factor * w, 3)) / 127.5 - 1).astype(np.float32)

    def oracle(dt):
        leaf = M.to_torch(wd, dt, requires_grad=True)
        yr, upd = M.upscaler_orig_forward(leaf, torch.tensor(x, dtype=dt), True, res, factor, trunk_bf16=True, tail_bf16=mode == "bf16+tail")
        loss = ((yr - torch.tensor(t, dtype=dt)) ** 2).mean()
        names = [kk for kk, v in leaf.items() if v.requires_grad]
        return yr.detach().double(), float(loss.detach()), dict(zip(names, [g.double() for g in torch.autograd.grad(loss, [leaf[kk] for kk in names])])), upd
    yr, lossr, gref, upd = oracle(torch.float64)
    y32, _, g32, _ = oracle(torch.float32)

    y, tape = G.forward(E.to_device_nchw(rt, x), True)
    assert tuple(y.shape) == (n, 3, factor * h, factor * w)
    val, dy = PM._pixel_loss(rt, y, E.to_device_nchw(rt, t), "mse", 1.0)
    G.backward(tape, dy, 0)
    l2 = lambda a, b, floor=0.0: float((a - b).norm() / (b.norm() + floor))
    e_y, e32_y = l2(E.to_nhwc(rt, y).cpu().double(), yr), l2(y32, yr)
    e_loss = abs(float(val.item()) - lossr) / lossr
    gmax = max(float(g.abs().max()) for g in gref.values())
    excluded, failed = [], []
    for kk, b in gref.items():
        a = G.ps.grad(kk).cpu().double()
        floor = 1e-4 * gmax * b.numel() ** 0.5
        real = float(b.norm()) >= floor
        e, e32 = l2(a, b, floor), l2(g32[kk], b, floor)
        report("    k%d x%d %-9s %-40s |g|2=%.2e rel L2 err=%.2e (oracle fp32-vs-fp64, same storage: %.2e)%s"
               % (k, factor, mode, kk, float(b.norm()), e, e32, "" if real else "   [zero gradient: excluded]"))
        if not real:
            excluded.append(kk)
        elif not e < max(1e-2, 2.5 * e32):
            failed.append((kk, e, e32))
    report("generator training pass k%d x%d [%s] vs oracle with the same storage: output err (rel L2)=%.2e (oracle fp32-vs-fp64 %.2e) loss err=%.1e excluded=%s"
           % (k, factor, mode, e_y, e32_y, e_loss, excluded))
    assert not failed, failed
    allowed = set(["prefinal/conv2d/bias"] + ["res_block/%d/conv_%s/bias" % (i, p) for i in range(res) for p in ("pre", "post")])
    assert set(excluded) <= allowed, sorted(set(excluded) - allowed)
    assert e_y < max(1e-3, 2.5 * e32_y) and e_loss < 1e-4, (e_y, e32_y, e_loss)
    sw = G.get_weights_dict()
    for kk, v in upd.items():                          # moving statistics: momentum 0.99, Bessel-corrected variance
        assert np.max(np.abs(sw[kk] - v.detach().numpy())) < 1e-4 * (np.max(np.abs(v.detach().numpy())) + 1e-3), kk


def test_bf16_modes_keep_refusing_other_filter_counts():
    from upscaler import model as PM
    for mode in ("bf16", "bf16+tail"):
        with pytest.raises(NotImplementedError):
            PM.make_upscaler_orig((64, 64, 3), kernel_size=5, filters=32, upscale_factor=4, res_block_num=1, trunk_dtype=mode)
    with pytest.raises(NotImplementedError):
        PM.make_upscaler_orig((64, 64, 3), kernel_size=7, upscale_factor=4, res_block_num=1, trunk_dtype="bf16")


# ---------------------------------------------------------------------------------------------------------------
# (e) the captured train step
# ---------------------------------------------------------------------------------------------------------------
def test_k5_x4_train_step_graph_replay_matches_eager(rt):
    """the reference-default generator ('bf16+tail', 5x5, x4) with the bf16 PatchGAN inside make_and_compile_gan2, 32x32 -> 128x128
    frames: two recorded steps reproduce two eagerly launched ones bit for bit (weights and the four losses) -- the 5x5 operand packs
    are re-derived inside the graph after every Adam update."""
    from upscaler import model as PM, _engine as E
    h, bs = 32, 4

    def run(graph):
        G = PM.make_upscaler_orig((4 * h, 4 * h, 3), kernel_size=5, upscale_factor=4, res_block_num=2, seed=7, trunk_dtype="bf16+tail")
        D = PM.make_discriminator_patchgan_70((4 * h, 4 * h, 3), seed=11, dtype="bf16")
        _, _, gan = PM.make_and_compile_gan2(G, D, (h, h, 3), (4 * h, 4 * h, 3), "mse", 1.0, lambda: PM.WassersteinLosses(), 1e-2,
                                             optimizer=PM.Adam())
        tr = gan.trainer
        rng = np.random.RandomState(5)
        steps = [(E.to_device_nchw(rt, rng.randint(0, 256, (bs, h, h, 3)) / 127.5 - 1),
                  E.to_device_nchw(rt, rng.randint(0, 256, (bs, 4 * h, 4 * h, 3)) / 127.5 - 1)) for _ in range(3)]
        out = []
        if graph:
            tr.capture_train_step(*steps[0])
            for a, b in steps[1:]:
                out.append(tr.train_step_graph(a, b))
        else:
            for a, b in steps:
                out.append(tr.train_step(a, b))
            out = out[1:]
        return out, G.ps.params.clone(), D.ps.params.clone()
    oe, ge, de = run(False)
    og, gg, dg = run(True)
    assert len(og) == 2 and all(len(s) == 4 for s in og)
    assert oe == og, (oe, og)
    assert torch.equal(ge, gg) and torch.equal(de, dg)
    assert all(np.isfinite(v) for step in og for v in step)


# ---------------------------------------------------------------------------------------------------------------
# (f) learning phase 0
# ---------------------------------------------------------------------------------------------------------------
def test_k5_x4_predict_matches_inference_engine(rt):
    """model.predict (learning phase 0 of the 'bf16+tail' model) against model.to_inference_bf16().predict on the same weights.  Both
    launch the same kernels on the same bf16 operand packs -- the 5x5 trunk convolutions with the folded BatchNormalization / PReLU /
    Add epilogue, the generic transposed convolutions, the 9x9 ends -- and differ only in how scale / shift are derived in fp32
    (vcg_bn_fold_batch against vcg_axpby + vcg_norm_finalize): an fp32 rounding of a scale can move an isolated activation across a
    bf16 rounding boundary, one bf16 ulp (2^-8 of that element) which the layers behind it average down.  Bound: 2^-8 of the output
    range in max-norm."""
    from upscaler import model as PM
    n, h, w = 2, 12, 20
    G = PM.make_upscaler_orig((4 * h, 4 * w, 3), kernel_size=5, upscale_factor=4, res_block_num=2, seed=7, trunk_dtype="bf16+tail")
    _randomize_bn(G, 3)
    x = (np.random.RandomState(1).randint(0, 256, (n, h, w, 3)) / 127.5 - 1).astype(np.float32)
    got = G.predict(x)
    ref = G.to_inference_bf16().predict(x)
    assert got.shape == ref.shape == (n, 4 * h, 4 * w, 3)
    e = rel_err(got, ref)
    report("k5 x4 'bf16+tail' predict vs inference engine: max-norm rel err %.2e (bound 2^-8 = %.2e), identical=%s" % (e, TOL_BF16, np.array_equal(got, ref)))
    assert e < TOL_BF16

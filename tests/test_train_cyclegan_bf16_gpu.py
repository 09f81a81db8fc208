"""bf16 TRAINING of make_generator_cyclegan (BASELINE.json north_star's generator): the data gradient of head/conv at 64 channels and
the data gradient with a joining gradient (vcg_conv2d_nhwc_bf16_dgrad_add) straight through the C ABI in guarded arenas, the layers built
on them (E.ConvTBf16 at 128 channels, E.Conv2DBf16 with dx_residual), the model against the storage-emulating fp64 oracle
(tests/_cyclegan_bf16_train_emulation.py), the captured train step, learning phase 0 against the inference engine, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

from _arena import input_arena, output_arena
from _cyclegan_bf16_train_emulation import CASES, FLOOR, N, H, W, RES, allowed_zero_gradients, l2, training_case
from conftest import rel_err, report

pytestmark = pytest.mark.gpu
TOL_BF16 = 2.0 ** -8


def _bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _nhwc_bf16(x_nchw):
    """host fp32 NCHW -> host bf16 NHWC (torch's round-to-nearest-even, as the product's conversion kernel)"""
    return x_nchw.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def _nchw_f64(y_nhwc_bf16):
    return y_nhwc_bf16.cpu().double().permute(0, 3, 1, 2)


def _sync_check(rc, what):
    from upscaler import _lib as L
    L.check(rc, what)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# (i) vcg_conv9x9_to3_bf16_wgrad at cin = 64
# ---------------------------------------------------------------------------------------------------------------
HEAD_WGRAD_CASES = [
    (1, 5, 6),                         # smaller than one tile
    (2, 9, 34),                        # ragged, two column tiles
    (3, 17, 66),
    (8, 40, 48),                       # 160 tiles
    (4, 50, 496),                      # 832 tiles on 256 workgroups: more than three each, the ring of three stages wraps; ragged in both directions
]


@pytest.mark.parametrize("n,h,w", HEAD_WGRAD_CASES)
def test_head_conv_wgrad_c64_abi(rt, n, h, w):
    """dW of Conv2D(3, 9, 'same') on 64 channels from bf16 NHWC x and fp32 NCHW dz against fp64 autograd on the bf16-rounded x and dz, to
    1e-4 max-norm (the bound of test_conv5x5_bf16_wgrad_abi); a second call is bit-identical; guarded arenas with a workspace of exactly
    the queried size: guards untouched, no NaN of an input guard in dW, the inputs unchanged"""
    from oracle import keras_ops as K
    from _arena import workspace_arena
    from upscaler import _lib as L
    g = torch.Generator().manual_seed(9 * h + w)
    x, dz = torch.randn(n, 64, h, w, generator=g), torch.randn(n, 3, h, w, generator=g)
    wr = torch.zeros(9, 9, 64, 3, dtype=torch.float64, requires_grad=True)
    y = K.conv2d(_bf16_round(x), wr, torch.zeros(3, dtype=torch.float64), 1, "same")
    (gw,) = torch.autograd.grad((y * _bf16_round(dz)).sum(), [wr])

    d = L.ConvDesc(n, 64, h, w, 3, h, w, 9, 9, 1, 4, 4)
    need = rt.lib.vcg_conv9x9_to3_bf16_wgrad_workspace_bytes(ctypes.byref(d))
    assert need > 0
    xh = _nhwc_bf16(x)
    a_x, a_dz = input_arena(xh, rt.device, "x"), input_arena(dz, rt.device, "dz")
    out = []
    for fill in (0xFF, 0x3F):                                      # whatever the workspace held before
        a_ws = workspace_arena(need, rt.device, fill=fill)
        a_dw = output_arena((9, 9, 64, 3), torch.float32, rt.device, "dw")
        _sync_check(rt.lib.vcg_conv9x9_to3_bf16_wgrad(ctypes.byref(d), a_x.ptr, a_dz.ptr, a_dw.ptr, a_ws.ptr, need, rt.stream), "vcg_conv9x9_to3_bf16_wgrad")
        for a in (a_x, a_dz, a_ws, a_dw):
            a.check()
        out.append(a_dw.view(torch.float32, (9, 9, 64, 3)).clone())
    assert torch.equal(a_x.view(torch.bfloat16, (n, h, w, 64)).view(torch.int16).cpu(), xh.view(torch.int16))
    assert torch.equal(a_dz.view(torch.float32, (n, 3, h, w)).cpu(), dz)
    assert not bool(torch.isnan(out[0]).any())
    e = rel_err(out[0], gw)
    report("head/conv wgrad 64 -> 3 n=%d %dx%d: dw=%.2e (workspace %d bytes)" % (n, h, w, e, need))
    assert e < 1e-4
    assert torch.equal(out[0], out[1])
    a_dw = output_arena((9, 9, 64, 3), torch.float32, rt.device, "dw")
    rc = rt.lib.vcg_conv9x9_to3_bf16_wgrad(ctypes.byref(d), a_x.ptr, a_dz.ptr, a_dw.ptr, a_ws.ptr, need - 1, rt.stream)
    torch.cuda.synchronize()
    assert rc == -4 and a_dw.untouched()                           # VCG_E_WORKSPACE, dW not written


# ---------------------------------------------------------------------------------------------------------------
# (ii) vcg_conv9x9_to3_bf16_dgrad at cin = 64
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(2, 9, 20), (1, 37, 70)])
def test_head_conv_dgrad_c64_abi(rt, n, h, w):
    """data gradient of Conv2D(3, 9, 'same') on 64 channels -- the stem's 3 -> 64 kernel on the kernel packed with the roles swapped --
    against fp64 autograd on the bf16-rounded dz and kernel, to 2^-8 max-norm (dx is stored in bf16); every buffer in a guarded arena"""
    from oracle import keras_ops as K
    from upscaler import _lib as L
    g = torch.Generator().manual_seed(64 + h)
    wk = torch.randn(9, 9, 64, 3, generator=g) * (1.0 / (81 * 3)) ** 0.5
    dz = torch.randn(n, 3, h, w, generator=g)
    xr = torch.zeros(n, 64, h, w, dtype=torch.float64, requires_grad=True)
    y = K.conv2d(xr, _bf16_round(wk), torch.zeros(3, dtype=torch.float64), 1, "same")
    (gx,) = torch.autograd.grad((y * _bf16_round(dz)).sum(), [xr])

    a_dz, a_w = input_arena(dz, rt.device, "dz"), input_arena(wk, rt.device, "kernel")
    a_wf = output_arena((L.FIRST9X9_WFRAG_BYTES,), torch.uint8, rt.device, "wfrag")
    a_dx = output_arena((n, h, w, 64), torch.bfloat16, rt.device, "dx")
    _sync_check(rt.lib.vcg_pack_conv9x9_3ch_bf16(a_w.ptr, 64, 1, a_wf.ptr, rt.stream), "vcg_pack_conv9x9_3ch_bf16")
    d = L.ConvDesc(n, 64, h, w, 3, h, w, 9, 9, 1, 4, 4)
    _sync_check(rt.lib.vcg_conv9x9_to3_bf16_dgrad(ctypes.byref(d), a_dz.ptr, a_wf.ptr, None, 0.0, a_dx.ptr, rt.stream), "vcg_conv9x9_to3_bf16_dgrad")
    for a in (a_dz, a_w, a_wf, a_dx):
        a.check()
    dx = a_dx.view(torch.bfloat16, (n, h, w, 64))
    assert not bool(torch.isnan(dx.float()).any())
    e = rel_err(_nchw_f64(dx), gx)
    report("head/conv dgrad 64 -> 3 n=%d %dx%d: dx=%.2e" % (n, h, w, e))
    assert e < TOL_BF16


# ---------------------------------------------------------------------------------------------------------------
# (iii) vcg_conv2d_nhwc_bf16_dgrad_add
# ---------------------------------------------------------------------------------------------------------------
DGRAD_ADD_CASES = [
    # channels, n, h, w
    (256, 1, 5, 7),                    # smaller than one tile
    (256, 2, 9, 20),                   # ragged in both directions
    (256, 3, 17, 33),                  # several tiles and images; below the tiled kernel's threshold: the streaming kernel
    (64, 2, 8, 16),                    # two row blocks only
    (256, 4, 35, 45),                  # 80 (tile, channel group) pairs: the LDS-tiled kernel with the residual epilogue, ragged tiles
    (128, 5, 33, 70),                  # the same at n_downsample=1's width: one channel group, three column tiles
]
_dgrad_cache = {}


def _dgrad_data(c, n, h, w):
    """operands and the fp64 reference of the data gradient of a 3x3 'same' c -> c convolution, computed once"""
    key = (c, n, h, w)
    if key not in _dgrad_cache:
        from oracle import keras_ops as K
        g = torch.Generator().manual_seed(3 * c + h)
        wk = torch.randn(3, 3, c, c, generator=g) * (2.0 / (9 * c)) ** 0.5
        dy, res = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g)
        xr = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
        y = K.conv2d(xr, _bf16_round(wk), torch.zeros(c, dtype=torch.float64), 1, "same")
        (gx,) = torch.autograd.grad((y * _bf16_round(dy)).sum(), [xr])
        _dgrad_cache[key] = dict(wk=wk, dy=dy, res=res, gx=gx)
    return _dgrad_cache[key]


@pytest.mark.parametrize("c,n,h,w", DGRAD_ADD_CASES)
def test_dgrad_add_abi(rt, c, n, h, w):
    """dx = bf16(dgrad(dy) + residual) against the fp64 sum to 2^-8 max-norm; with a zero residual bit-equal to
    vcg_conv2d_nhwc_bf16_dgrad; every buffer in a guarded arena (input guards are NaN: an out-of-range read would show in dx)"""
    from upscaler import _engine as E, _lib as L
    D = _dgrad_data(c, n, h, w)
    wd = E.pack_conv_frag_bf16(rt, D["wk"].to(rt.device), 9, c, c, 1)
    a_w = input_arena(wd, rt.device, "wfrag_t")
    a_dy = input_arena(_nhwc_bf16(D["dy"]), rt.device, "dy")
    a_res = input_arena(_nhwc_bf16(D["res"]), rt.device, "dx_residual")
    a_zero = input_arena(torch.zeros(n, h, w, c, dtype=torch.bfloat16), rt.device, "zero residual")
    d = L.ConvDesc(n, c, h, w, c, h, w, 3, 3, 1, 1, 1)
    out = []
    for res in (a_res, a_zero):
        a_dx = output_arena((n, h, w, c), torch.bfloat16, rt.device, "dx")
        _sync_check(rt.lib.vcg_conv2d_nhwc_bf16_dgrad_add(ctypes.byref(d), a_dy.ptr, a_w.ptr, res.ptr, a_dx.ptr, rt.stream), "vcg_conv2d_nhwc_bf16_dgrad_add")
        a_dx.check()
        out.append(a_dx.view(torch.bfloat16, (n, h, w, c)).clone())
    a_dx = output_arena((n, h, w, c), torch.bfloat16, rt.device, "dx")
    _sync_check(rt.lib.vcg_conv2d_nhwc_bf16_dgrad(ctypes.byref(d), a_dy.ptr, a_w.ptr, None, 0.0, a_dx.ptr, rt.stream), "vcg_conv2d_nhwc_bf16_dgrad")
    for a in (a_w, a_dy, a_res, a_zero, a_dx):
        a.check()
    plain = a_dx.view(torch.bfloat16, (n, h, w, c))
    assert not bool(torch.isnan(out[0].float()).any())
    e = rel_err(_nchw_f64(out[0]), D["gx"] + _bf16_round(D["res"]))
    e0 = rel_err(_nchw_f64(plain), D["gx"])
    report("dgrad_add 3x3 %d -> %d n=%d %dx%d: dx+res=%.2e (plain dgrad %.2e) zero residual bit-equal=%s"
           % (c, c, n, h, w, e, e0, torch.equal(out[1].view(torch.int16), plain.view(torch.int16))))
    assert e < TOL_BF16 and e0 < TOL_BF16
    assert torch.equal(out[1].view(torch.int16), plain.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------
# (iv) layers
# ---------------------------------------------------------------------------------------------------------------
def _bind(rt, layer, weights):
    from upscaler import _engine as E
    ps = E.ParamStore()
    layer.declare(ps)
    ps.materialize(rt)
    layer.bind(rt, ps)
    ps.set_weights({k: v.numpy() for k, v in weights.items()})
    return ps


def test_conv_transpose_bf16_layer_128_to_64(rt):
    """E.ConvTBf16 3x3 on 128 input channels without activation (up/1/conv_transp): y and dx to 2^-8 (stored in bf16), kernel and bias
    gradient to 1e-4, against fp64 autograd of K.conv2d_transpose_same on the bf16-rounded operands"""
    from oracle import keras_ops as K
    from upscaler import _engine as E
    cin, cout, k, n, h, w = 128, 64, 3, 2, 6, 10
    g = torch.Generator().manual_seed(11 * cin + cout + h)
    x = torch.randn(n, cin, h, w, generator=g)
    wk = torch.randn(k, k, cout, cin, generator=g) * (0.5 / (k * cin ** 0.5))
    bias = torch.randn(cout, generator=g) * 0.3
    dz = torch.randn(n, cout, 2 * h, 2 * w, generator=g)
    xr, wr, br = _bf16_round(x).requires_grad_(True), _bf16_round(wk).requires_grad_(True), bias.double().requires_grad_(True)
    z = K.conv2d_transpose_same(xr, wr, br, 2)
    gx, gw, gb = torch.autograd.grad((z * _bf16_round(dz)).sum(), [xr, wr, br])

    layer = E.ConvTBf16("t", cin, cout, k)
    ps = _bind(rt, layer, {"t/kernel": wk, "t/bias": bias})
    y, ctx = layer.forward(_nhwc_bf16(x).to(rt.device))
    dx = layer.backward(ctx, _nhwc_bf16(dz).to(rt.device), True, True, 0)
    e_y, e_dx = rel_err(_nchw_f64(y), z.detach()), rel_err(_nchw_f64(dx), gx)
    e_dw, e_db = rel_err(ps.grad("t/kernel"), gw), rel_err(ps.grad("t/bias"), gb)
    report("bf16 convT layer 3x3 %d->%d n=%d %dx%d: fwd=%.2e dgrad=%.2e wgrad=%.2e dbias=%.2e" % (cin, cout, n, h, w, e_y, e_dx, e_dw, e_db))
    assert e_y < TOL_BF16 and e_dx < TOL_BF16
    assert e_dw < 1e-4 and e_db < 1e-4


def test_conv2d_bf16_layer_backward_with_dx_residual(rt):
    """E.Conv2DBf16.backward honours dx_residual: dx = data gradient + residual, one rounding; the parameter gradients are unchanged"""
    from oracle import keras_ops as K
    from upscaler import _engine as E
    c, n, h, w = 256, 2, 9, 20
    D = _dgrad_data(c, n, h, w)
    g = torch.Generator().manual_seed(5)
    x, bk = torch.randn(n, c, h, w, generator=g), torch.randn(c, generator=g) * 0.1
    xr, wr, br = _bf16_round(x).requires_grad_(True), _bf16_round(D["wk"]).requires_grad_(True), bk.double().requires_grad_(True)
    (K.conv2d(xr, wr, br, 1, "same") * _bf16_round(D["dy"])).sum().backward()
    layer = E.Conv2DBf16("c", c, c, 3)
    ps = _bind(rt, layer, {"c/kernel": D["wk"], "c/bias": bk})
    y, ctx = layer.forward(_nhwc_bf16(x).to(rt.device))
    dyd, resd = _nhwc_bf16(D["dy"]).to(rt.device), _nhwc_bf16(D["res"]).to(rt.device)
    dx = layer.backward(ctx, dyd, True, True, 0, dx_residual=resd)
    dx0 = layer.backward(ctx, dyd, True, False, 0)
    e_dx, e_dx0 = rel_err(_nchw_f64(dx), xr.grad + _bf16_round(D["res"])), rel_err(_nchw_f64(dx0), xr.grad)
    e_dw, e_db = rel_err(ps.grad("c/kernel"), wr.grad), rel_err(ps.grad("c/bias"), br.grad)
    report("bf16 Conv2DBf16 256->256 backward with dx_residual: dgrad+res=%.2e dgrad=%.2e wgrad=%.2e dbias=%.2e" % (e_dx, e_dx0, e_dw, e_db))
    assert e_dx < TOL_BF16 and e_dx0 < TOL_BF16 and e_dw < 1e-4 and e_db < 1e-4
    assert not torch.equal(dx, dx0)
    # a stride-2 layer has no joining-gradient form: an error, not a dropped gradient
    down = E.Conv2DBf16("s", 64, 128, 3, 2)
    _bind(rt, down, {"s/kernel": torch.zeros(3, 3, 64, 128), "s/bias": torch.zeros(128)})
    xs = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device=rt.device)
    _, cs = down.forward(xs)
    with pytest.raises(NotImplementedError):
        down.backward(cs, torch.zeros(1, 4, 4, 128, dtype=torch.bfloat16, device=rt.device), True, False, 0, dx_residual=xs)


# ---------------------------------------------------------------------------------------------------------------
# (v) the model
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm,f,down", CASES)
def test_cyclegan_bf16_training_forward_and_gradients(rt, norm, f, down):
    """Training-mode forward, MSE loss, every parameter gradient and (batch norm) the moving statistics against the fp64 oracle evaluated
    with the same storage roundings: per tensor max(1e-2, 2.5 x that tensor's fp32-vs-fp64 distance under the same emulation) in relative
    L2, the yardstick of test_k5_x4_generator_training_forward_and_gradients.  No device-supplied activation masks go to the oracle.
    Numerically-zero gradients are excluded by that test's floor; they may only be biases of convolutions that a norm follows."""
    from upscaler import model as PM, _engine as E
    c = training_case(norm, f, down)
    G = PM.make_generator_cyclegan((f * H, f * W, 3), n_downsample=down, res_block_num=RES, upscale_factor=f, norm=norm, seed=7, dtype="bf16")
    G.set_weights_dict(c["weights"])
    r64, r32 = c["f64"], c["f32"]
    y, tape = G.forward(E.to_device_nchw(rt, c["x"]), True)
    assert tuple(y.shape) == (N, 3, f * H, f * W) and y.dtype == torch.float32
    val, dy = PM._pixel_loss(rt, y, E.to_device_nchw(rt, c["t"]), "mse", 1.0)
    G.backward(tape, dy, 0)
    e_y, e32_y = l2(E.to_nhwc(rt, y).cpu().double(), r64["y"]), l2(r32["y"], r64["y"])
    e_loss = abs(float(val.item()) - r64["loss"]) / r64["loss"]
    gmax = max(float(g.abs().max()) for g in r64["grads"].values())
    excluded, failed = [], []
    for kk, b in r64["grads"].items():
        a = G.ps.grad(kk).cpu().double()
        floor = FLOOR * gmax * b.numel() ** 0.5
        real = float(b.norm()) >= floor
        e, e32 = l2(a, b, floor), l2(r32["grads"][kk], b, floor)
        report("    cyclegan bf16 %-8s x%d down%d %-36s |g|2=%.2e rel L2 err=%.2e (oracle fp32-vs-fp64, same storage: %.2e)%s"
               % (norm, f, down, kk, float(b.norm()), e, e32, "" if real else "   [zero gradient: excluded]"))
        if not real:
            excluded.append(kk)
        elif not e < max(1e-2, 2.5 * e32):
            failed.append((kk, e, e32))
    report("cyclegan bf16 training pass %s x%d down%d vs oracle with the same storage: output err (rel L2)=%.2e (oracle fp32-vs-fp64 %.2e) loss err=%.1e excluded=%s"
           % (norm, f, down, e_y, e32_y, e_loss, excluded))
    assert not failed, failed
    assert set(excluded) <= allowed_zero_gradients(f, down), sorted(set(excluded) - allowed_zero_gradients(f, down))
    assert e_y < max(1e-3, 2.5 * e32_y) and e_loss < 1e-4, (e_y, e32_y, e_loss)
    sw = G.get_weights_dict()
    assert (norm == "batch") == bool(r64["upd"])
    for kk, v in r64["upd"].items():                   # moving statistics: momentum 0.99, Bessel-corrected variance
        assert np.max(np.abs(sw[kk] - v)) < 1e-4 * (np.max(np.abs(v)) + 1e-3), kk


def test_cyclegan_bf16_gradients_reach_both_slots(rt):
    """a data-parallel step reads ps.grad(name, which): the backward pass writes the slot it is asked for"""
    from upscaler import model as PM, _engine as E
    c = training_case(*CASES[0])
    norm, f, down = CASES[0]
    G = PM.make_generator_cyclegan((f * H, f * W, 3), n_downsample=down, res_block_num=RES, upscale_factor=f, norm=norm, seed=7, dtype="bf16")
    G.set_weights_dict(c["weights"])
    got = []
    for which in (0, 1):
        y, tape = G.forward(E.to_device_nchw(rt, c["x"]), True)
        _, dy = PM._pixel_loss(rt, y, E.to_device_nchw(rt, c["t"]), "mse", 1.0)
        G.backward(tape, dy, which)
        got.append({k: G.ps.grad(k, which).clone() for k in c["f64"]["grads"]})
    for k in got[0]:
        assert torch.equal(got[0][k], got[1][k]), k


# ---------------------------------------------------------------------------------------------------------------
# (vi) the captured train step
# ---------------------------------------------------------------------------------------------------------------
def test_cyclegan_bf16_train_step_graph_replay_matches_eager(rt):
    """make_generator_cyclegan(dtype='bf16') with the bf16 PatchGAN inside make_and_compile_gan2, 64x64 -> 128x128 frames, batch 2: two
    recorded steps reproduce two eagerly launched ones bit for bit (weights and the four losses); every value is finite"""
    from upscaler import model as PM, _engine as E
    h, bs = 64, 2

    def run(graph):
        G = PM.make_generator_cyclegan((2 * h, 2 * h, 3), upscale_factor=2, res_block_num=2, dtype="bf16")
        D = PM.make_discriminator_patchgan_70((2 * h, 2 * h, 3), seed=11, dtype="bf16")
        _, _, gan = PM.make_and_compile_gan2(G, D, (h, h, 3), (2 * h, 2 * h, 3), "mse", 1.0, lambda: PM.WassersteinLosses(), 1e-2,
                                             optimizer=PM.Adam())
        tr = gan.trainer
        rng = np.random.RandomState(5)
        steps = [(E.to_device_nchw(rt, rng.randint(0, 256, (bs, h, h, 3)) / 127.5 - 1),
                  E.to_device_nchw(rt, rng.randint(0, 256, (bs, 2 * h, 2 * h, 3)) / 127.5 - 1)) for _ in range(3)]
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
    assert bool(torch.isfinite(gg).all()) and bool(torch.isfinite(dg).all())


# ---------------------------------------------------------------------------------------------------------------
# (vii) learning phase 0
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_cyclegan_bf16_predict_matches_inference_engine(rt, norm):
    """model.predict (learning phase 0 on the bf16 layers) against model.to_inference_bf16().predict on the same weights: the same
    kernels on the same bf16 operand packs; the bound of test_k5_x4_predict_matches_inference_engine, 2^-8 of the output range"""
    from upscaler import model as PM
    f, down = 2, 2
    c = training_case("batch", f, down) if norm == "batch" else None
    G = PM.make_generator_cyclegan((f * H, f * W, 3), n_downsample=down, res_block_num=RES, upscale_factor=f, norm=norm, seed=7, dtype="bf16")
    if c is not None:
        G.set_weights_dict(c["weights"])
    x = (np.random.RandomState(1).randint(0, 256, (N, H, W, 3)) / 127.5 - 1).astype(np.float32)
    got = G.predict(x)
    ref = G.to_inference_bf16().predict(x)
    assert got.shape == ref.shape == (N, f * H, f * W, 3)
    e = rel_err(got, ref)
    report("cyclegan bf16 %s predict vs inference engine: max-norm rel err %.2e (bound 2^-8 = %.2e), identical=%s" % (norm, e, TOL_BF16, np.array_equal(got, ref)))
    assert e < TOL_BF16


# ---------------------------------------------------------------------------------------------------------------
# (viii) refusals
# ---------------------------------------------------------------------------------------------------------------
def test_cyclegan_bf16_refuses_what_fp32_builds(rt):
    from upscaler import model as PM
    for shape, kw in (((16, 24, 3), dict(filters=32)), ((16, 24, 4), {}), ((16, 24, 3), dict(n_downsample=3)), ((16, 24, 3), dict(kernel_size=7))):
        kw = dict({"res_block_num": 1}, **kw)
        with pytest.raises(NotImplementedError, match="filters=64"):
            PM.make_generator_cyclegan(shape, dtype="bf16", **kw)
        G = PM.make_generator_cyclegan(shape, dtype="fp32", **kw)
        assert G.input_shape[-1] == shape[2] and G.output_shape[-1] == 3          # (head/conv always writes RGB)
        assert G.dtype == "fp32" and "dtype" not in G.cyclegan_generator           # the topology record the inference engine keys on is unchanged

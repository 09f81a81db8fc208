"""bf16 trunk TRAINING of make_upscaler_attention (train_gan3.py's default -gm resnet-att): the gate's backward kernel
(vcg_conv_in_gate_bf16_bwd) and the 3-channel weight gradient at 5x5 (vcg_conv3ch_bf16_wgrad) through the C ABI, the layer built on them
(E.GateConvBf16) against the fp32 graph's three nodes, the model (trunk_dtype='bf16') against the storage-emulating fp64 oracle
(tests/_attention_bf16_train_emulation.py), both gradient slots, learning phase 0, the captured train step and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

from _attention_bf16_train_emulation import CASES, FLOOR, N, H, W, RES, allowed_zero_gradients, l2, training_case
from conftest import rel_err, report
from test_infer_attention_bf16_gpu import GATE_SHAPES, TOL_BF16, _ulp_scaled

pytestmark = pytest.mark.gpu


def _r(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _nhwc_bf16(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def _nchw_f64(y_nhwc_bf16):
    return y_nhwc_bf16.cpu().double().permute(0, 3, 1, 2)


def _bits(t):
    return t.view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------
# (i) vcg_conv_in_gate_bf16_bwd
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", GATE_SHAPES)
@pytest.mark.parametrize("k", [3, 5])
def test_conv_in_gate_bf16_bwd(rt, n, h, w, k):
    """dm = bf16(dy s + dres) and da = bf16(dy m s (1 - s)), s = sigmoid(conv(u) + b), against the fp64 formula on the same bf16-rounded
    operands: max-norm relative error < 2^-8 and the ulp-scaled element-wise check < 1 (test_infer_attention_bf16_gpu.py's bounds), with
    and without a joining gradient; a NULL dres gives the bits of a dres of zeros; a second call is bit-identical.  Outputs start as NaN."""
    from oracle import keras_ops as K
    from upscaler import _engine as E, _lib as L
    g = torch.Generator().manual_seed(n * 100000 + h * 1000 + w * 10 + k)
    u = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    # pre-sigmoid values spanning about +-6 (test_conv_in_gate_bf16's scale): s (1 - s) runs from 0.25 down to a few 1e-3
    wk = torch.randn(k, k, 3, 64, generator=g) * (2.5 / (k * k) ** 0.5)
    bias = torch.rand(64, generator=g) * 2 - 1
    m, dy, dres = (torch.randn(n, 64, h, w, generator=g) for _ in range(3))
    ud, bd = u.to(rt.device), bias.to(rt.device)
    wf = E.pack_conv_in_gate_bf16(rt, wk.to(rt.device), 3, k, k, 64)
    md, dyd, drd = (_nhwc_bf16(t).to(rt.device) for t in (m, dy, dres))
    zero = torch.zeros_like(drd)
    d = L.ConvDesc(n, 3, h, w, 64, h, w, k, k, 1, k // 2, k // 2)

    def run(res):
        dm = torch.full((n, h, w, 64), float("nan"), dtype=torch.bfloat16, device=rt.device)
        da = torch.full_like(dm, float("nan"))
        L.check(rt.lib.vcg_conv_in_gate_bf16_bwd(ctypes.byref(d), ud.data_ptr(), wf.data_ptr(), bd.data_ptr(), md.data_ptr(), dyd.data_ptr(),
                                                 None if res is None else res.data_ptr(), dm.data_ptr(), da.data_ptr(), rt.stream),
                "vcg_conv_in_gate_bf16_bwd")
        torch.cuda.synchronize()
        return dm, da
    before = [t.clone() for t in (md, dyd, drd)]
    dm1, da1 = run(drd)
    dm2, da2 = run(drd)
    dm0, da0 = run(None)
    dmz, daz = run(zero)
    for t, b in zip((md, dyd, drd), before):
        assert torch.equal(_bits(t), _bits(b))
    a = K.conv2d(_r(u), _r(wk), bias.double(), 1, "same")
    s = torch.sigmoid(a)
    ref_da = _r(dy) * _r(m) * s * (1 - s)
    sl = s * (1 - s)
    line = "bf16 in-gate bwd k=%d n=%d %dx%d  pre-sigmoid range [%.1f, %.1f]  s(1-s) in [%.1e, %.2f]" % (k, n, h, w, float(a.min()), float(a.max()),
                                                                                                     float(sl.min()), float(sl.max()))
    for name, got, ref in (("dm+dres", dm1, _r(dy) * s + _r(dres)), ("dm", dm0, _r(dy) * s), ("da", da1, ref_da), ("da(no dres)", da0, ref_da)):
        assert not bool(torch.isnan(got.float()).any()), name
        e, ew = rel_err(_nchw_f64(got), ref), _ulp_scaled(_nchw_f64(got), ref)
        line += "  %s err=%.2e ulp-scaled=%.2f" % (name, e, ew)
        assert e < TOL_BF16 and ew < 1.0, (name, e, ew)
    report(line)
    assert torch.equal(_bits(dm1), _bits(dm2)) and torch.equal(_bits(da1), _bits(da2))
    assert torch.equal(_bits(dm0), _bits(dmz)) and torch.equal(_bits(da0), _bits(daz)) and torch.equal(_bits(da0), _bits(da1))


# ---------------------------------------------------------------------------------------------------------------
# (ii) vcg_conv3ch_bf16_wgrad at 5x5
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(2, 9, 20), (1, 37, 70)])
def test_conv3ch_bf16_wgrad_k5(rt, n, h, w):
    """dW and dbias of Conv2D(64, 5, 'same') on the frames from fp32 NCHW x and bf16 NHWC dz against fp64 autograd on the bf16-rounded
    operands, to 1e-4 max-norm (the bound of test_head_conv_wgrad_c64_abi); a second call is bit-identical"""
    from oracle import keras_ops as K
    from upscaler import _lib as L
    g = torch.Generator().manual_seed(5 * h + w)
    x, dz = torch.rand(n, 3, h, w, generator=g) * 2 - 1, torch.randn(n, 64, h, w, generator=g)
    wr = torch.zeros(5, 5, 3, 64, dtype=torch.float64, requires_grad=True)
    br = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    gw, gb = torch.autograd.grad((K.conv2d(_r(x), wr, br, 1, "same") * _r(dz)).sum(), [wr, br])
    d = L.ConvDesc(n, 3, h, w, 64, h, w, 5, 5, 1, 2, 2)
    need = rt.lib.vcg_conv3ch_bf16_wgrad_workspace_bytes(ctypes.byref(d))
    assert need > 0
    xd, dzd = x.to(rt.device), _nhwc_bf16(dz).to(rt.device)
    out = []
    for fill in (0xFF, 0x3F):                                      # whatever the workspace held before
        ws = torch.full((need,), fill, dtype=torch.uint8, device=rt.device)
        dw = torch.full((5, 5, 3, 64), float("nan"), device=rt.device)
        db = torch.full((64,), float("nan"), device=rt.device)
        L.check(rt.lib.vcg_conv3ch_bf16_wgrad(ctypes.byref(d), xd.data_ptr(), dzd.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), need, rt.stream),
                "vcg_conv3ch_bf16_wgrad")
        torch.cuda.synchronize()
        out.append((dw, db))
    e_w, e_b = rel_err(out[0][0], gw), rel_err(out[0][1], gb)
    report("3-channel wgrad 5x5 n=%d %dx%d: dw=%.2e db=%.2e (workspace %d bytes)" % (n, h, w, e_w, e_b, need))
    assert not bool(torch.isnan(out[0][0]).any()) and not bool(torch.isnan(out[0][1]).any())
    assert e_w < 1e-4 and e_b < 1e-4
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---------------------------------------------------------------------------------------------------------------
# (iii) E.GateConvBf16 against the fp32 graph's three nodes (Conv2D, sigmoid gate, Multiply)
# ---------------------------------------------------------------------------------------------------------------
def _bind(rt, layer, weights):
    from upscaler import _engine as E
    ps = E.ParamStore()
    layer.declare(ps)
    ps.materialize(rt)
    layer.bind(rt, ps)
    ps.set_weights({k: v.numpy() for k, v in weights.items()})
    return ps


@pytest.mark.parametrize("k,n,h,w", [(3, 2, 9, 20), (5, 1, 13, 21)])          # w = 21: the weight gradient's fp32 fallback at odd widths
def test_gate_conv_bf16_layer_matches_the_fp32_nodes(rt, k, n, h, w):
    """Both paths get bf16-representable frames, kernel, m, dy and dres, so they multiply the same operands and differ by the bf16 path's
    roundings alone: y, dm (with the joining gradient) and da are stored in bf16 -- 2^-8 max-norm and ulp-scaled < 1 against the fp32
    nodes.  The weight / bias gradient reads da rounded to bf16 where the fp32 path reads it in fp32: per element of dW the difference is
    at most 2^-9 sum |da| |u| (half a bf16 ulp of every da), with sum |da| |u| evaluated by the fp32 kernel on the absolute values, plus
    fp32 summation noise of 1e-5 of that sum."""
    from upscaler import _engine as E, _lib as L
    g = torch.Generator().manual_seed(100 * k + w)
    rb = lambda t: t.to(torch.bfloat16).float()
    u = rb(torch.rand(n, 3, h, w, generator=g) * 2 - 1)
    wk = rb(torch.randn(k, k, 3, 64, generator=g) * (2.5 / (k * k) ** 0.5))
    bias = torch.rand(64, generator=g) * 2 - 1
    m, dy, dres = (rb(torch.randn(n, 64, h, w, generator=g)) for _ in range(3))
    gate = E.GateConvBf16("g", 3, 64, k)
    conv = E.Conv2D("g", 3, 64, k)
    ps_b, ps_f = _bind(rt, gate, {"g/kernel": wk, "g/bias": bias}), _bind(rt, conv, {"g/kernel": wk, "g/bias": bias})
    ud, md, dyd, drd = (t.to(rt.device) for t in (u, m, dy, dres))
    # fp32: attention = conv(u); y = sigmoid(attention) * m; backward of the gate, then of the convolution (no data gradient: u is the input)
    a, cctx = conv.forward(ud)
    y32, da32, dm32 = rt.empty(*md.shape), rt.empty(*md.shape), rt.empty(*md.shape)
    L.check(rt.lib.vcg_sigmoid_gate_fwd(a.data_ptr(), md.data_ptr(), y32.data_ptr(), md.numel(), rt.stream), "vcg_sigmoid_gate_fwd")
    L.check(rt.lib.vcg_sigmoid_gate_bwd(a.data_ptr(), md.data_ptr(), dyd.data_ptr(), da32.data_ptr(), dm32.data_ptr(), md.numel(), rt.stream),
            "vcg_sigmoid_gate_bwd")
    conv.backward(cctx, da32, False, True, 0)
    conv.backward((ud.abs(), None, cctx[2]), da32.abs(), False, True, 1)          # slot 1: sum |da| |u| and sum |da|
    # bf16
    mb = _nhwc_bf16(m).to(rt.device)
    y, ctx = gate.forward(ud, mb)
    assert len(ctx) == 2 and ctx[0] is ud and ctx[1] is mb
    dm = gate.backward(ctx, _nhwc_bf16(dy).to(rt.device), 0, dx_residual=_nhwc_bf16(dres).to(rt.device))
    torch.cuda.synchronize()
    line = "GateConvBf16 k=%d n=%d %dx%d vs fp32 nodes:" % (k, n, h, w)
    for name, got, ref in (("y", y, y32), ("dm", dm, dm32 + drd)):
        e, ew = rel_err(_nchw_f64(got), ref.cpu().double()), _ulp_scaled(_nchw_f64(got), ref.cpu().double())
        line += " %s err=%.2e ulp-scaled=%.2f" % (name, e, ew)
        assert e < TOL_BF16 and ew < 1.0, (name, e, ew)
    for name in ("g/kernel", "g/bias"):
        got, ref, bound = (p.grad(name, s).cpu().double() for p, s in ((ps_b, 0), (ps_f, 0), (ps_f, 1)))
        excess = float(((got - ref).abs() - (2.0 ** -9 + 1e-5) * bound).max())
        line += " d%s max-norm=%.2e worst excess over the bound=%.2e" % (name[2:], rel_err(got, ref), excess)
        assert excess <= 0.0, (name, excess)
    report(line)


# ---------------------------------------------------------------------------------------------------------------
# (iv) the model
# ---------------------------------------------------------------------------------------------------------------
def _model(k, f, **kw):
    from upscaler import model as PM
    return PM.make_upscaler_attention((f * H, f * W, 3), kernel_size=k, upscale_factor=f, res_block_num=RES, seed=7, **kw)


@pytest.mark.parametrize("k,f", CASES)
def test_attention_bf16_training_forward_and_gradients(rt, k, f):
    """Training-mode forward, MSE loss, every parameter gradient and the moving statistics against the fp64 oracle evaluated with the same
    storage roundings: the rule of test_cyclegan_bf16_training_forward_and_gradients unchanged -- per tensor relative L2 below
    max(1e-2, 2.5 x that tensor's fp32-vs-fp64 distance under the same emulation), output below max(1e-3, 2.5 x its own), loss 1e-4, moving
    statistics 1e-4.  No device-supplied activation masks go to the oracle.  Numerically-zero gradients are excluded by that test's floor;
    they may only be biases of convolutions that a BatchNormalization follows."""
    from upscaler import model as PM, _engine as E
    c = training_case(k, f)
    G = _model(k, f, trunk_dtype="bf16")
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
        report("    attention bf16 trunk k%d x%d %-50s |g|2=%.2e rel L2 err=%.2e (oracle fp32-vs-fp64, same storage: %.2e)%s"
               % (k, f, kk, float(b.norm()), e, e32, "" if real else "   [zero gradient: excluded]"))
        if not real:
            excluded.append(kk)
        elif not e < max(1e-2, 2.5 * e32):
            failed.append((kk, e, e32))
    report("attention bf16 trunk training pass k%d x%d vs oracle with the same storage: output err (rel L2)=%.2e (oracle fp32-vs-fp64 %.2e) loss err=%.1e excluded=%s"
           % (k, f, e_y, e32_y, e_loss, excluded))
    assert not failed, failed
    assert set(excluded) <= allowed_zero_gradients(), sorted(set(excluded) - allowed_zero_gradients())
    assert e_y < max(1e-3, 2.5 * e32_y) and e_loss < 1e-4, (e_y, e32_y, e_loss)
    sw = G.get_weights_dict()
    assert len(r64["upd"]) == 2 * (2 * RES + 1)
    for kk, v in r64["upd"].items():                   # moving statistics: momentum 0.99, Bessel-corrected variance
        assert np.max(np.abs(sw[kk] - v)) < 1e-4 * (np.max(np.abs(v)) + 1e-3), kk


def test_attention_bf16_gradients_reach_both_slots(rt):
    """a data-parallel step reads ps.grad(name, which): the backward pass writes the slot it is asked for"""
    from upscaler import model as PM, _engine as E
    k, f = CASES[0]
    c = training_case(k, f)
    G = _model(k, f, trunk_dtype="bf16")
    G.set_weights_dict(c["weights"])
    got = []
    for which in (0, 1):
        G.set_weights_dict(c["weights"])               # (the training forward moves the moving statistics)
        y, tape = G.forward(E.to_device_nchw(rt, c["x"]), True)
        _, dy = PM._pixel_loss(rt, y, E.to_device_nchw(rt, c["t"]), "mse", 1.0)
        G.backward(tape, dy, which)
        got.append({kk: G.ps.grad(kk, which).clone() for kk in c["f64"]["grads"]})
    for kk in got[0]:
        assert torch.equal(got[0][kk], got[1][kk]), kk


@pytest.mark.parametrize("k,f", CASES)
def test_attention_bf16_learning_phase_0(rt, k, f):
    """predict (the same nodes on the moving statistics) against the emulation in inference mode, trunk roundings only: the project's
    3e-2 in relative L2, or 2.5 x the emulation's own fp32-vs-fp64 distance where that is larger; a second predict is bit-identical"""
    c = training_case(k, f)
    G = _model(k, f, trunk_dtype="bf16")
    G.set_weights_dict(c["weights"])
    got = G.predict(c["x"])
    e, e32 = l2(torch.tensor(got).double(), c["f64"]["y0"]), l2(c["f32"]["y0"], c["f64"]["y0"])
    report("attention bf16 trunk k%d x%d learning phase 0 vs emulation: rel L2 %.2e (oracle fp32-vs-fp64 %.2e)" % (k, f, e, e32))
    assert got.shape == (N, f * H, f * W, 3) and e < max(3e-2, 2.5 * e32)
    assert np.array_equal(got, G.predict(c["x"]))
    assert G.get_weights_dict()["after_res/batch_norm/moving_mean"].tolist() == c["weights"]["after_res/batch_norm/moving_mean"].tolist()


def test_attention_bf16_inference_engine_reads_a_bf16_trunk_model(rt):
    """net.attention_generator and to_inference_bf16() on a bf16-trunk model: the engine reads parameters by name, so it computes the bits
    it computes from the fp32 model with the same weights"""
    k, f = CASES[0]
    c = training_case(k, f)
    Gb, Gf = _model(k, f, trunk_dtype="bf16"), _model(k, f)
    assert Gb.attention_generator == Gf.attention_generator and (Gb.trunk_dtype, Gf.trunk_dtype) == ("bf16", "fp32")
    assert list(Gb.get_weights_dict()) == list(Gf.get_weights_dict())          # same names, same order
    for kk, v in Gf.get_weights_dict().items():
        assert np.array_equal(v, Gb.get_weights_dict()[kk]), kk                # same seed, same initial weights
    Gb.set_weights_dict(c["weights"])
    Gf.set_weights_dict(c["weights"])
    assert np.array_equal(Gb.to_inference_bf16().predict(c["x"]), Gf.to_inference_bf16().predict(c["x"]))


# ---------------------------------------------------------------------------------------------------------------
# (v) the captured train step
# ---------------------------------------------------------------------------------------------------------------
def test_attention_bf16_train_step_graph_replay_matches_eager(rt):
    """make_upscaler_attention(trunk_dtype='bf16') with the bf16 PatchGAN inside make_and_compile_gan2, 32x32 -> 64x64 frames, batch 2: two
    recorded steps reproduce two eagerly launched ones bit for bit (weights and the four losses); every value is finite"""
    from upscaler import model as PM, _engine as E
    h, bs = 32, 2

    def run(graph):
        G = PM.make_upscaler_attention((2 * h, 2 * h, 3), kernel_size=3, upscale_factor=2, res_block_num=2, trunk_dtype="bf16")
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
# (vi) refusals
# ---------------------------------------------------------------------------------------------------------------
def test_attention_bf16_refuses_what_fp32_builds(rt):
    from upscaler import model as PM
    for kw in (dict(filters=32), dict(norm="instance"), dict(kernel_size=7), dict(upscale_factor=8)):
        kw = dict({"res_block_num": 1}, **kw)
        with pytest.raises(NotImplementedError, match="filters=64"):
            PM.make_upscaler_attention((32, 48, 3), trunk_dtype="bf16", **kw)
    with pytest.raises(NotImplementedError, match="filters=64"):
        PM.make_upscaler_attention((32, 48, 4), res_block_num=1, trunk_dtype="bf16")
    with pytest.raises(NotImplementedError, match="bf16\\+tail"):
        PM.make_upscaler_attention((32, 48, 3), res_block_num=1, trunk_dtype="bf16+tail")
    with pytest.raises(ValueError):
        PM.make_upscaler_attention((32, 48, 3), res_block_num=1, trunk_dtype="fp16")


def test_attention_fp32_keyword_builds_what_the_default_builds(rt):
    """trunk_dtype='fp32' is today's model: the same node kinds and layer classes, a bit-equal forward"""
    k, f = CASES[0]
    c = training_case(k, f)
    Ga, Gb = _model(k, f), _model(k, f, trunk_dtype="fp32")
    sig = lambda G: [(kind, type(layer).__name__, ins) for kind, layer, ins, _ in G.graph.nodes]
    assert sig(Ga) == sig(Gb) and {kind for kind, _, _ in sig(Ga)} <= {"input", "conv", "norm", "gate", "concat", "resize", "atanh", "convt"}
    Ga.set_weights_dict(c["weights"])
    Gb.set_weights_dict(c["weights"])
    assert np.array_equal(Ga.predict(c["x"]), Gb.predict(c["x"]))

"""Element-wise launches of the fp32 train step that moved into a neighbouring kernel, each against the launches it replaces, BIT FOR BIT
(torch.equal), and against the fp64 oracle:

  (1) vcg_conv2d_fwd_affine + vcg_norm_finalize_batch == vcg_conv2d_fwd -> vcg_norm_finalize (inference form) -> vcg_norm_act_fwd
  (2) vcg_norm_act_bwd (batch mode: the launch that combines the slices also writes the parameter gradients) against fp64, and
      independent of what the workspace held
  (3) UpscalerOrig.predict == its layers called one by one; a captured train step == the eager one, moving statistics loaded between
      two replays included (the batched finalize is inside the graph)

fp64 bound: 1e-3 max-norm relative, the file-wide bound of tests/test_kernels_gpu.py.  A LeakyReLU mask in the final
convolution's data gradient (with a sum-only bias-gradient pass) and the whole norm-backward reduction inside the apply pass were built
with the same bit-equality, measured slower and taken out again; their tests went with them."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err, report

pytestmark = pytest.mark.gpu
TOL = 1e-3


def _dev(rt, t):
    return t.float().contiguous().to(rt.device)


# ---- (1) ---------------------------------------------------------------------------------------------------------------------------
# name: cin, cout, k, n, h, w
AFFINE_SHAPES = {
    "k3_64_17x33": (64, 64, 3, 2, 17, 33),      # 64-column tiles: ragged rows, one column in the second x-tile
    "k3_24to40_17x33": (24, 40, 3, 2, 17, 33),  # channels past cout, and past the end of the bias / scale / shift / slope vectors
    "k3_64_17x30": (64, 64, 3, 2, 17, 30),      # the 32-column instantiation
    "k5_64_9x40": (64, 64, 5, 2, 9, 40),
}
_AFF = {}


def _affine_case(rt, name):
    """operands on the device, the three-launch result for {none, PReLU} x {no residual, residual} and the fp64 references: made once"""
    if name in _AFF:
        return _AFF[name]
    from oracle import keras_ops as K
    from upscaler import _engine as E, _lib as L
    cin, cout, k, n, h, w = AFFINE_SHAPES[name]
    g = torch.Generator().manual_seed(cin * 7 + cout + k + w)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wk = torch.randn(k, k, cin, cout, generator=g, dtype=torch.float64) / np.sqrt(k * k * cin)
    bias = torch.rand(cout, generator=g, dtype=torch.float64) - 0.5
    gamma = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5
    beta = torch.rand(cout, generator=g, dtype=torch.float64) * 2 - 1.2       # a visible share of pre-activations below zero
    mmean = torch.rand(cout, generator=g, dtype=torch.float64) * 0.6 - 0.3
    mvar = torch.rand(cout, generator=g, dtype=torch.float64) * 1.5 + 0.5
    mvar[::5] = torch.tensor([0.0, 1e-7, 1e-5, 3e-4, 1e-3, 0.0, 2e-6, 1e-4] * 8, dtype=torch.float64)[:len(mvar[::5])]   # near 0: eps carries them
    slopes = torch.rand(cout, generator=g, dtype=torch.float64) - 0.4         # both signs
    res = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    d = L.ConvDesc(n, cin, h, w, cout, h, w, k, k, 1, k // 2, k // 2)
    c = dict(d=d, x=_dev(rt, x), w=_dev(rt, wk), bias=_dev(rt, bias), gamma=_dev(rt, gamma), beta=_dev(rt, beta), mmean=_dev(rt, mmean),
             mvar=_dev(rt, mvar), slopes=_dev(rt, slopes), res=_dev(rt, res), shape=(n, cout, h, w))
    # the existing sequence
    z = rt.empty(n, cout, h, w)
    ep = L.Epilogue(c["bias"].data_ptr(), L.ACT_NONE, 0.0, None, None)
    L.check(rt.lib.vcg_conv2d_fwd(ctypes.byref(d), c["x"].data_ptr(), c["w"].data_ptr(), z.data_ptr(), ctypes.byref(ep), rt.stream), "vcg_conv2d_fwd")
    scale, shift, invstd = rt.empty(cout), rt.empty(cout), rt.empty(cout)
    L.check(rt.lib.vcg_norm_finalize(c["mmean"].data_ptr(), c["mvar"].data_ptr(), c["gamma"].data_ptr(), c["beta"].data_ptr(), cout, 1, E.BN_EPS,
                                     scale.data_ptr(), shift.data_ptr(), invstd.data_ptr(), None, None, 0.0, 0, rt.stream), "vcg_norm_finalize")
    c["scale"], c["shift"] = scale, shift
    zr = K.batchnorm(K.conv2d(x, wk, bias, 1, "same"), gamma, beta, mmean, mvar, False)[0]
    c["neg_share"] = float((zr < 0).double().mean())
    c["seq"], c["ref"] = {}, {}
    for act in ("none", "prelu"):
        for with_res in (False, True):
            y = rt.empty(n, cout, h, w)
            L.check(rt.lib.vcg_norm_act_fwd(z.data_ptr(), n, cout, h * w, scale.data_ptr(), shift.data_ptr(), 0,
                                            L.ACT_PRELU if act == "prelu" else L.ACT_NONE, 0.0, c["slopes"].data_ptr() if act == "prelu" else None,
                                            c["res"].data_ptr() if with_res else None, y.data_ptr(), rt.stream), "vcg_norm_act_fwd")
            c["seq"][act, with_res] = y
            r = K.prelu(zr, slopes) if act == "prelu" else zr
            c["ref"][act, with_res] = r + res if with_res else r
    _AFF[name] = c
    return c


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", ["none", "prelu"])
@pytest.mark.parametrize("name", list(AFFINE_SHAPES))
def test_affine_epilogue_has_the_bits_of_conv_then_norm_act(rt, name, act, with_res):
    from upscaler import _engine as E, _lib as L
    c = _affine_case(rt, name)
    n, cout, h, w = c["shape"]
    # the batched finalize writes what vcg_norm_finalize writes (two entries: the second one's slot is checked too)
    buf = rt.empty(2, 2, cout)
    col = lambda t: (ctypes.c_void_p * 2)(t.data_ptr(), t.data_ptr())
    L.check(rt.lib.vcg_norm_finalize_batch(col(c["mmean"]), col(c["mvar"]), col(c["gamma"]), col(c["beta"]), 2, cout, E.BN_EPS, buf[0].data_ptr(),
                                           buf[1].data_ptr(), rt.stream), "vcg_norm_finalize_batch")
    for i in range(2):
        assert torch.equal(buf[0, i], c["scale"]) and torch.equal(buf[1, i], c["shift"])
    y = torch.full((n, cout, h, w), float("nan"), device=rt.device)
    ep = L.Epilogue(c["bias"].data_ptr(), L.ACT_PRELU if act == "prelu" else L.ACT_NONE, 0.0, c["slopes"].data_ptr() if act == "prelu" else None,
                    c["res"].data_ptr() if with_res else None)
    L.check(rt.lib.vcg_conv2d_fwd_affine(ctypes.byref(c["d"]), c["x"].data_ptr(), c["w"].data_ptr(), y.data_ptr(), ctypes.byref(ep),
                                         buf[0, 1].data_ptr(), buf[1, 1].data_ptr(), rt.stream), "vcg_conv2d_fwd_affine")
    seq, ref = c["seq"][act, with_res], c["ref"][act, with_res]
    e_seq, e_new = rel_err(seq, ref), rel_err(y, ref)
    diff = int((y.view(torch.int32) != seq.view(torch.int32)).sum())
    report("fp32 fusions (1) affine %-16s act=%-5s res=%d: words that differ %d, err three launches %.2e fused %.2e, negative share %.2f"
           % (name, act, with_res, diff, e_seq, e_new, c["neg_share"]))
    assert 0.1 < c["neg_share"] < 0.9
    assert e_seq < TOL and e_new < TOL
    assert torch.equal(y, seq)


# ---- (2) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [1, 66, 1024])
@pytest.mark.parametrize("c", [3, 64, 300])
@pytest.mark.parametrize("mode", ["batch", "instance"])
def test_norm_act_bwd_against_fp64_whatever_the_workspace_held(rt, mode, c, hw):
    from upscaler import _engine as E, _lib as L
    n = 3
    inst = mode == "instance"
    eps = E.IN_EPS if inst else E.BN_EPS
    g = torch.Generator().manual_seed(c * 10 + hw)
    x = (torch.randn(n, c, hw, generator=g) * 1.7 + 0.4).double()
    dy = torch.randn(n, c, hw, generator=g).double()
    gamma = None if inst else (torch.rand(c, generator=g) + 0.5).double().requires_grad_(True)
    beta = None if inst else (torch.rand(c, generator=g) - 0.5).double().requires_grad_(True)
    alpha = (torch.rand(c, generator=g) - 0.4).double().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    axes = (2,) if inst else (0, 2)
    mean = xr.mean(axes, keepdim=True)
    var = ((xr - mean) ** 2).mean(axes, keepdim=True)
    z = (xr - mean) / torch.sqrt(var + eps)
    if not inst:
        z = z * gamma.view(1, c, 1) + beta.view(1, c, 1)
    y = torch.clamp(z, min=0) + alpha.view(1, c, 1) * torch.clamp(z, max=0)
    (y * dy).sum().backward()
    rows = n * c if inst else c
    mean_d = _dev(rt, mean.detach().reshape(rows))
    invstd_d = _dev(rt, (1.0 / torch.sqrt(var.detach() + eps)).reshape(rows))
    xd, dyd, ad = _dev(rt, x), _dev(rt, dy), _dev(rt, alpha.detach())
    gd, bd = (None, None) if inst else (_dev(rt, gamma.detach()), _dev(rt, beta.detach()))
    m = L.NORM_INSTANCE if inst else L.NORM_BATCH
    wsn = rt.lib.vcg_norm_act_bwd_workspace_bytes(n, c, hw, m)
    outs = []
    for fill in (0xFF, 0x3F):
        ws = torch.full((wsn,), fill, dtype=torch.uint8, device=rt.device)
        dx = torch.full((n, c, hw), float("nan"), device=rt.device)
        dg, db, da = (torch.full((c,), float("nan"), device=rt.device) for _ in range(3))
        L.check(rt.lib.vcg_norm_act_bwd(xd.data_ptr(), dyd.data_ptr(), n, c, hw, m, mean_d.data_ptr(), invstd_d.data_ptr(),
                                        None if inst else gd.data_ptr(), None if inst else bd.data_ptr(), L.ACT_PRELU, 0.0, ad.data_ptr(), 1,
                                        dx.data_ptr(), None if inst else dg.data_ptr(), None if inst else db.data_ptr(), da.data_ptr(),
                                        ws.data_ptr(), wsn, rt.stream), "vcg_norm_act_bwd")
        outs.append((dx, da) if inst else (dx, da, dg, db))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    refs = [xr.grad, alpha.grad] + ([] if inst else [gamma.grad, beta.grad])
    errs = [rel_err(a, r) for a, r in zip(outs[0], refs)]
    if float(xr.grad.abs().max()) == 0.0:
        # instance norm of one-element planes: xhat is 0 and dx is exactly 0 in fp64, so the max-norm RELATIVE error has no scale; dx is the
        # difference of terms of the size invstd * |dz|, which is what the kernel's rounding is relative to
        scale = float(invstd_d.max()) * float(dy.abs().max())
        errs[0] = float(outs[0][0].abs().max()) / scale
    report("fp32 fusions (2) norm bwd %-8s c=%d hw=%d errs=%s" % (mode, c, hw, ["%.1e" % e for e in errs]))
    assert max(errs) < TOL


# ---- (3) ---------------------------------------------------------------------------------------------------------------------------
def _frames(seed, n, h, w):
    return (np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)) / 127.5 - 1).astype(np.float32)


def _lively(G, seed):
    """non-trivial normalisation parameters, moving statistics and PReLU slopes (both signs)"""
    w = G.get_weights_dict()
    rng = np.random.RandomState(seed)
    for k in w:
        if k.endswith(("/beta", "/bias", "/moving_mean")):
            w[k] = rng.uniform(-0.3, 0.3, w[k].shape).astype(np.float32)
        elif k.endswith(("/gamma", "/moving_variance")):
            w[k] = rng.uniform(0.5, 1.5, w[k].shape).astype(np.float32)
        elif k.endswith("/alpha"):
            w[k] = rng.uniform(-0.2, 0.3, w[k].shape).astype(np.float32)
    G.set_weights_dict(w)


def test_predict_has_the_bits_of_its_layers_one_by_one(rt):
    from upscaler import _engine as E, model as PM
    G = PM.make_upscaler_orig((64, 66, 3), kernel_size=3, upscale_factor=2, res_block_num=2)
    _lively(G, 4)
    x = _frames(1, 2, 32, 33)
    xd = E.to_device_nchw(rt, x)
    h, _ = G.c_init.forward(xd)
    h, _ = G.a_init.forward(h, False)
    skip = h
    for c1, n1, c2, n2 in G.blocks:
        gen = h
        h, _ = c1.forward(h)
        h, _ = n1.forward(h, False)
        h, _ = c2.forward(h)
        h, _ = n2.forward(h, False, residual=gen)
    h, _ = G.c_pre.forward(h)
    h, _ = G.n_pre.forward(h, False, residual=skip)
    for u in G.ups:
        h, _ = u.forward(h)
    want, _ = G.c_fin.forward(h)
    got, _ = G.forward(xd, False)
    diff = int((got.view(torch.int32) != want.view(torch.int32)).sum())
    report("fp32 fusions (3) predict 32x33 x2, 2 blocks: words that differ from the layers one by one %d" % diff)
    assert torch.equal(got, want)
    assert np.array_equal(G.predict(x), E.to_nhwc(rt, want).cpu().numpy())


def _trainer(seed):
    from upscaler import model as PM
    G = PM.make_upscaler_orig((64, 66, 3), kernel_size=3, upscale_factor=2, res_block_num=2, seed=seed)
    D = PM.make_discriminator_patchgan_70((64, 66, 3), seed=seed + 4)
    _, _, gan = PM.make_and_compile_gan2(G, D, (32, 33, 3), (64, 66, 3), "mse", 1.0, lambda: PM.WassersteinLosses(), 1e-2, optimizer=PM.Adam())
    return G, D, gan.trainer


def test_captured_step_replays_the_eager_one_and_sees_loaded_moving_statistics(rt, tmp_path):
    from upscaler import _engine as E
    lr = [E.to_device_nchw(rt, _frames(20 + i, 2, 32, 33)) for i in range(3)]
    hr = [E.to_device_nchw(rt, _frames(30 + i, 2, 64, 66)) for i in range(3)]
    # a state with other weights and moving statistics, from a trainer of its own
    Gs, _, ts = _trainer(17)
    _lively(Gs, 9)
    ts.train_step(lr[2], hr[2])
    path = str(tmp_path / "other.safetensors")
    ts.save_state(path)

    def run(graph):
        G, D, tr = _trainer(7)
        out = []
        if graph:
            tr.capture_train_step(lr[0], hr[0])
            out.append(tr.train_step_graph(lr[1], hr[1]))
            tr.load_state(path)
            out.append(tr.train_step_graph(lr[2], hr[2]))
        else:
            tr._t_dev = torch.tensor([tr.opt.iterations, 0], dtype=torch.int32, device=rt.device)
            tr.train_step(lr[0], hr[0])
            out.append(tr.train_step(lr[1], hr[1]))
            tr.load_state(path)
            out.append(tr.train_step(lr[2], hr[2]))
        return out, G.ps.params.clone(), D.ps.params.clone()

    oe, ge, de = run(False)
    og, gg, dg = run(True)
    report("fp32 fusions (3) graph replay losses %s eager %s" % (og, oe))
    assert oe == og
    assert oe[0] != oe[1]
    assert torch.equal(ge, gg) and torch.equal(de, dg)

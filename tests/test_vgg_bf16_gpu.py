"""VGG19Features(dtype='bf16') and the bf16 branch of the perceptual losses (VGG_LOSS / VGG_MSE_LOSS / VGG_MAE_LOSS,
upscaling/upscaler/model.py:101-157) on the device.  No check here compares a free-running bf16 gradient with the fp64 oracle: 0.3 % of a
layer's ReLU masks flip under the bf16 roundings (tests/test_vgg_bf16_emulation_cpu.py) and the free-running image gradient then differs
from fp64 by 27-40 % in relative L2 whatever the kernels do -- such a test would measure flips.  Instead:

  * forward, per launch: every stored ReLU output (the features are the sixteenth) against the fp64 function of that launch applied to the
    DEVICE's own input tensor -- max-norm relative error < 2^-8 and the ulp-scaled element-wise bar < 1, the per-stored-tensor check of
    tests/test_infer_incep_bf16_gpu.py; the pooling in between is exact and enters through the next layer's input;
  * forward, end to end: features within 2 x d_ref of the fp64 oracle in relative L2, d_ref the emulation's own distance;
  * backward: backward_data on the device's tape against the emulation's UN-rounded fp64 linear backward evaluated on the device's own
    taps -- no flips by construction -- relative L2 below 2 x e_chain, the emulation's gradient-rounding chain error;
  * loss path: _content_loss_and_grad for the three kinds; the value against the fp64 loss of the device's own features plus the fp64
    pixel term (1e-4), dfake against the same teacher-forced backward; the cosine between the free-running dfake and the fp64 oracle's is
    reported, not bounded;
  * a GanTrainer step with VGG_MSE_LOSS(dtype='bf16') on a bf16 and on an fp32 generator: finite losses, and two recorded steps equal two
    eagerly launched ones bit for bit; weights exchange with the fp32 model, a weight change re-packs; unserved shapes raise.
The factor 2 leaves room for the device's fp32 accumulation order on top of the rounding points the emulation has."""
import numpy as np
import pytest
import torch

import _vgg_bf16_emulation as V
from conftest import rel_err, report
from oracle import keras_ops as K, models as M

pytestmark = pytest.mark.gpu
_RUNS = {}


def _say(line):
    print(line)
    report(line)


def _nchw64(t_nhwc):
    return t_nhwc.float().cpu().double().permute(0, 3, 1, 2).contiguous()


def _run(rt, shape):
    """the bf16 extractor on the shape's frames, once per session: (model, features, tape, taps as fp64 NCHW)"""
    if shape not in _RUNS:
        from upscaler import _engine as E, model as PM
        vm = PM.VGG19Features(shape[1:], "random", seed=19, dtype="bf16")
        taps = []
        f, tape = vm.forward(E.to_device_nchw(rt, V.reference(shape)["x"]), training=True, taps=taps)
        assert len(taps) == 16 and len(tape) == 16 and all(a is b for a, b in zip(taps, tape))
        _RUNS[shape] = (vm, f, tape, [_nchw64(t) for t in taps])
    return _RUNS[shape]


def _ulp_scaled(got, ref):
    return float(((got - ref).abs() / (ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max())).max())


@pytest.mark.parametrize("shape", V.SHAPES)
def test_every_stored_tensor_teacher_forced_and_features_end_to_end(rt, shape):
    ref = V.reference(shape)
    vm, f, _, taps = _run(rt, shape)
    n, h, w, _ = shape
    assert f.dtype == torch.bfloat16 and tuple(f.shape) == (n, h // 16, w // 16, 512) and vm.output_shape == (None, h // 16, w // 16, 512)
    wt = ref["w"]
    worst = (0.0, 0.0, None)
    for k, (name, first) in enumerate(V.LAYERS):
        if k == 0:
            inp = V.r_bf16(torch.tensor(ref["x"], dtype=torch.float64).permute(0, 3, 1, 2))
        else:
            inp = torch.nn.functional.max_pool2d(taps[k - 1], 2, 2) if first else taps[k - 1]
        want = torch.relu(K.conv2d(inp, V.r_bf16(wt[name + "/kernel"]), wt[name + "/bias"], 1, "same"))
        assert tuple(taps[k].shape) == tuple(want.shape), name
        e, eu = rel_err(taps[k], want), _ulp_scaled(taps[k], want)
        if eu > worst[1]:
            worst = (e, eu, name)
        assert e < 2.0 ** -8 and eu < 1.0, (name, e, eu)
    d_dev = V.rel_l2(_nchw64(f).permute(0, 2, 3, 1), ref["f_oracle"])
    _say("vgg bf16 %s: worst stored tensor %s max-norm err %.2e ulp-scaled %.2f; features vs fp64 oracle rel L2 %.2e (d_ref %.2e, bound 2 x d_ref)"
         % (shape, worst[2], worst[0], worst[1], d_dev, ref["d_ref"]))
    assert d_dev < 2 * ref["d_ref"]


@pytest.mark.parametrize("shape", V.SHAPES)
def test_backward_data_teacher_forced_on_the_device_taps(rt, shape):
    ref = V.reference(shape)
    vm, f, tape, taps = _run(rt, shape)
    g = torch.Generator().manual_seed(11)
    dz = (torch.randn(f.shape, generator=g) * (f.cpu().float() > 0)).to(torch.bfloat16)          # bf16 NHWC, in front of block5_conv4's ReLU
    dx = vm.backward_data(tape, dz.to(rt.device))
    n, h, w, _ = shape
    assert dx.dtype == torch.float32 and tuple(dx.shape) == (n, 3, h, w)
    want = V.backward(ref["w"], taps, _nchw64(dz), (n, 3, h, w), bf16_kernels=True, round_grads=False)
    e, e_chain = V.rel_l2(dx.cpu(), want), V.chain_error(shape)
    _say("vgg bf16 %s: backward_data vs un-rounded fp64 backward on the device's taps rel L2 %.2e (e_chain %.2e, bound 2 x e_chain)" % (shape, e, e_chain))
    assert float(want.norm()) > 0 and e < 2 * e_chain


@pytest.mark.parametrize("kind", ["vgg", "vgg_mse", "vgg_mae"])
def test_content_loss_and_grad(rt, kind):
    from upscaler import _engine as E, model as PM
    shape = V.SHAPES[1]
    n, h, w, _ = shape
    ref = V.reference(shape)
    vm, f_fake, _, taps = _run(rt, shape)
    img = shape[1:]
    loss_obj = {"vgg": lambda: PM.VGG_LOSS(img, vgg19=vm), "vgg_mse": lambda: PM.VGG_MSE_LOSS(img, 0.1, vgg19=vm),
                "vgg_mae": lambda: PM.VGG_MAE_LOSS(img, 0.1, vgg19=vm, dtype="bf16")}[kind]()
    assert loss_obj.dtype == "bf16" and loss_obj.model is vm
    fake = ref["x"]
    hr = (np.random.RandomState(4).randint(0, 256, shape) / 127.5 - 1).astype(np.float32)
    fake_d, hr_d = E.to_device_nchw(rt, fake), E.to_device_nchw(rt, hr)
    val, dfake = PM._content_loss_and_grad(rt, PM._content_kind(loss_obj.loss), 1.0, fake_d, hr_d)
    assert tuple(val.shape) == (1,) and val.dtype == torch.float32 and dfake.dtype == torch.float32 and tuple(dfake.shape) == (n, 3, h, w)
    # the references, from the device's own features and taps
    f_real, none = vm.forward(hr_d)
    assert none is None
    pk, rate = ("mae" if kind == "vgg_mae" else "mse"), (0.0 if kind == "vgg" else 0.1)
    fr, ff = _nchw64(f_real), _nchw64(f_fake)
    dp = torch.tensor(fake, dtype=torch.float64) - torch.tensor(hr, dtype=torch.float64)
    pix = float((dp * dp).mean() if pk == "mse" else dp.abs().mean())
    dpix = ((2.0 * dp if pk == "mse" else torch.sign(dp)) / dp.numel()).permute(0, 3, 1, 2)
    want_val = V.loss_value(fr, ff, pk) + rate * pix
    want = V.backward(ref["w"], taps, V.loss_grad(fr, ff, pk, 1.0, round_grads=False), (n, 3, h, w), True, False) + rate * dpix
    e_val = abs(float(val.item()) - want_val) / want_val
    e, e_chain = V.rel_l2(dfake.cpu(), want), V.chain_error(shape)
    host = loss_obj.loss(hr, fake)                            # the host-side .loss(y_true, y_pred)
    _say("vgg bf16 content loss %s %s: value %.6g (fp64 of the device's features %.6g, err %.1e; host .loss %.6g) dfake rel L2 %.2e (bound 2 x e_chain = %.2e)"
         % (kind, shape, float(val.item()), want_val, e_val, host, e, 2 * e_chain))
    assert e_val < 1e-4 and abs(host - want_val) / want_val < 1e-4
    assert e < 2 * e_chain
    # reported, not bounded: the free-running gradient against the fp64 oracle's (ReLU / arg-max flips, not kernels, set this figure)
    xt = torch.tensor(fake, dtype=torch.float64, requires_grad=True)
    ht = torch.tensor(hr, dtype=torch.float64)
    df, dq = M.vgg19_block5_conv4(ref["w"], ht) - M.vgg19_block5_conv4(ref["w"], xt), ht - xt
    lo = ((df ** 2).mean() + rate * (dq ** 2).mean()) if pk == "mse" else (df.abs().mean() + rate * dq.abs().mean())
    (g_or,) = torch.autograd.grad(lo, xt)
    a, b = dfake.cpu().double().permute(0, 2, 3, 1).flatten(), g_or.flatten()
    _say("vgg bf16 content loss %s %s: free-running dfake vs the fp64 oracle's: cosine %.4f, rel L2 %.2e; loss %.6g vs %.6g (reported only)"
         % (kind, shape, float(a @ b / (a.norm() * b.norm())), V.rel_l2(a, b), float(val.item()), float(lo.detach())))


def test_weights_exchange_repack_and_predict(rt):
    from upscaler import _engine as E, model as PM
    shape = V.SHAPES[2]
    vm, f, _, _ = _run(rt, shape)
    x = V.reference(shape)["x"]
    v32 = PM.VGG19Features(shape[1:], "random", seed=19)
    w32, w16 = v32.get_weights_dict(), vm.get_weights_dict()
    assert v32.dtype == "fp32" and vm.dtype == "bf16" and vm.count_params() == v32.count_params() == 20024384
    assert list(w32) == list(w16) and all(w32[k].shape == w16[k].shape and np.array_equal(w32[k], w16[k]) for k in w32)
    p = vm.predict(x)                                         # fp32 NHWC, the stored features
    assert p.dtype == np.float32 and p.shape == (shape[0], shape[1] // 16, shape[2] // 16, 512) and np.array_equal(p, f.float().cpu().numpy())
    # new weights: the features change (a stale pack would not), equal a fresh model's, and travel through the fp32 model bit for bit
    new = M.init_vgg19_features(seed=20)
    other = PM.VGG19Features(shape[1:], new, dtype="bf16")
    f_new, _ = other.forward(E.to_device_nchw(rt, x))
    v32.set_weights_dict(new)
    vm.set_weights_dict(v32.get_weights_dict())
    try:
        got = vm.get_weights_dict()
        assert all(np.array_equal(got[k], new[k]) for k in new)
        f2, _ = vm.forward(E.to_device_nchw(rt, x))
        assert not torch.equal(f2, f) and torch.equal(f2, f_new)
    finally:
        vm.set_weights_dict(w16)                              # the shared model goes back to the seed-19 weights
    f3, _ = vm.forward(E.to_device_nchw(rt, x))
    assert torch.equal(f3, f)


def test_refusals(rt):
    from upscaler import model as PM
    for img in ((64, 64, 4), (8, 8, 3)):
        with pytest.raises(NotImplementedError, match="serves frames of 3 channels"):
            PM.VGG19Features(img, "random", dtype="bf16")
        with pytest.raises(NotImplementedError, match="serves frames of 3 channels"):
            PM.VGG_MSE_LOSS(img, 0.1, vgg19="random", dtype="bf16")
    vm = _run(rt, V.SHAPES[2])[0]
    for bad in (rt.empty(1, 4, 32, 32), rt.empty(1, 3, 8, 32)):          # first forward: never a silent fp32 fallback
        with pytest.raises(NotImplementedError, match="serves frames of 3 channels"):
            vm.forward(bad)
    with pytest.raises(ValueError):
        PM.VGG_LOSS(V.SHAPES[2][1:], vgg19=vm, dtype="fp32")             # contradicts the instance's dtype
    with pytest.raises(RuntimeError):
        vm.backward_data(None, torch.zeros(1, 2, 2, 512, dtype=torch.bfloat16, device=rt.device))


@pytest.mark.parametrize("gen", ["bf16", "fp32"])
def test_gan_train_step_with_bf16_vgg_mse_loss(rt, gen):
    """make_and_compile_gan2 with VGG_MSE_LOSS(dtype='bf16') around a bf16 and an fp32 generator (32x32 -> 64x64, PatchGAN critic): the
    four losses are finite and two recorded steps reproduce two eagerly launched ones bit for bit, weights included."""
    from upscaler import model as PM, _engine as E
    h, bs = 32, 2
    loss_obj = PM.VGG_MSE_LOSS((2 * h, 2 * h, 3), 0.1, vgg19="random", dtype="bf16")

    def run(graph):
        G = PM.make_upscaler_orig((2 * h, 2 * h, 3), kernel_size=3, upscale_factor=2, res_block_num=1, seed=7, trunk_dtype=gen)
        D = PM.make_discriminator_patchgan_70((2 * h, 2 * h, 3), seed=11, dtype=gen)
        _, _, gan = PM.make_and_compile_gan2(G, D, (h, h, 3), (2 * h, 2 * h, 3), loss_obj.loss, 1.0, lambda: PM.WassersteinLosses(), 1e-2,
                                             optimizer=PM.Adam())
        tr = gan.trainer
        rng = np.random.RandomState(5)
        steps = [(E.to_device_nchw(rt, rng.randint(0, 256, (bs, h, h, 3)) / 127.5 - 1),
                  E.to_device_nchw(rt, rng.randint(0, 256, (bs, 2 * h, 2 * h, 3)) / 127.5 - 1)) for _ in range(3)]
        if graph:
            tr.capture_train_step(*steps[0])
            out = [tr.train_step_graph(a, b) for a, b in steps[1:]]
        else:
            out = [tr.train_step(a, b) for a, b in steps][1:]
        return out, G.ps.params.clone(), D.ps.params.clone()
    oe, ge, de = run(False)
    og, gg, dg = run(True)
    _say("vgg bf16 train step (%s generator): eager losses %s, recorded %s" % (gen, oe, og))
    assert len(og) == 2 and all(len(s) == 4 and all(np.isfinite(v) for v in s) for s in og)
    assert oe == og, (oe, og)
    assert torch.equal(ge, gg) and torch.equal(de, dg)

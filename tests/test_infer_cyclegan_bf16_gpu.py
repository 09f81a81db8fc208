"""bf16 inference of make_generator_cyclegan (BASELINE.json north_star's generator shape): the one kernel this topology adds -- head/conv on
64 channels, vcg_conv9x9_c64to3_bf16_fwd[_window] -- and Bf16CycleGanGenerator.

Kernel bounds as in test_infer_attention_bf16_gpu.py: fp64 oracle on the SAME bf16-rounded operands, max-norm relative error < 2^-8 and the
ulp-scaled element-wise check < 1, outputs pre-filled with NaN.

The engine's parity check is per layer and teacher-forced: ``forward(x, taps=t)`` hands out every tensor the pass stores, and for each of them
the fp64 layer function applied to the DEVICE'S OWN stored input (bf16-rounded weights, fp64 statistics of the device's z) is the reference,
with the kernel bounds above on every element.  (The "within 2.5x the emulation's fp32-vs-fp64 distance" rule of the other engines' tests is
heavy-tailed for this network: instance norm amplifies single bf16 rounding flips, so that distance is 1.8e-2 ... 2.7e-2 at most shapes but
1.9e-4 at some by luck of the seed, where a product with another summation order would fail for no fault of its own.)  End to end the
output is within 3e-2 in L2 of the plain fp64 oracle -- the project's fixed bf16-vs-fp64 number -- while bf16 storage alone, in exact
arithmetic (tests/_cyclegan_bf16_emulation.py in fp64), accounts for at most 1.5e-2 of it."""
import ctypes

import numpy as np
import pytest
import torch

from _cyclegan_bf16_emulation import cyclegan_forward_emulated
from conftest import rel_err, report

pytestmark = pytest.mark.gpu
TOL_BF16 = 2.0 ** -8


def _bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _to_nhwc_bf16(rt, x):
    from upscaler import _lib as L
    n, c, h, w = x.shape
    y = torch.empty(n, h, w, c, dtype=torch.bfloat16, device=rt.device)
    L.check(rt.lib.vcg_f32_nchw_to_bf16_nhwc(x.data_ptr(), y.data_ptr(), n, c, h, w, rt.stream), "to_bf16")
    return y


def _nchw(y):
    return y.float().permute(0, 3, 1, 2).cpu().double()


def _ulp_scaled(got, ref):
    return float(((got - ref).abs() / (ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max())).max())


def _randomize(w, seed):
    """non-trivial BatchNormalization statistics / affine parameters / PReLU slopes / biases, as after training (the distributions of
    test_infer_attention_bf16_gpu.py's _randomize_bn)"""
    rng = np.random.RandomState(seed)
    for k, v in w.items():
        if k.endswith("/gamma"):
            w[k] = rng.uniform(0.7, 1.3, v.shape).astype(np.float32)
        elif k.endswith(("/beta", "/moving_mean", "/bias")):
            w[k] = rng.uniform(-0.2, 0.2, v.shape).astype(np.float32)
        elif k.endswith("/moving_variance"):
            w[k] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif k.endswith("/alpha"):
            w[k] = rng.uniform(0.0, 0.3, v.shape).astype(np.float32)
    return w


# ---- 1. head/conv on 64 channels ------------------------------------------------------------------------------------------------------
F9_SHAPES = [(1, 1, 1), (1, 9, 70), (2, 40, 130), (1, 140, 66)]         # work item: a 64-column strip x a segment of rows


def _head_operands(rt, n, h, w, tanh):
    from upscaler import _lib as L
    g = torch.Generator().manual_seed(64 * 1000 + h * 10 + w + tanh)
    x = torch.randn(n, 64, h, w, generator=g)
    wk = torch.randn(9, 9, 64, 3, generator=g) * (1.0 / 72)
    bias = torch.randn(3, generator=g) * 0.3
    xd, wd, bd = _to_nhwc_bf16(rt, x.to(rt.device)), wk.to(rt.device), bias.to(rt.device)
    nbytes = rt.lib.vcg_conv9x9_c64to3_bf16_wfrag_bytes()
    assert nbytes == (2304 + 4) * 16
    wf = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=rt.device)
    L.check(rt.lib.vcg_pack_conv9x9_c64to3_bf16(wd.data_ptr(), wf.data_ptr(), rt.stream), "vcg_pack_conv9x9_c64to3_bf16")
    return x, wk, bias, xd, wf, bd, L.ConvDesc(n, 64, h, w, 3, h, w, 9, 9, 1, 4, 4)


@pytest.mark.parametrize("n,h,w", F9_SHAPES)
@pytest.mark.parametrize("tanh", [1, 0])
def test_conv9x9_c64to3_bf16(rt, tanh, n, h, w):
    from oracle import keras_ops as K
    from upscaler import _lib as L
    x, wk, bias, xd, wf, bd, d = _head_operands(rt, n, h, w, tanh)
    y = torch.full((n, 3, h, w), float("nan"), dtype=torch.float32, device=rt.device)
    L.check(rt.lib.vcg_conv9x9_c64to3_bf16_fwd(ctypes.byref(d), xd.data_ptr(), wf.data_ptr(), bd.data_ptr(), tanh, y.data_ptr(), rt.stream),
            "vcg_conv9x9_c64to3_bf16_fwd")
    got = y.cpu().double()
    assert not torch.isnan(got).any()
    ref = K.conv2d(_bf16_round(x), _bf16_round(wk), bias.double(), 1, "same")
    if tanh:
        ref = torch.tanh(ref)
    e, ew = rel_err(got, ref), _ulp_scaled(got, ref)
    report("bf16 conv9x9 64->3 n=%d %dx%d tanh=%d  err=%.2e  elementwise(ulp-scaled)=%.2f" % (n, h, w, tanh, e, ew))
    assert e < TOL_BF16 and ew < 1.0
    # the uint8 form over the whole frame is vcg_nchw_to_frames_u8 of the fp32 form, and its fp32 window form is the fp32 form
    want8 = torch.empty(n, h, w, 3, dtype=torch.uint8, device=rt.device)
    L.check(rt.lib.vcg_nchw_to_frames_u8(y.data_ptr(), want8.data_ptr(), n, h, w, 3, rt.stream), "vcg_nchw_to_frames_u8")
    for kind, want in ((L.OUT_U8_NHWC, want8), (L.OUT_F32_NCHW, y)):
        out = torch.full_like(want, 0xFF) if kind == L.OUT_U8_NHWC else torch.full_like(want, float("nan"))
        L.check(rt.lib.vcg_conv9x9_c64to3_bf16_fwd_window(ctypes.byref(d), xd.data_ptr(), wf.data_ptr(), bd.data_ptr(), tanh, kind, out.data_ptr(),
                                                          0, h, 0, h, rt.stream), "vcg_conv9x9_c64to3_bf16_fwd_window")
        assert torch.equal(out.view(-1).view(torch.uint8), want.view(-1).view(torch.uint8)), kind


@pytest.mark.parametrize("tanh", [1, 0])
def test_conv9x9_c64to3_bf16_windows_are_the_whole_image(rt, tanh):
    """rows (0, h), (3, 11) and (h - 5, 5) at (2, 40, 130): bit-identical to the whole image's rows in both output kinds, placed at y_row0 = 2
    in an image of rows + 5 rows whose other bytes keep their prefill"""
    from upscaler import _lib as L
    n, h, w = 2, 40, 130
    x, wk, bias, xd, wf, bd, d = _head_operands(rt, n, h, w, tanh)
    y = torch.full((n, 3, h, w), float("nan"), dtype=torch.float32, device=rt.device)
    L.check(rt.lib.vcg_conv9x9_c64to3_bf16_fwd(ctypes.byref(d), xd.data_ptr(), wf.data_ptr(), bd.data_ptr(), tanh, y.data_ptr(), rt.stream),
            "vcg_conv9x9_c64to3_bf16_fwd")
    y8 = torch.empty(n, h, w, 3, dtype=torch.uint8, device=rt.device)
    L.check(rt.lib.vcg_nchw_to_frames_u8(y.data_ptr(), y8.data_ptr(), n, h, w, 3, rt.stream), "vcg_nchw_to_frames_u8")
    for row0, rows in ((0, h), (3, 11), (h - 5, 5)):
        y_row0, y_h = 2, rows + 5
        o32 = torch.full((n, 3, y_h, w), float("nan"), dtype=torch.float32, device=rt.device)
        o8 = torch.full((n, y_h, w, 3), 0xA5, dtype=torch.uint8, device=rt.device)
        for kind, out in ((L.OUT_F32_NCHW, o32), (L.OUT_U8_NHWC, o8)):
            L.check(rt.lib.vcg_conv9x9_c64to3_bf16_fwd_window(ctypes.byref(d), xd.data_ptr(), wf.data_ptr(), bd.data_ptr(), tanh, kind, out.data_ptr(),
                                                              row0, rows, y_row0, y_h, rt.stream), "vcg_conv9x9_c64to3_bf16_fwd_window")
        assert torch.equal(o32[:, :, y_row0:y_row0 + rows].view(torch.int32), y[:, :, row0:row0 + rows].view(torch.int32)), (row0, rows)
        assert torch.equal(o8[:, y_row0:y_row0 + rows], y8[:, row0:row0 + rows]), (row0, rows)
        outside = torch.ones(y_h, dtype=torch.bool, device=rt.device)
        outside[y_row0:y_row0 + rows] = False
        assert bool(torch.isnan(o32[:, :, outside]).all()) and bool((o8[:, outside] == 0xA5).all()), (row0, rows)


# ---- 2., 3. the engine -------------------------------------------------------------------------------------------------------------
# norm, kernel_size, upscale_factor, n_downsample, res_block_num, frames, h, w
CASES = [("instance", 3, 1, 2, 2, 2, 16, 24),
         ("instance", 3, 2, 2, 1, 2, 16, 24),
         ("batch", 3, 2, 1, 2, 2, 24, 40),
         ("instance", 5, 1, 2, 1, 2, 16, 24),
         ("instance", 3, 1, 2, 1, 8, 48, 160),
         ("batch", 3, 2, 1, 1, 8, 48, 160)]
_IDS = ["%s-k%d-f%d-nd%d-res%d-n%d-%dx%d" % c for c in CASES]
_RUNS = {}


def _kw(case):
    norm, k, f, nd, res, n, h, w = case
    return dict(filters=64, n_downsample=nd, res_block_num=res, upscale_factor=f, norm=norm, kernel_size=k)


def _weights(case, seed=3):
    """the weights of a case, made on the CPU by the oracle (so that the reference-only distances can be looked at without a device)"""
    from oracle import generators as OG
    norm, k, f, nd, res, n, h, w = case
    return _randomize(OG.init_weights(OG.generator_cyclegan, (h, w, 3), seed, **_kw(case)), seed + 2)


def _frames(case, seed=1):
    norm, k, f, nd, res, n, h, w = case
    return (np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)) / 127.5 - 1).astype(np.float32)


def _build(case, seed=3):
    from upscaler import model as PM
    norm, k, f, nd, res, n, h, w = case
    G = PM.make_generator_cyclegan((f * h, f * w, 3), seed=7, **_kw(case))
    wd = _weights(case, seed)
    assert set(G.get_weights_dict()) == set(wd)
    G.set_weights_dict(wd)
    return G, wd


def _run(rt, case):
    """engine, weights, frames, the tapped eager pass and predict of a case: made once, shared by the tests below, never modified"""
    from upscaler import _engine as E
    if case not in _RUNS:
        G, wd = _build(case)
        assert G.cyclegan_generator == dict(_kw(case), channels=3)
        inf = G.to_inference_bf16()
        x = _frames(case)
        taps = {}
        y = inf.forward(E.to_device_nchw(rt, x), taps=taps)
        torch.cuda.synchronize()
        eager = y.clone()
        _RUNS[case] = (inf, wd, x, taps, eager)
    return _RUNS[case]


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_every_stored_tensor_teacher_forced(rt, case):
    """every tensor the pass stores against the fp64 layer function of the device's own stored input: rel_err < 2^-8 and ulp-scaled < 1 on
    every element; and which statistics path ran"""
    from oracle import keras_ops as K
    from oracle import models as M
    from upscaler import _lib as L
    norm, k, f, nd, res, n, h, w = case
    inf, wd, x, taps, _ = _run(rt, case)
    w64 = M.to_torch(wd, torch.float64)
    rb = _bf16_round

    # the statistics path: the tiled kernel's epilogue records at 48 x 160, the streaming kernel + a statistics pass at the small shapes
    rec = inf.stats_records(n, h, w)
    assert set(rec) == {"down/%d/conv" % i for i in range(nd)} | {"res_block/%d/conv_%s" % (i, p) for i in range(res) for p in ("pre", "post")}
    hh, ww, ci = h, w, 64
    for i in range(nd + 1):
        last = i == nd
        d = L.ConvDesc(n, ci, hh, ww, ci if last else 2 * ci, hh if last else hh // 2, ww if last else ww // 2, k, k, 1 if last else 2,
                       *(K.same_pads(hh, k, 1 if last else 2)[1], K.same_pads(ww, k, 1 if last else 2)[1]))
        q = rt.lib.vcg_conv2d_nhwc_bf16_stats_records(ctypes.byref(d), L.STATS_INSTANCE)
        names = ["res_block/%d/conv_%s" % (j, p) for j in range(res) for p in ("pre", "post")] if last else ["down/%d/conv" % i]
        if (h, w) == (48, 160):
            assert q > 0, (names, q)
        else:
            assert q < 0, (names, q)          # (-3: the streaming kernel serves the shape, the tiled one with the epilogue does not)
        for nm in names:
            assert rec[nm] == (q if norm == "instance" else -1), (nm, rec[nm], q)
        if not last:
            hh, ww, ci = hh // 2, ww // 2, 2 * ci
    if case == ("instance", 3, 1, 2, 1, 8, 48, 160):
        assert (rec["down/0/conv"], rec["down/1/conv"], rec["res_block/0/conv_pre"], rec["res_block/0/conv_post"]) == (9, 4, 4, 4)

    def dev(name):
        t = taps[name]
        return t.cpu().double() if t.dtype == torch.float32 else _nchw(t)

    def nrm(z, name):
        if norm == "instance":
            return K.instancenorm(z)
        return K.batchnorm(z, w64[name + "/gamma"], w64[name + "/beta"], w64[name + "/moving_mean"], w64[name + "/moving_variance"], False)[0]

    layers = [("conv", "stem/conv", "stem/norm", "stem/prelu", 1)]
    layers += [("conv", "down/%d/conv" % i, "down/%d/norm" % i, "down/%d/prelu" % i, 2) for i in range(nd)]
    for i in range(res):
        b = "res_block/%d" % i
        layers += [("conv", b + "/conv_pre", b + "/batch_norm_pre", b + "/prelu", 1), ("conv", b + "/conv_post", b + "/batch_norm_post", b + "/final_add", 1)]
    layers += [("convt", "up/%d/conv_transp" % i, "up/%d/norm" % i, "up/%d/prelu" % i, 2) for i in range(nd + {1: 0, 2: 1, 4: 2}[f])]
    assert list(taps) == [nm for l in layers for nm in (l[1], l[3])] + ["head/conv"]

    worst, checked = (0.0, 0.0, ""), 0

    def check(name, ref):
        nonlocal worst, checked
        got = dev(name)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert not torch.isnan(got).any(), name
        e, ew = rel_err(got, ref), _ulp_scaled(got, ref)
        if ew > worst[1]:
            worst = (e, ew, name)
        checked += got.numel()
        assert e < TOL_BF16 and ew < 1.0, (name, e, ew)

    with torch.no_grad():
        cur, block_in = rb(torch.tensor(x, dtype=torch.float64).permute(0, 3, 1, 2)), None
        for kind, conv, nname, out, stride in layers:
            if conv.endswith("/conv_pre"):
                block_in = cur
            wk, b = rb(w64[conv + "/kernel"]), w64[conv + "/bias"]
            check(conv, K.conv2d_transpose_same(cur, wk, b, 2) if kind == "convt" else K.conv2d(cur, wk, b, stride, "same"))
            z = dev(conv)
            check(out, block_in + nrm(z, nname) if out.endswith("/final_add") else K.prelu(nrm(z, nname), w64[out + "/alpha"]))
            cur = dev(out)
        check("head/conv", torch.tanh(K.conv2d(cur, rb(w64["head/conv/kernel"]), w64["head/conv/bias"], 1, "same")))
    report("bf16 cyclegan per-layer (teacher-forced) %s: %d tensors, %d elements, worst ulp-scaled %.2f (max-norm %.2e) at %s"
           % (_IDS[CASES.index(case)], len(taps), checked, worst[1], worst[0], worst[2]))


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_end_to_end_against_the_fp64_oracle(rt, case):
    """L2 < 3e-2 against the plain fp64 oracle, of which bf16 storage in exact arithmetic (the fp64 emulation) accounts for at most 1.5e-2;
    predict goes through the captured graph: equal to the eager pass and to a second predict, bit for bit"""
    from oracle import generators as OG
    from oracle import models as M
    norm, k, f, nd, res, n, h, w = case
    inf, wd, x, _, eager = _run(rt, case)
    got = inf.predict(x)
    assert got.shape == (n, f * h, f * w, 3) and got.dtype == np.float32
    assert np.array_equal(got, inf.predict(x))                                 # second call: pure graph replay
    assert np.array_equal(got, eager.permute(0, 2, 3, 1).cpu().numpy())        # the graph is the eager pass
    w64, x64 = M.to_torch(wd, torch.float64), torch.tensor(x, dtype=torch.float64)
    with torch.no_grad():
        yp = OG.generator_cyclegan(OG.Net(w64, False), x64, **_kw(case)).numpy()
        ye = cyclegan_forward_emulated(w64, x64, nd, res, f, norm).numpy()
    l2 = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    g = got.astype(np.float64)
    d_ref, e_l2, e_max, e_emul = l2(ye, yp), l2(g, yp), rel_err(g, yp), l2(g, ye)
    report("bf16 cyclegan inference %s: vs fp64 oracle L2 %.2e max-norm %.2e; vs bf16-emulating oracle L2 %.2e; bf16 storage alone "
           "(fp64 emulation vs oracle) L2 %.2e max-norm %.2e" % (_IDS[CASES.index(case)], e_l2, e_max, e_emul, d_ref, rel_err(ye, yp)))
    assert d_ref <= 1.5e-2
    assert e_l2 < 3e-2


# ---- 4. uint8 frames ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[_IDS[0], _IDS[2]])
def test_upscale_frames(rt, case):
    """5 frames in batches of 2 (a ragged last batch): vcg_nchw_to_frames_u8 of replay on the same frames, bit for bit"""
    from upscaler import data as PD
    norm, k, f, nd, res, n, h, w = case
    inf = _run(rt, case)[0]
    u8 = np.random.RandomState(f + 10).randint(0, 256, (5, h, w, 3)).astype(np.uint8)
    want = torch.cat([PD.device_to_frames_u8(inf.replay(PD.frames_u8_to_device(u8[i:i + 2]))) for i in range(0, 5, 2)]).cpu().numpy()
    got = inf.upscale_frames(u8, batch_size=2)
    assert got.dtype == np.uint8 and got.shape == (5, f * h, f * w, 3)
    assert np.array_equal(got, want)
    assert np.array_equal(inf.upscale_frames(u8, batch_size=2), got)              # second call: pure replay
    assert int(got.min()) < int(got.max())                                        # (equal constant frames would show nothing)


# ---- 5. chunking -----------------------------------------------------------------------------------------------------------------------
def test_chunked_launches(rt):
    """the launch limit lowered to two frames' largest tensor: 4 frames run as 2 + 2, the launches of predict on the two halves"""
    case = ("instance", 3, 1, 2, 1, 4, 48, 64)
    G, _ = _build(case)
    x = _frames(case)
    whole = G.to_inference_bf16()
    assert whole._chunk(4, 48, 64) == 4
    halves = np.concatenate([whole.predict(x[:2]), whole.predict(x[2:])], 0)
    chunked = G.to_inference_bf16()
    per = 48 * 64 * 64 * 2                   # stem/conv's output and head/conv's input, the largest tensors of a frame
    chunked.LAUNCH_LIMIT = 2 * per
    assert chunked._chunk(4, 48, 64) == 2 and chunked._chunk(3, 48, 64) == 2 and chunked._chunk(5, 48, 64) == 2
    assert np.array_equal(chunked.predict(x, batch_size=4), halves)
    # one frame that does not fit is refused
    chunked.LAUNCH_LIMIT = per - 1
    with pytest.raises(NotImplementedError, match="fits a launch"):
        chunked.predict(x[:1])


# ---- 6. refresh ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_refresh_after_a_weight_update(rt, norm):
    case = (norm, 3, 2, 1, 1, 2, 16, 24)
    G, wd = _build(case, seed=3)
    x = _frames(case)
    inf = G.to_inference_bf16()
    before = inf.predict(x)
    G.set_weights_dict(_weights(case, seed=11))
    inf.refresh()
    after = inf.predict(x)
    assert not np.array_equal(after, before)
    assert np.array_equal(after, G.to_inference_bf16().predict(x))


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refuses_unserved_topologies(rt):
    from upscaler import model as PM
    for kw in ({"filters": 32}, {"n_downsample": 3}):
        G = PM.make_generator_cyclegan((16, 24, 3), **dict({"res_block_num": 1}, **kw))
        with pytest.raises(NotImplementedError, match="filters=64"):
            G.to_inference_bf16()
    G = PM.make_generator_cyclegan((16, 24, 1), res_block_num=1)
    with pytest.raises(NotImplementedError, match="RGB"):
        G.to_inference_bf16()
    inf = _run(rt, CASES[0])[0]
    with pytest.raises(NotImplementedError, match="row bands"):
        inf.predict(_frames(CASES[0]), band_rows=4)
    with pytest.raises(NotImplementedError, match="row bands"):
        inf.upscale_frames(np.zeros((1, 16, 24, 3), np.uint8), band_rows=4)
    assert not hasattr(PM.make_upscaler_orig_functional((48, 64, 3), kernel_size=3, upscale_factor=2, res_block_num=1), "cyclegan_generator")

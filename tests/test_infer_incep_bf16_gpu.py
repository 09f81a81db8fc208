"""bf16 inference of make_upscaler_incep_resnet (train_gan3.py's -gm inc-resnet): ``G.to_inference_bf16()`` = Bf16IncepResnetGenerator.

Per case, with weights randomised as tests/test_generators_gpu.py's _randomise does:
  * every tensor the pass stores (``forward(x, taps=t)``) against the fp64 function of ONE launch applied to the device's own stored input
    (tests/_incep_bf16_emulation.py: layer_plan): max-norm relative error < 2^-8 and the ulp-scaled element-wise check < 1, the bars of
    tests/test_infer_cyclegan_bf16_gpu.py; padded channels of 19-, 25- and 48-channel tensors are exact zeros;
  * predict (the captured graph) equal bit for bit to the eager pass and to a second predict;
  * upscale_frames equal to predict quantised by upscaling/upscaler/data.py:266-270's rule; refresh() after a weight change; fp32 G.predict
    unchanged by building and running the engine;
  * end to end, computed here: d_ref = L2(fp64 emulation, fp64 oracle), the distance of the rounding points alone, must stay <= 1.5e-2 (the
    cap of the cyclegan test), and the device's L2 against the fp64 oracle <= 2 * d_ref -- one d_ref of margin for rounding flips from the
    fp32 accumulation order (on the CPU an fp32-accumulating twin of the emulation differed from it by about half a d_ref).

Cases (a / b / c blocks, upscale_factor, frames, h x w): 3-path k3 + 2-path k7 + 2-path k3, x2, 2 frames of 20x36; 2-path k5 + 3-path k5 +
2-path with c_block_kernel = 5 (the keyword is both group c's kernel and the kernel of prefinal/conv2d and the tail), x4, 1 frame of 16x24; the
first again at 1x48x160, where tiles are crossed; one with a_block_num = 0."""
import numpy as np
import pytest
import torch

import _incep_bf16_emulation as EM
from conftest import rel_err, report

pytestmark = pytest.mark.gpu
TOL_BF16 = 2.0 ** -8

_K1 = dict(a_block_type="3path", a_block_num=1, a_block_kernel=3, b_block_type="2path", b_block_num=1, b_block_kernel=7,
           c_block_type="2path", c_block_num=1, c_block_kernel=3, upscale_factor=2)
_K2 = dict(a_block_type="2path", a_block_num=1, a_block_kernel=5, b_block_type="3path", b_block_num=1, b_block_kernel=5,
           c_block_type="2path", c_block_num=1, c_block_kernel=5, upscale_factor=4)
_K4 = dict(a_block_type="3path", a_block_num=0, a_block_kernel=3, b_block_type="2path", b_block_num=1, b_block_kernel=7,
           c_block_type="3path", c_block_num=1, c_block_kernel=3, upscale_factor=2)
CASES = {"3p3-2p7-2p3-x2-n2-20x36": (_K1, 2, 20, 36), "2p5-3p5-2p5-x4-n1-16x24": (_K2, 1, 16, 24), "3p3-2p7-2p3-x2-n1-48x160": (_K1, 1, 48, 160),
         "none-2p7-3p3-x2-n1-12x20": (_K4, 1, 12, 20)}
_RUNS = {}


def _randomise(gw, seed):
    rng = np.random.RandomState(seed)
    for n_, v in gw.items():                              # non-trivial BN / PReLU parameters (tests/test_generators_gpu.py)
        if n_.endswith(("/bias", "/beta", "/moving_mean")):
            gw[n_] = rng.uniform(-0.1, 0.1, v.shape).astype(np.float32)
        elif n_.endswith(("/gamma", "/moving_variance")):
            gw[n_] = rng.uniform(0.8, 1.2, v.shape).astype(np.float32)
        elif n_.endswith("/alpha"):
            gw[n_] = rng.uniform(0.0, 0.3, v.shape).astype(np.float32)
    return gw


def _weights(cid, seed=3):
    from oracle import generators as OG
    kw, n, h, w = CASES[cid]
    return _randomise(OG.init_weights(OG.upscaler_incep_resnet, (h, w, 3), seed, filters=64, **kw), seed + 1)


def _frames(cid, seed=1):
    kw, n, h, w = CASES[cid]
    return (np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)) / 127.5 - 1).astype(np.float32)


def _build(cid, seed=3):
    from upscaler import model as PM
    kw, n, h, w = CASES[cid]
    f = kw["upscale_factor"]
    G = PM.make_upscaler_incep_resnet((f * h, f * w, 3), filters=64, **kw)
    wd = _weights(cid, seed)
    assert set(G.get_weights_dict()) == set(wd)
    G.set_weights_dict(wd)
    return G, wd


def _run(rt, cid):
    """model, engine, weights, frames, the fp32 predict before the engine existed, the tapped eager pass: made once per case, never modified"""
    from upscaler import _engine as E
    if cid not in _RUNS:
        G, wd = _build(cid)
        x = _frames(cid)
        fp32_before = G.predict(x)
        assert G.incep_resnet_generator == dict(CASES[cid][0], filters=64, channels=3)
        inf = G.to_inference_bf16()
        taps = {}
        y = inf.forward(E.to_device_nchw(rt, x), taps=taps)
        torch.cuda.synchronize()
        _RUNS[cid] = (G, inf, wd, x, fp32_before, taps, y.clone())
    return _RUNS[cid]


def _ulp_scaled(got, ref):
    return float(((got - ref).abs() / (ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max())).max())


@pytest.mark.parametrize("cid", list(CASES))
def test_every_stored_tensor_teacher_forced(rt, cid):
    from oracle import models as M
    kw, n, h, w = CASES[cid]
    G, inf, wd, x, _, taps, _ = _run(rt, cid)
    w64 = M.to_torch(wd, torch.float64)
    plan = EM.layer_plan(w64, torch.tensor(x, dtype=torch.float64), **kw)
    assert [name for name, _ in plan] == list(taps)          # every stored tensor, in launch order
    blocks = EM.block_names(**kw)
    assert inf.launches() == 1 + sum(5 if b[1] == "3path" else 4 for b in blocks) + 1 + len(inf.ups) + 1
    dev, worst, checked = {}, (0.0, 0.0, ""), 0
    with torch.no_grad():
        for name, fn in plan:
            ref = fn(dev)
            t = taps[name]
            if t.dtype == torch.float32:          # final/conv: fp32 NCHW
                got = t.cpu().double()
            else:                                 # bf16 NHWC, channels padded with zeros to a multiple of 32
                full = t.float().cpu()
                c = ref.shape[1]
                assert full.shape[3] == (c + 31) // 32 * 32, name
                assert bool((full[..., c:] == 0).all()), "%s: padded channels are not zero" % name
                got = full[..., :c].permute(0, 3, 1, 2).double()
            assert got.shape == ref.shape, (name, got.shape, ref.shape)
            assert not torch.isnan(got).any(), name
            e, ew = rel_err(got, ref), _ulp_scaled(got, ref)
            if ew > worst[1]:
                worst = (e, ew, name)
            checked += got.numel()
            assert e < TOL_BF16 and ew < 1.0, (name, e, ew)
            dev[name] = got
    report("bf16 inc-resnet per-launch (teacher-forced) %s: %d tensors, %d elements, worst ulp-scaled %.2f (max-norm %.2e) at %s"
           % (cid, len(taps), checked, worst[1], worst[0], worst[2]))


@pytest.mark.parametrize("cid", list(CASES))
def test_end_to_end_and_graph(rt, cid):
    from oracle import generators as OG, models as M
    kw, n, h, w = CASES[cid]
    f = kw["upscale_factor"]
    G, inf, wd, x, fp32_before, _, eager = _run(rt, cid)
    got = inf.predict(x)
    assert got.shape == (n, f * h, f * w, 3) and got.dtype == np.float32
    assert np.array_equal(got, inf.predict(x))                                 # second call: pure graph replay
    assert np.array_equal(got, eager.permute(0, 2, 3, 1).cpu().numpy())        # the graph is the eager pass
    assert np.array_equal(G.predict(x), fp32_before)                           # the fp32 model is untouched by the engine
    w64, x64 = M.to_torch(wd, torch.float64), torch.tensor(x, dtype=torch.float64)
    with torch.no_grad():
        yp = OG.upscaler_incep_resnet(OG.Net(w64, False), x64, filters=64, **kw).numpy()
        ye = EM.incep_forward_emulated(w64, x64, bf16=True, filters=64, **kw).numpy()
    l2 = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    g = got.astype(np.float64)
    d_ref, e_l2 = l2(ye, yp), l2(g, yp)
    report("bf16 inc-resnet inference %s: vs fp64 oracle L2 %.2e max-norm %.2e; vs bf16-emulating oracle L2 %.2e; rounding points alone "
           "(fp64 emulation vs oracle) d_ref %.2e; fp32 predict vs oracle L2 %.2e" % (cid, e_l2, rel_err(g, yp), l2(g, ye), d_ref,
                                                                                      l2(fp32_before.astype(np.float64), yp)))
    assert d_ref <= 1.5e-2
    assert e_l2 <= 2 * d_ref


@pytest.mark.parametrize("cid", ["3p3-2p7-2p3-x2-n2-20x36", "2p5-3p5-2p5-x4-n1-16x24"])
def test_upscale_frames(rt, cid):
    """5 frames in batches of 2 (a ragged last batch): vcg_nchw_to_frames_u8 (data.py:266-270's rule) of replay on the same frames, bit for bit"""
    from upscaler import data as PD
    kw, n, h, w = CASES[cid]
    f = kw["upscale_factor"]
    inf = _run(rt, cid)[1]
    u8 = np.random.RandomState(f + 10).randint(0, 256, (5, h, w, 3)).astype(np.uint8)
    want = torch.cat([PD.device_to_frames_u8(inf.replay(PD.frames_u8_to_device(u8[i:i + 2]))) for i in range(0, 5, 2)]).cpu().numpy()
    got = inf.upscale_frames(u8, batch_size=2)
    assert got.dtype == np.uint8 and got.shape == (5, f * h, f * w, 3)
    assert np.array_equal(got, want)
    assert np.array_equal(inf.upscale_frames(u8, batch_size=2), got)              # second call: pure replay
    assert int(got.min()) < int(got.max())
    # row bands are the inherited tail's: the same frames, bit for bit
    assert np.array_equal(inf.upscale_frames(u8, batch_size=2, band_rows=7), got)


def test_refresh_after_a_weight_update(rt):
    cid = "none-2p7-3p3-x2-n1-12x20"
    G, _ = _build(cid, seed=3)
    x = _frames(cid)
    inf = G.to_inference_bf16()
    before = inf.predict(x)
    G.set_weights_dict(_weights(cid, seed=11))
    inf.refresh()
    after = inf.predict(x)
    assert not np.array_equal(after, before)
    assert np.array_equal(after, G.to_inference_bf16().predict(x))


def test_refuses_unserved_topologies(rt):
    from upscaler import model as PM
    for kw in ({"filters": 32}, {"upscale_factor": 1}, {"a_block_kernel": 7}):
        G = PM.make_upscaler_incep_resnet((16, 24, 3), **dict(dict(a_block_num=1, b_block_num=0, c_block_num=0, upscale_factor=2), **kw))
        with pytest.raises(NotImplementedError, match="filters=64"):
            G.to_inference_bf16()
    assert not hasattr(PM.make_upscaler_orig_functional((48, 64, 3), kernel_size=3, upscale_factor=2, res_block_num=1), "incep_resnet_generator")

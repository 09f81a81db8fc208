"""uint8 frames in and out of the bf16 inference engines, and the row-banded tail.

The yardstick everywhere is the path that existed before: vcg_conv9x9_to3_bf16_fwd for the window kernel, vcg_nchw_to_frames_u8 for the
uint8 conversion, the unbanded engine (replay / predict with band_rows=None) for the banded one.  Everything is compared bit for bit:
  * a row of final/conv is accumulated by the march over input rows yo-4 .. yo+4 whatever the segment it belongs to, and a zero row adds
    exact zeros, so a window's rows equal the whole image's;
  * an output pixel of a transposed convolution is a sum over (tap, channel) in a fixed order inside each kernel (convt3x3_c64_bf16_kernel:
    the static k-loop; gconv_bf16_kernel: taps, then k-steps; gconv_lds_bf16_kernel: 64-channel chunk, then (column offset, channel group),
    then row offset), padding contributes exact zeros, so a band's rows equal the whole image's -- as long as the band and the whole image
    run the SAME kernel.  launch_gconv (bf16_gconv.hip) picks the LDS-tiled kernel from 64 (tile, channel group) pairs per launch on and the
    streaming kernel below, and the two order the sum differently, so across that threshold a band is not bit-identical to the whole image
    (DESIGN.md section 9.5).  test_engine_banded_is_bit_identical therefore uses frames of 24 x 24 low-res pixels, where every launch of the
    whole image and of every band stays below the threshold (n * ceil(2w/32) * ceil(48/8) * 2 = 48 pairs at the second stage), and
    test_engine_banded_across_the_kernel_threshold frames of 24 x 40, where the whole image is above it and short bands are below, with
    the bound that reordering allows (_banded_tolerance)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def _randomize_bn(G, seed):
    """non-trivial BatchNormalization statistics / affine parameters / PReLU slopes, as after training (test_infer_x4_bf16_gpu.py)"""
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


# ---- 1. the window kernel against the existing entry point ----------------------------------------------------------------------------
_CASES = {}


def _final_case(rt, cin, n, h, w):
    """x, packed weights, bias on the device and, per tanh_act, the whole image by the existing entry point and its uint8 conversion:
    computed once per shape and shared, never modified"""
    from upscaler import _lib as L
    key = (cin, n, h, w)
    if key not in _CASES:
        g = torch.Generator().manual_seed(cin * 7 + n * 1000 + h * 10 + w)
        x = torch.randn(n, h, w, cin, generator=g).to(torch.bfloat16).to(rt.device)
        # 81 * cin products of unit-variance x: a weight scale of 1.2 / sqrt(81 cin) puts the pre-tanh values at a standard deviation of 1.2,
        # i.e. over about +-2 and more: tanh reaches both ends of the uint8 range
        wk = (torch.randn(9, 9, cin, 3, generator=g) * (1.2 / (81 * cin) ** 0.5)).to(rt.device)
        bias = (torch.randn(3, generator=g) * 0.2).to(rt.device)
        wf = torch.empty(rt.lib.vcg_conv9x9_to3_bf16_wfrag_bytes(cin), dtype=torch.uint8, device=rt.device)
        L.check(rt.lib.vcg_pack_conv9x9_to3_bf16(wk.data_ptr(), cin, wf.data_ptr(), rt.stream), "pack")
        d = L.ConvDesc(n, cin, h, w, 3, h, w, 9, 9, 1, 4, 4)
        ref = {}
        for act in (0, 1):
            y = torch.full((n, 3, h, w), float("nan"), device=rt.device)
            L.check(rt.lib.vcg_conv9x9_to3_bf16_fwd(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), bias.data_ptr(), act, y.data_ptr(), rt.stream), "fwd")
            u8 = torch.empty(n, h, w, 3, dtype=torch.uint8, device=rt.device)
            L.check(rt.lib.vcg_nchw_to_frames_u8(y.data_ptr(), u8.data_ptr(), n, h, w, 3, rt.stream), "to u8")
            ref[act] = (y, u8)
        torch.cuda.synchronize()
        _CASES[key] = (x, wf, bias, d, ref)
    return _CASES[key]


def _window(rt, case, act, kind, row0, rows, y_row0, y_h):
    """the window entry point into a sentinel-filled image of y_h rows; returns the image as raw bytes [n][planes or rows...]"""
    from upscaler import _lib as L
    x, wf, bias, d, _ = case
    n, w = d.n, d.w
    if kind == L.OUT_U8_NHWC:
        y = torch.full((n, y_h, w, 3), SENTINEL, dtype=torch.uint8, device=rt.device)
    else:
        y = torch.full((n, 3, y_h, w * 4), SENTINEL, dtype=torch.uint8, device=rt.device)          # fp32 NCHW as bytes
    L.check(rt.lib.vcg_conv9x9_to3_bf16_fwd_window(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), bias.data_ptr(), act, kind, y.data_ptr(),
                                                   row0, rows, y_row0, y_h, rt.stream), "window")
    torch.cuda.synchronize()
    return y


SHAPES = [(1, 1, 1), (2, 9, 70), (1, 37, 65), (3, 20, 130)]


@pytest.mark.parametrize("n,h,w", SHAPES)
@pytest.mark.parametrize("cin", [128, 256])
@pytest.mark.parametrize("act", [0, 1])
def test_window_kernel_against_the_existing_entry(rt, cin, n, h, w, act):
    from upscaler import _lib as L
    case = _final_case(rt, cin, n, h, w)
    ref32, ref8 = case[4][act]
    assert not torch.isnan(ref32).any()
    if h * w >= 600 and act == 1:
        assert int(ref8.min()) <= 2 and int(ref8.max()) >= 253                       # the uint8 outputs use the whole range
    if h * w >= 600 and act == 0:
        assert float(ref32.abs().max()) > 2.0
    ref32_bytes = ref32.contiguous().view(torch.uint8).view(n, 3, h, w * 4)
    # (a) the full window in fp32 is the existing entry point's output, bit for bit; (b) in uint8 it is vcg_nchw_to_frames_u8 of (a)
    assert torch.equal(_window(rt, case, act, L.OUT_F32_NCHW, 0, h, 0, h), ref32_bytes)
    assert torch.equal(_window(rt, case, act, L.OUT_U8_NHWC, 0, h, 0, h), ref8)
    # (c) sub-windows, placed at y_row0 in images of y_row0 + rows + 3 rows: the rows written equal the whole result's, every other byte
    # keeps its sentinel
    tried = 0
    for row0, rows in ((0, h), (4, h - 8), (0, 5), (h - 3, 3), (7, 1)):
        if rows <= 0 or row0 < 0 or row0 + rows > h:
            continue
        for y_row0 in (0, 2):
            y_h = y_row0 + rows + 3
            tried += 1
            got = _window(rt, case, act, L.OUT_F32_NCHW, row0, rows, y_row0, y_h)
            want = torch.full_like(got, SENTINEL)
            want[:, :, y_row0:y_row0 + rows] = ref32_bytes[:, :, row0:row0 + rows]
            assert torch.equal(got, want), ("f32", row0, rows, y_row0)
            got = _window(rt, case, act, L.OUT_U8_NHWC, row0, rows, y_row0, y_h)
            want = torch.full_like(got, SENTINEL)
            want[:, y_row0:y_row0 + rows] = ref8[:, row0:row0 + rows]
            assert torch.equal(got, want), ("u8", row0, rows, y_row0)
    assert tried >= 2


# ---- 2. the engine, uint8 in and out --------------------------------------------------------------------------------------------------
def _engine(k, f, norm="batch", h=24, w=40):
    from upscaler import model as PM
    G = PM.make_upscaler_orig((f * h, f * w, 3), kernel_size=k, upscale_factor=f, res_block_num=2, norm=norm, seed=7)
    _randomize_bn(G, 5)
    return G.to_inference_bf16()


def _check_u8(inf, u8, f, **kw):
    from upscaler import data as PD
    want = torch.cat([PD.device_to_frames_u8(inf.replay(PD.frames_u8_to_device(u8[i:i + 2]))) for i in range(0, u8.shape[0], 2)]).cpu().numpy()
    got = inf.upscale_frames(u8, batch_size=2, **kw)
    assert got.dtype == np.uint8 and got.shape == (u8.shape[0], f * u8.shape[1], f * u8.shape[2], 3)
    assert np.array_equal(got, want)
    assert np.array_equal(inf.upscale_frames(u8, batch_size=2, **kw), got)              # second call: pure replay
    assert int(got.max()) - int(got.min()) > 16                                       # (not a constant image)
    return got


@pytest.mark.parametrize("k,f", [(3, 2), (3, 4), (5, 2), (5, 4)])
def test_engine_uint8_frames(rt, k, f):
    """3 frames of 24 x 40 in batches of 2: a ragged last batch"""
    inf = _engine(k, f)
    u8 = np.random.RandomState(k * 10 + f).randint(0, 256, (3, 24, 40, 3)).astype(np.uint8)
    got = _check_u8(inf, u8, f)
    assert np.array_equal(inf.upscale_frames(torch.from_numpy(u8), batch_size=2), got)           # torch input
    assert np.array_equal(inf.upscale_frames([fr for fr in u8], batch_size=2), got)              # a list of HxWx3 images
    with pytest.raises(ValueError):
        inf.upscale_frames(u8.astype(np.float32))
    inf.refresh()
    assert not inf._graphs                                                                       # refresh() clears every graph


def test_engine_uint8_frames_instance_norm(rt):
    inf = _engine(5, 4, norm="instance")
    _check_u8(inf, np.random.RandomState(3).randint(0, 256, (3, 24, 40, 3)).astype(np.uint8), 4)


# ---- 3. the engine, banded ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,f", [(5, 4), (3, 2), (3, 4)])
def test_engine_banded_is_bit_identical(rt, k, f):
    h, w, n = 24, 24, 2
    inf = _engine(k, f, h=h, w=w)
    u8 = np.random.RandomState(k + f).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    x = (u8 / 127.5 - 1).astype(np.float32)
    want8, want32 = inf.upscale_frames(u8), inf.predict(x)
    assert len(inf._plan(n, h, w, None)[1]) == 1
    for band_rows in (5, 8, 1, 24):
        assert len(inf._plan(n, h, w, band_rows)[1]) == -(-h // band_rows)
        assert np.array_equal(inf.upscale_frames(u8, band_rows=band_rows), want8), band_rows
        assert np.array_equal(inf.predict(x, band_rows=band_rows), want32), band_rows
    # a lowered limit forces the automatic plan to band: half the frame's largest tensor -> at least 3 bands (each carries its halo)
    inf.TAIL_LIMIT = f * f * (h // 2) * w * 256 * 2
    bands = inf._plan(n, h, w, None)[1]
    assert len(bands) >= 3
    assert np.array_equal(inf.upscale_frames(u8), want8)
    assert np.array_equal(inf.predict(x), want32)


def _banded_tolerance(inf, n, h, w):
    """Elementwise bound on |banded - unbanded| of the engine's fp32 output (NHWC), from the unbanded pass's own stage tensors; None where
    the two must be bit-identical.

    What can differ.  A stage on the generic transposed convolution may run the streaming kernel on a band and the LDS-tiled kernel on the
    whole image.  Both sum the same products (bf16 x bf16, exact in fp32) in fp32 in different orders, so the two sums differ by fp32
    rounding only -- about sqrt(K) * 2^-24 of their terms' scale, K <= 25 * 256 -- and the stage stores them rounded to bf16.  So a
    stage-output element is either the same bf16 number or the adjacent one: it moves by at most one bf16 step, <= 2^-7 |u|.  The bound
    lets EVERY element of such a stage move by a whole step (in fact only those whose sum lies within the fp32 difference of a rounding
    boundary do, about one in a hundred).  A stage on convt3x3_c64_bf16_kernel (the first stage at kernel_size 3) runs one kernel with one
    order for every shape: identical inputs, identical outputs.
    How it travels.  The steps' signs are those of rounding errors: taken as independent and zero-mean, a sum sum_i w_i d_i with |d_i| <= c_i
    exceeds 6 * sqrt(sum_i w_i^2 c_i^2) with probability < 2 exp(-18) = 3e-8 (Hoeffding), against 1e5 output values.  So per element, in
    variances: V_s = (2^-7 u_s)^2 + convT(w_s^2, V_(s-1)) (LeakyReLU's slopes are <= 1; the second term is the first stage's steps
    arriving through the second, in front of its own rounding), V_y = conv9x9(w_f^2, V_last), and |dy| <= 6 sqrt(V_y) * (1 + 2^-6) + 4e-7:
    tanh has slope <= 1; final/conv is one kernel with one order, and its own fp32 rounding on two different inputs is, by the same
    argument, 2 * 6 sqrt(K_f) 2^-24 * 6 sqrt(conv9x9(w_f^2, u^2)) with K_f = 81 * 256, i.e. 6e-4 / (6 * 2^-7) = 1.3 % of the first term:
    the factor 1 + 2^-6; 4e-7 is twice fast_tanh's absolute error (bf16_conv9x9_to3.hip).  The weights are the bf16-rounded ones."""
    from oracle import keras_ops as K
    m = inf.model
    us = inf._buffers(n, h, w)["us"]                      # the stage outputs of the last unbanded fp32 pass (all n frames: one launch here)
    assert us[0].shape[0] == n
    sq = lambda t: t.to(torch.bfloat16).float().cpu() ** 2
    var = None
    for up, u in zip(m.ups, us):
        if not inf._generic(up, 0):
            assert var is None                            # (only the first stage, whose input is the trunk's output: the same everywhere)
            continue
        step = (u.float().cpu().permute(0, 3, 1, 2) * 2.0 ** -7) ** 2
        var = step if var is None else step + K.conv2d_transpose_same(var, sq(up.ps[up.name + "/kernel"]), None)
    if var is None:
        return None
    vy = K.conv2d(var, sq(m.c_fin.ps[m.c_fin.name + "/kernel"]), None)
    return (6.0 * (1 + 2.0 ** -6) * vy.sqrt() + 4e-7).permute(0, 2, 3, 1).contiguous().numpy()


@pytest.mark.parametrize("k,f", [(5, 4), (3, 2), (3, 4)])
def test_engine_banded_across_the_kernel_threshold(rt, k, f):
    """24 x 40 low-res pixels, 2 frames: the whole image's generic transposed convolutions run the LDS-tiled kernel (k5 x4: 72 (tile,
    channel group) pairs at the first stage), bands of 1, 5 or 8 rows the streaming kernel.  The fp32 output stays within the bound the
    reordering allows (_banded_tolerance), the uint8 output within 127.5 times that plus one level (two roundings to integers); k3 x2 has
    no generic stage and one band is the same launches, so those are bit-identical.
    Measured on an MI355X: k5 x4 fp32 max |diff| 3.91e-5 against a bound of 1.0e-2 (median over the image; max 1.09e-2), 19 of 92160 uint8
    values differ by one level; k3 x4 3.73e-5 against 6.4e-3 (max 6.7e-3), 7 values; the same for bands of 1, 5 and 8 rows and for the
    automatic plan under a lowered limit.  The bound is far from tight because it lets every stage-output element move."""
    h, w, n = 24, 40, 2
    inf = _engine(k, f, h=h, w=w)
    u8 = np.random.RandomState(k + f).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    x = (u8 / 127.5 - 1).astype(np.float32)
    want8, want32 = inf.upscale_frames(u8), inf.predict(x)
    tol = _banded_tolerance(inf, n, h, w)
    assert (tol is None) == (k == 3 and f == 2)
    if tol is not None:
        print("k%d x%d tolerance: max %.3e median %.3e" % (k, f, tol.max(), np.median(tol)))

    def check(band_rows, exact):
        got8, got32 = inf.upscale_frames(u8, band_rows=band_rows), inf.predict(x, band_rows=band_rows)
        d32 = np.abs(got32 - want32)
        d8 = np.abs(got8.astype(np.int32) - want8.astype(np.int32))
        print("k%d x%d band_rows %r: fp32 max diff %.3e, %d of %d values differ; uint8 max diff %d, %d differ"
              % (k, f, band_rows, d32.max(), int((d32 > 0).sum()), d32.size, d8.max(), int((d8 > 0).sum())))
        if exact:
            assert np.array_equal(got32, want32) and np.array_equal(got8, want8), band_rows
        else:
            assert (d32 <= tol).all(), (band_rows, float((d32 - tol).max()))
            assert (d8 <= 127.5 * tol + 1).all(), band_rows

    for band_rows in (5, 8, 1, 24):
        check(band_rows, tol is None or band_rows == 24)
    inf.TAIL_LIMIT = f * f * (h // 2) * w * 256 * 2          # the automatic plan has to band: at least 3 bands
    assert len(inf._plan(n, h, w, None)[1]) >= 3
    check(None, tol is None)


def test_upscale_frames_of_no_frames(rt):
    inf = _engine(3, 2)
    out = inf.upscale_frames(np.empty((0, 24, 40, 3), dtype=np.uint8))
    assert out.dtype == np.uint8 and out.shape == (0, 48, 80, 3)


# ---- 4. the attention generator -------------------------------------------------------------------------------------------------------
def test_attention_engine_uint8_frames(rt):
    from upscaler import data as PD
    from upscaler import model as PM
    G = PM.make_upscaler_attention((64, 96, 3), kernel_size=3, upscale_factor=4, res_block_num=2, seed=7)
    _randomize_bn(G, 5)
    inf = G.to_inference_bf16()
    u8 = np.random.RandomState(9).randint(0, 256, (2, 16, 24, 3)).astype(np.uint8)
    want = PD.device_to_frames_u8(inf.replay(PD.frames_u8_to_device(u8))).cpu().numpy()
    got = inf.upscale_frames(u8)
    assert got.dtype == np.uint8 and got.shape == (2, 64, 96, 3) and np.array_equal(got, want)
    assert np.array_equal(inf.upscale_frames(u8), got)
    with pytest.raises(NotImplementedError, match="row bands are served for make_upscaler_orig"):
        inf.upscale_frames(u8, band_rows=4)
    with pytest.raises(NotImplementedError, match="row bands are served for make_upscaler_orig"):
        inf.predict((u8 / 127.5 - 1).astype(np.float32), band_rows=4)

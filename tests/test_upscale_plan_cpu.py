"""The band plan of the bf16 inference engine's tail (upscaler/_infer.py: tail_halo, band_plan, tail_plan) and the argument checks of
vcg_conv9x9_to3_bf16_fwd_window, all on the CPU.

A band is a range of low-res rows of the trunk's output, extended by the halo that its window of output rows needs through the
transposed convolutions and final/conv's 9x9.  The halo is judged here against the fp64 oracle (oracle/keras_ops.py), not against the
derivation in tail_halo: rows outside a band's extent must not reach its window (sufficient), and the outermost row of the extent at an
interior edge must (minimal)."""
import ctypes

import pytest
import torch

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
LIMIT = 0xFFFFFFE0


@pytest.fixture(scope="module")
def infer():
    import __graft_entry__ as g
    g.build()
    from upscaler import _infer
    return _infer


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("stages", [1, 2])
def test_plan_shape(infer, k, stages):
    f = 2 ** stages
    for h in (1, 5, 7, 12, 24):
        for band_rows in (1, 2, 5, h, h + 3, None):
            bands = infer.band_plan(h, k, stages, band_rows)
            assert bands[0].ia == 0 and bands[-1].ib == h
            for a, b in zip(bands, bands[1:]):
                assert a.ib == b.ia and a.y_row0 + a.rows == b.y_row0           # [ia, ib) partition [0, h) in order, the windows [0, f h)
            assert bands[0].y_row0 == 0 and bands[-1].y_row0 + bands[-1].rows == f * h
            for b in bands:
                assert 0 <= b.start <= b.ia < b.ib <= b.end <= h                  # the extent lies inside the image and holds the band
                assert b.rows == f * (b.ib - b.ia) and b.y_row0 == f * b.ia and b.row0 == f * (b.ia - b.start)
                assert b.row0 + b.rows <= f * (b.end - b.start)                   # the window lies inside the band's up-sampled rows
                if band_rows is not None:
                    assert b.ib - b.ia <= band_rows
            if band_rows is None or band_rows >= h:
                assert len(bands) == 1 and bands[0].start == 0 and bands[0].end == h and bands[0].row0 == 0
            else:
                assert len(bands) == -(-h // band_rows)
    with pytest.raises(ValueError):
        infer.band_plan(8, k, stages, 0)


def _tail(x, wts, wf):
    """the tail in fp64: Conv2DTranspose(k, strides 2, 'same') + LeakyReLU(0.2) per stage, then the 9x9 'same' convolution"""
    from oracle import keras_ops as K
    for wt in wts:
        x = K.leaky_relu(K.conv2d_transpose_same(x, wt, None, 2), 0.2)
    return K.conv2d(x, wf, None, 1, "same")


@pytest.mark.parametrize("k,stages", [(5, 2), (3, 1), (3, 2), (5, 1)])
def test_halo_is_sufficient_and_minimal_against_the_oracle(infer, k, stages):
    """h = 12 in bands of 4 rows: a top-edge, an interior and a bottom-edge band (plus bands of 1 and 5 rows).  All weights and inputs are
    positive, so no dependence cancels."""
    g = torch.Generator().manual_seed(10 * k + stages)
    h, w, c, f = 12, 6, 2, 2 ** stages
    wts = [torch.rand(k, k, c, c, generator=g, dtype=torch.float64) + 0.1 for _ in range(stages)]
    wf = torch.rand(9, 9, c, c, generator=g, dtype=torch.float64) + 0.1
    x = torch.rand(1, c, h, w, generator=g, dtype=torch.float64) + 0.5
    full = _tail(x, wts, wf)
    e_top, e_bot = infer.tail_halo(k, stages)
    kinds = set()
    for band_rows in (4, 1, 5):
        for b in infer.band_plan(h, k, stages, band_rows):
            win = full[:, :, b.y_row0:b.y_row0 + b.rows]
            # sufficient (1): garbage in every row outside the extent does not reach the window
            xg = x.clone()
            xg[:, :, :b.start] = 1e6
            xg[:, :, b.end:] = 1e6
            got = _tail(xg, wts, wf)[:, :, b.y_row0:b.y_row0 + b.rows]
            assert torch.allclose(got, win, rtol=1e-12, atol=0), (band_rows, b)
            # sufficient (2): the tail on the band's rows ALONE (zero padding at its edges, as the engine runs it) has the window right
            alone = _tail(x[:, :, b.start:b.end].contiguous(), wts, wf)[:, :, b.row0:b.row0 + b.rows]
            assert torch.allclose(alone, win, rtol=1e-12, atol=0), (band_rows, b)
            # minimal: the outermost row of the extent at an interior edge does reach the window
            for edge, row in (("top", b.start), ("bottom", b.end - 1)):
                interior = b.start > 0 and b.ia - b.start == e_top if edge == "top" else b.end < h and b.end - b.ib == e_bot
                if not interior:
                    continue
                xg = x.clone()
                xg[:, :, row] = 1e6
                got = _tail(xg, wts, wf)[:, :, b.y_row0:b.y_row0 + b.rows]
                assert float((got - win).abs().max()) > 1.0, (band_rows, b, edge)
                kinds.add(edge)
            kinds.add("top-edge" if b.start == 0 else "bottom-edge" if b.end == h else "interior")
    assert kinds >= {"top", "bottom", "top-edge", "bottom-edge", "interior"}


def test_hand_derived_halo(infer):
    assert infer.tail_halo(5, 2) == (3, 2) and infer.tail_halo(3, 1) == (3, 2)


def test_automatic_plan(infer):
    """k5, two stages, 256 channels.  A launch's largest tensor is the last stage's output, f*rows x f*w x 256 bf16.
    (540, 960) -> 2160 x 3840 is 2160 * 3840 * 512 = 4 246 732 800 bytes: BELOW the limit 0xFFFFFFE0 = 4 294 967 264 (98.9 % of it), and
    with final/conv's 8 halo rows and 64 KiB 4 262 526 976, still below -- one frame per launch fits, so the automatic plan is the single
    band on which the engine ran before it had bands.  The frame that does exceed the limit is the next wider one, DCI 4K
    (540, 1024) -> 2160 x 4096 = 4 529 848 320 bytes: that one must be banded."""
    assert 2160 * 3840 * 512 == 4246732800 < LIMIT < 2160 * 4096 * 512
    for (h, w), need_bands in (((540, 960), False), ((540, 1024), True), ((1080, 2048), True)):
        for windowed in (False, True):
            ch, bands = infer.tail_plan(1, h, w, 5, 2, None, 256, LIMIT, False, windowed)
            assert ch == 1
            assert (len(bands) >= 2) == need_bands, (h, w, bands)
            big = max(infer.band_bytes(b, w, 2, 256) for b in bands)
            assert big <= LIMIT
            if len(bands) > 1:
                assert max(infer.band_bytes(b, w, 2, 256, 8) for b in bands) + 65536 <= LIMIT       # final/conv's descriptor
                rows = -(-h // len(bands))
                assert bands == infer.band_plan(h, 5, 2, rows)                                       # equal bands
                fewer = infer.band_plan(h, 5, 2, -(-h // (len(bands) - 1)))                          # ... and the fewest that fit
                assert max(infer.band_bytes(b, w, 2, 256, 8) for b in fewer) + 65536 > LIMIT
    # x2 (one stage) at 1080 x 1920 has the same byte count as x4 at 540 x 960
    assert len(infer.tail_plan(1, 1080, 1920, 5, 1, None, 256, LIMIT)[1]) == 1
    assert len(infer.tail_plan(1, 1080, 2048, 5, 1, None, 256, LIMIT)[1]) >= 2
    # 32 frames of 128 x 128: a single band, 16 + 16 frames per launch (31 fit: 2 launches, spread evenly), as before
    ch, bands = infer.tail_plan(32, 128, 128, 5, 2, None, 256, LIMIT)
    per = 16 * 128 * 128 * 512
    assert len(bands) == 1 and ch == 16 and LIMIT // per == 31
    assert infer.tail_chunk(32, 128, 128, 2) == 16 and infer.tail_chunk(9, 270, 480, 2, 128) == 5 and infer.tail_chunk(8, 270, 480, 2, 128) == 8
    # the k3 x2 topology keeps all frames in one launch, whatever the size
    assert infer.tail_plan(32, 256, 256, 3, 1, None, 256, LIMIT, legacy=True) == (32, infer.band_plan(256, 3, 1, None))
    # a lowered limit forces bands at a small shape; a forced band that does not fit is refused
    ch, bands = infer.tail_plan(2, 24, 40, 5, 2, None, 256, 16 * 12 * 40 * 512)
    assert len(bands) >= 3 and ch == 1
    with pytest.raises(ValueError):
        infer.tail_plan(2, 24, 40, 5, 2, 12, 256, 16 * 8 * 40 * 512)


def test_window_entry_point_refuses_before_any_device_work(infer):
    from upscaler import _lib as L
    cl = L.load()
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)          # non-null addresses: never dereferenced by the checks below
    fn = cl.vcg_conv9x9_to3_bf16_fwd_window
    d = L.ConvDesc(2, 256, 20, 30, 3, 20, 30, 9, 9, 1, 4, 4)

    def call(desc=d, x=one, wf=one, y=two, kind=L.OUT_U8_NHWC, row0=4, rows=8, y_row0=2, y_h=10):
        return fn(ctypes.byref(desc) if desc is not None else None, x, wf, one, 1, kind, y, row0, rows, y_row0, y_h, None)

    assert call(desc=None) == E_NULL and call(x=None) == E_NULL and call(wf=None) == E_NULL and call(y=None) == E_NULL
    for kw in (dict(rows=0), dict(rows=-3), dict(row0=-1), dict(row0=13, rows=8), dict(row0=0, rows=21), dict(y_row0=-1), dict(y_row0=3),
               dict(y_h=9), dict(rows=2 ** 31 - 1, row0=2 ** 31 - 1)):
        assert call(**kw) == E_SHAPE, kw
    assert call(desc=L.ConvDesc(2, 256, 20, 30, 3, 20, 31, 9, 9, 1, 4, 4)) == E_SHAPE
    assert call(desc=L.ConvDesc(0, 256, 20, 30, 3, 20, 30, 9, 9, 1, 4, 4)) == E_SHAPE
    for kind in (-1, 2, 7):
        assert call(kind=kind) == E_UNSUPPORTED
    for bad in (L.ConvDesc(2, 64, 20, 30, 3, 20, 30, 9, 9, 1, 4, 4), L.ConvDesc(2, 192, 20, 30, 3, 20, 30, 9, 9, 1, 4, 4),
                L.ConvDesc(2, 256, 20, 30, 4, 20, 30, 9, 9, 1, 4, 4), L.ConvDesc(2, 256, 20, 30, 3, 20, 30, 7, 7, 1, 3, 3),
                L.ConvDesc(2, 256, 20, 30, 3, 20, 30, 9, 9, 2, 4, 4), L.ConvDesc(2, 256, 20, 30, 3, 20, 30, 9, 9, 1, 3, 4)):
        assert call(desc=bad) == E_UNSUPPORTED
        assert cl.vcg_conv9x9_to3_bf16_fwd(ctypes.byref(bad), one, one, one, 1, two, None) == E_UNSUPPORTED       # as the existing entry
    # a band that does not fit the descriptor form: (h + 8) * w * cin * 2 + 64 KiB > 0xFFFFFFE0
    big = L.ConvDesc(1, 256, 2300, 3840, 3, 2300, 3840, 9, 9, 1, 4, 4)
    assert call(desc=big, row0=0, rows=16, y_row0=0, y_h=16) == E_UNSUPPORTED
    assert L.OUT_F32_NCHW == 0 and L.OUT_U8_NHWC == 1


def test_attention_engine_says_what_its_tail_serves(infer):
    """no model needed: the refusal of bands is _plan's, before any device work"""
    eng = object.__new__(infer.Bf16AttentionGenerator)
    eng.k, eng.ups, eng.legacy = 3, [None, None], False
    with pytest.raises(NotImplementedError, match="row bands are served for make_upscaler_orig"):
        eng._plan(2, 16, 24, band_rows=4)
    with pytest.raises(NotImplementedError, match="whole frames"):
        eng._plan(1, 1080, 1920, None)                   # 4320 x 7680 x 128 channels: 8.5 GB
    ch, bands = eng._plan(1, 540, 960, None, 1)          # a 2160 x 3840 frame, uint8 output: one band
    assert ch == 1 and len(bands) == 1

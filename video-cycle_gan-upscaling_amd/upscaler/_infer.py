"""Inference-only generator on the bf16-storage kernels (BASELINE.json config C5: "inference-only generator,
batch=32 256->512 bf16, hipGraph-captured per-frame step").

Serves ``make_upscaler_orig`` models (upscaling/upscaler/model.py:267-295) with 64 filters on RGB frames, kernel_size 3 or 5
and any power-of-two upscale_factor: BASELINE.json's configs (kernel_size 3, x2) and the reference's own defaults (kernel_size 5,
x4, 16 residual blocks; model.py:267, its CLI's -k 5 -u 4).  What the reference does per call is
``upscaler.predict(batch)`` (upscaling/upscaler/data.py:358-363, train_gan3.py:346): a forward pass with the
BatchNormalization layers in inference mode.  Here that pass is

    initial/conv 9x9 3->64 + PReLU            vcg_conv9x9_from3_bf16_fwd (fp32 NCHW frames in, bf16 NHWC out)
    res blocks: conv 3x3 + BN + PReLU         vcg_conv2d_bf16_fwd, BN folded into the epilogue's scale/shift
                conv 3x3 + BN + Add           same kernel, residual operand = block input
    prefinal conv 3x3 + BN + Add(long skip)   same kernel
    upsampling: ConvT 3x3 s2 64->256 + LReLU  vcg_conv_transpose2d_bf16_fwd
    final/conv 9x9 256->3 + tanh              vcg_conv9x9_to3_bf16_fwd (fp32 NCHW out), or vcg_conv9x9_to3_bf16_fwd_window
                                              (a window of rows; fp32 NCHW or uint8 NHWC frames out)

The 5x5 trunk convolutions run on the same entry point (the generic kernels' plan, weights as their MFMA fragments), and the
up-sampling stages that convt3x3_c64 does not serve -- 5x5, and 3x3 on 256 channels -- on vcg_conv_transpose2d_nhwc_bf16_fwd,
one per stage (64->256, then 256->256).  22 launches for the k3 x2
topology, recorded once per input shape into a hipGraph and replayed per batch.  Activations are bf16 NHWC,
accumulation and the epilogue arithmetic fp32; the weights are rounded to bf16 once, when the engine is built or
``refresh()`` is called after a weight update.  The folded BatchNormalization parameters
(scale = gamma / sqrt(moving_var + 1e-3), shift = (bias - moving_mean) * scale + beta) are 64-element fp32 vectors
derived by vcg_axpby + vcg_norm_finalize when the engine is built or refreshed.

Frames in and out.  ``predict`` / ``replay`` take and return fp32 (numpy NHWC / device NCHW in [-1, 1]) as the reference's
``upscaler.predict`` does.  ``upscale_frames`` is the reference's whole inference path, convert_image_series_to_array -> predict ->
convert_array_to_image (data.py:253-270, 358-363): uint8 frames in, uint8 frames out.  One byte per sample crosses the bus each way:
vcg_frames_u8_to_nchw fills the captured graph's input on the device, and final/conv stores the uint8 NHWC frame itself.

Row bands.  Every kernel of the tail (the up-sampling stages and final/conv) uses 32-bit offsets inside a launch, so a launch's largest
tensor must stay below 4 GiB.  Where one frame's does not (540x1024 -> 2160x4096: 4.53 GB; 2160x3840 still fits), the tail runs on row
bands of the trunk's output (``band_plan``): the transposed convolutions unchanged on a band extended by the halo its window needs, final/conv on the
window of the band's rows that are right."""
import collections
import ctypes
import os

import numpy as np
import torch

from . import _engine as E
from . import _lib as L


TAIL_LIMIT = 0xFFFFFFE0          # bytes of a tail launch's largest tensor: the kernels' offsets are 32-bit inside a launch

# A band of the tail: low-res rows [ia, ib) of the trunk's output, extended to [start, end) (clipped to the image) so that the window's
# rows and their 4-row halo are right; the final launch computes rows [row0, row0 + rows) of the band's up-sampled rows and stores them as
# rows [y_row0, y_row0 + rows) of the frame.
Band = collections.namedtuple("Band", "ia ib start end row0 rows y_row0")


def tail_halo(k, n_stages):
    """(e_top, e_bot): the low-res rows above / below its own that a band needs.  final/conv reads 4 rows above and below a window; output
    row o of a TF-SAME Conv2DTranspose(k, strides 2) with crop = max(k - 2, 0) // 2 reads input rows ceil((o + crop - k + 1) / 2) ...
    floor((o + crop) / 2).  Run back from a window [f * ia, f * ib) through the stages: every coordinate is (a multiple of the remaining
    factor) * ia + a constant, so the recursion on the constants alone (ia = ib = 0) gives the halo of every band."""
    crop = max(k - 2, 0) // 2
    lo, hi = -4, 3                       # first / last row read around the window [0, 0): rows -4 .. -1 above it, 0 .. 3 below
    for _ in range(n_stages):
        lo = -((-(lo + crop - k + 1)) // 2)
        hi = (hi + crop) // 2
    return -lo, hi + 1


def band_plan(h, k, n_stages, band_rows=None):
    """The bands of a frame of h low-res rows: band_rows rows each (the last one shorter); None: one band."""
    if band_rows is not None and int(band_rows) < 1:
        raise ValueError("band_rows must be a positive number of low-res rows, got %r" % (band_rows,))
    f = 2 ** n_stages
    e_top, e_bot = tail_halo(k, n_stages)
    step = h if band_rows is None else min(int(band_rows), h)
    bands = []
    for ia in range(0, h, step):
        ib = min(ia + step, h)
        start, end = max(0, ia - e_top), min(h, ib + e_bot)
        bands.append(Band(ia, ib, start, end, f * (ia - start), f * (ib - ia), f * ia))
    return bands


def band_bytes(band, w, n_stages, channels, halo_rows=0):
    """bytes of the largest tensor of one frame's band: the last stage's output, plus halo_rows rows (final/conv's descriptor covers 4 rows
    above and 4 below the band it reads)"""
    f = 2 ** n_stages
    return (f * (band.end - band.start) + halo_rows) * f * w * channels * 2


def _fits(band, w, n_stages, channels, limit, windowed):
    """does one frame's band fit the tail's launches: the transposed convolutions' tensors, and for the window launch of final/conv its
    descriptor (band + 8 rows + 64 KiB, vcg_conv9x9_to3_bf16_fwd_window)"""
    if windowed:
        return band_bytes(band, w, n_stages, channels, 8) + 65536 <= limit
    return band_bytes(band, w, n_stages, channels) <= limit


def tail_chunk(n, h, w, n_stages, channels=256, limit=TAIL_LIMIT, legacy=False):
    """frames per launch of an unbanded tail: as many as keep the last stage's output within the limit, spread evenly over the launches"""
    if legacy:
        return n
    f = 2 ** n_stages
    per = f * f * h * w * channels * 2
    ch = max(1, min(n, limit // per))
    launches = -(-n // ch)
    return -(-n // launches)                 # the same number of launches, frames spread evenly (32 -> 16 + 16, not 31 + 1)


def tail_plan(n, h, w, k, n_stages, band_rows=None, channels=256, limit=TAIL_LIMIT, legacy=False, windowed=False):
    """(frames per launch, bands) of the tail for n frames of h x w low-res pixels.
    band_rows None: one band wherever one frame's tail fits the limit, with the frames per launch tail_chunk gives (the k3 x2 topology: all
    of them, its launch sequence unchanged); otherwise the fewest equal bands whose largest tensor fits at one frame per launch.  An
    integer forces bands of that many low-res rows.
    windowed: a single band goes through final/conv's window launch too (uint8 output) and has to fit its descriptor."""
    if band_rows is not None:
        bands = band_plan(h, k, n_stages, band_rows)
    else:
        bands = band_plan(h, k, n_stages, None)
        if not _fits(bands[0], w, n_stages, channels, limit, windowed):
            for nb in range(2, h + 1):
                bands = band_plan(h, k, n_stages, -(-h // nb))
                if all(_fits(b, w, n_stages, channels, limit, True) for b in bands):
                    break
            else:
                raise ValueError("a band of one low-res row of width %d exceeds the tail's limit of %d bytes" % (w, limit))
    if len(bands) == 1:
        if windowed and not _fits(bands[0], w, n_stages, channels, limit, True):
            raise ValueError("band_rows=%r: the band exceeds the tail's limit of %d bytes" % (band_rows, limit))
        return tail_chunk(n, h, w, n_stages, channels, limit, legacy), bands
    if not all(_fits(b, w, n_stages, channels, limit, True) for b in bands):
        raise ValueError("band_rows=%r: a band's largest tensor exceeds the tail's limit of %d bytes" % (band_rows, limit))
    ch = max(1, min(n, limit // max(band_bytes(b, w, n_stages, channels) for b in bands)))
    launches = -(-n // ch)
    return -(-n // launches), bands


class Bf16Generator:
    TAIL_LIMIT = TAIL_LIMIT    # a test can lower it on an instance to force automatic banding at a small shape
    TAIL_CHANNELS = 256        # channels of the up-sampling stages' outputs (model.py:288): what the 4 GiB rule of _tail_chunk counts

    def __init__(self, model):
        from .model import UpscalerOrig
        if not isinstance(model, UpscalerOrig):
            raise TypeError("Bf16Generator serves make_upscaler_orig models")
        c1 = model.blocks[0][0] if model.blocks else model.c_pre
        if c1.cin != 64 or c1.cout != 64 or model.c_init.cin != 3:
            raise NotImplementedError("bf16 inference is instantiated for filters=64 on 3-channel (RGB) frames; "
                                      "use model.predict for other shapes")
        if c1.k not in (3, 5) or model.upscale_times < 1:
            raise NotImplementedError("bf16 inference is instantiated for kernel_size 3 or 5 and upscale_factor >= 2; "
                                      "use model.predict for other shapes")
        self.k = c1.k
        # the k3 x2 topology keeps its launch sequence exactly (BASELINE.json C5); the others chunk the tail by the 4 GiB rule
        self.legacy = self.k == 3 and model.upscale_times == 1
        self.instance = model.n_pre.norm == "instance"        # per-image statistics cannot be folded: bf16 norm kernels
        self.model = model
        self.rt = model.rt
        self._graphs = {}
        self._bufs = {}
        self.refresh()

    # ---- parameters ------------------------------------------------------------------------------------------
    def _pack(self, conv, transpose):
        """3x3 layers of the k3 topology: [tap][out][in] bf16 (Conv2D (k,k,in,out) with transpose=1, Conv2DTranspose (k,k,out,in) with
        transpose=0); every other layer: the generic kernels' MFMA fragments (vcg_pack_conv_frag_bf16: mode 0 for a Conv2D, mode 1 for a
        Conv2DTranspose, whose kernel is the data gradient's of a stride-2 Conv2D)"""
        w, taps = conv.ps[conv.name + "/kernel"], conv.k * conv.k
        if self._generic(conv, transpose):
            return E.pack_conv_frag_bf16(self.rt, w, taps, conv.cout, conv.cin, 1 - transpose)
        return E.pack_conv_kernel_bf16(self.rt, w, taps, conv.cout, conv.cin, transpose, 0)

    @staticmethod
    def _generic(conv, transpose):
        """True where the layer runs on the generic kernels: a 5x5 layer, or a transposed one on more than 64 input channels"""
        return conv.k != 3 or (not transpose and conv.cin != 64)

    def _fold(self, conv, norm):
        """scale = gamma / sqrt(moving_var + eps), shift = (bias - moving_mean) * scale + beta, by the same kernels the
        training path uses: vcg_axpby forms (moving_mean - bias), vcg_norm_finalize turns it into scale / shift"""
        rt, ps = self.rt, conv.ps
        c = conv.cout
        if self.instance:          # non-affine instance norm: only the convolution's bias is applied in its epilogue
            return E.filled_like(rt, ps[conv.name + "/bias"], 1.0), ps[conv.name + "/bias"]
        mean = ps[norm.name + "/moving_mean"].clone()
        E.axpby(rt, ps[conv.name + "/bias"], mean, -1.0, 1.0)
        scale, shift = rt.empty(c), rt.empty(c)
        L.check(rt.lib.vcg_norm_finalize(mean.data_ptr(), ps[norm.name + "/moving_variance"].data_ptr(), ps[norm.name + "/gamma"].data_ptr(),
                                         ps[norm.name + "/beta"].data_ptr(), c, 1, E.BN_EPS, scale.data_ptr(), shift.data_ptr(), None, None, None,
                                         0.0, 0, rt.stream), "vcg_norm_finalize")
        return scale, shift

    def refresh(self):
        """(re)derive the packed bf16 weights and the folded BatchNormalization vectors from the model's parameters"""
        m, rt = self.model, self.rt
        self.trunk = []
        for (c1, n1, c2, n2) in m.blocks:
            s1, h1 = self._fold(c1, n1)
            s2, h2 = self._fold(c2, n2)
            self.trunk.append((self._pack(c1, 1), s1, h1, c1.ps[n1.prelu_name + "/alpha"], self._pack(c2, 1), s2, h2))
        sp, hp = self._fold(m.c_pre, m.n_pre)
        self.prefinal = (self._pack(m.c_pre, 1), sp, hp)
        # one weight set per up-sampling stage: 64 -> 256, then 256 -> 256 (model.py:286-288)
        self.up_layers = m.ups
        self.ups = [(self._pack(up, 0), up.ps[up.name + "/bias"], float(up.alpha), up.cin) for up in m.ups]
        self.up = self.ups[0][:3]
        self.final = (E.pack_final9x9_bf16(rt, m.c_fin.ps[m.c_fin.name + "/kernel"]), m.c_fin.ps[m.c_fin.name + "/bias"])
        self.first = (E.pack_first9x9_bf16(rt, m.c_init.ps[m.c_init.name + "/kernel"]), m.c_init.ps[m.c_init.name + "/bias"],
                      m.c_init.ps[m.a_init.prelu_name + "/alpha"])
        self._graphs.clear()          # recorded graphs hold the old parameter buffers
        self._staging = None          # upscale_frames' pinned and device staging buffers

    # ---- one forward pass (22 launches) -----------------------------------------------------------------------
    def _trunk_buffers(self, n, h, w):
        key = ("trunk", n, h, w)
        if key not in self._bufs:
            dev = self.rt.device
            bf = lambda c, hh, ww: torch.empty(n, hh, ww, c, dtype=torch.bfloat16, device=dev)
            self._bufs[key] = {"skip": bf(64, h, w),
                               "a": bf(64, h, w), "b": bf(64, h, w), "c": bf(64, h, w),
                               "z": bf(64, h, w) if self.instance else None,
                               "stats": torch.empty(5, n * 64, dtype=torch.float32, device=dev) if self.instance else None}
        return self._bufs[key]

    def _buffers(self, n, h, w):
        """the trunk's buffers and those of the unbanded fp32 tail"""
        key = (n, h, w)
        if key not in self._bufs:
            dev = self.rt.device
            ch = self._tail_chunk(n, h, w)
            f = 2 ** len(self.ups)
            # one bf16 NHWC buffer per up-sampling stage: [ch, 2h, 2w, 256], [ch, 4h, 4w, 256], ...
            us = [torch.empty(ch, 2 ** (s + 1) * h, 2 ** (s + 1) * w, 256, dtype=torch.bfloat16, device=dev) for s in range(len(self.ups))]
            self._bufs[key] = dict(self._trunk_buffers(n, h, w), u=us[0], us=us,
                                   y=torch.empty(n, 3, f * h, f * w, dtype=torch.float32, device=dev))
        return self._bufs[key]

    def _band_buffers(self, n, h, w, ch, bands, out_kind):
        """the banded (or uint8) tail: flat buffers sized for the largest band of ch frames -- the band's rows of the trunk output and one
        per up-sampling stage, viewed per band as compact [c, rows, w, C] tensors -- and the frames it writes"""
        key = (n, h, w, ch, tuple(bands), out_kind)
        if key not in self._bufs:
            dev = self.rt.device
            f = 2 ** len(self.ups)
            rows = max(b.end - b.start for b in bands)
            part = max([b.end - b.start for b in bands if b.end - b.start < h] or [0])      # (a band of all rows reads the trunk output in place)
            flat = lambda count: torch.empty(count, dtype=torch.bfloat16, device=dev)
            y = (torch.empty(n, f * h, f * w, 3, dtype=torch.uint8, device=dev) if out_kind == L.OUT_U8_NHWC
                 else torch.empty(n, 3, f * h, f * w, dtype=torch.float32, device=dev))
            self._bufs[key] = {"in": flat(ch * part * w * 64) if part else None,
                               "us": [flat(ch * 4 ** (s + 1) * rows * w * 256) for s in range(len(self.ups))], "y": y}
        return self._bufs[key]

    def _factor(self):
        """output frame size / input frame size: one doubling per up-sampling stage here and in the attention generator; an engine whose
        up-sampling stages also undo down-sampling ones (Bf16CycleGanGenerator) overrides it"""
        return 2 ** len(self.ups)

    def _tail_chunk(self, n, h, w):
        """frames per launch of the up-sampling stages and final/conv of an unbanded tail.  Beyond the k3 x2 topology, a launch's largest
        tensor (the last stage's output, 2 * 256 bytes per pixel) stays below 4 GiB: the kernels' offsets are 32-bit inside an image, and
        final/conv's descriptor covers the whole launch"""
        return tail_chunk(n, h, w, len(self.ups), self.TAIL_CHANNELS, self.TAIL_LIMIT, self.legacy)

    def _plan(self, n, h, w, band_rows=None, out_kind=L.OUT_F32_NCHW):
        """(frames per launch, bands) of the tail; one band and fp32 output is the path without bands, with _tail_chunk's frames per launch"""
        ch, bands = tail_plan(n, h, w, self.k, len(self.ups), band_rows, self.TAIL_CHANNELS, self.TAIL_LIMIT, self.legacy,
                              windowed=out_kind != L.OUT_F32_NCHW)
        return ch, tuple(bands)

    def _conv(self, x, w, y, scale, shift, act, alpha, res, n, h, wd):
        rt = self.rt
        if self.instance:
            return self._conv_instance_norm(x, w, y, shift, act, alpha, res, n, h, wd)
        k = self.k
        d = L.ConvDesc(n, 64, h, wd, 64, h, wd, k, k, 1, k // 2, k // 2)
        ep = L.EpilogueBf16(scale.data_ptr(), shift.data_ptr(), act, 0.0, alpha.data_ptr() if alpha is not None else None,
                            res.data_ptr() if res is not None else None)
        L.check(rt.lib.vcg_conv2d_bf16_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), y.data_ptr(), ctypes.byref(ep), rt.stream),
                "vcg_conv2d_bf16_fwd")

    def _conv_instance_norm(self, x, w, y, bias, act, alpha, res, n, h, wd):
        """conv (+bias) -> per-image statistics -> normalise + activation + Add, all on bf16 NHWC"""
        rt = self.rt
        B = self._trunk_buffers(n, h, wd)
        k = self.k
        d = L.ConvDesc(n, 64, h, wd, 64, h, wd, k, k, 1, k // 2, k // 2)
        ep = L.EpilogueBf16(None, bias.data_ptr(), L.ACT_NONE, 0.0, None, None)
        L.check(rt.lib.vcg_conv2d_bf16_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), B["z"].data_ptr(), ctypes.byref(ep), rt.stream),
                "vcg_conv2d_bf16_fwd")
        self._norm_act(B["z"], y, B["stats"], alpha, res)

    def _norm_act(self, z, y, stats, alpha, res, nrec=-1, part=None, scale=None, shift=None):
        """the norm (+ PReLU with the slopes alpha, + Add of res) behind a convolution, z -> y on bf16 NHWC.  stats: instance norm's
        [5, >= n * c] scratch -- the per-image scale / shift come from the convolution's epilogue records part (nrec > 0 per image:
        vcg_norm_finalize_partials) or from a statistics pass over z; None: the per-channel scale / shift given"""
        rt = self.rt
        n, h, w, c = z.shape
        if stats is not None:
            mean, var, scale, shift, invstd = (stats[i] for i in range(5))
            if nrec > 0:
                L.check(rt.lib.vcg_norm_finalize_partials(part.data_ptr(), nrec, n, c, float(h * w), None, None, E.IN_EPS, mean.data_ptr(),
                                                          scale.data_ptr(), shift.data_ptr(), invstd.data_ptr(), None, None, 0.0, 0, rt.stream),
                        "vcg_norm_finalize_partials")
            else:
                ws, wsn = rt.workspace(rt.lib.vcg_norm_stats_bf16_workspace_bytes(n, c, h * w, L.NORM_INSTANCE))
                L.check(rt.lib.vcg_norm_stats_bf16(z.data_ptr(), n, c, h * w, L.NORM_INSTANCE, mean.data_ptr(), var.data_ptr(), ws, wsn,
                                                   rt.stream), "vcg_norm_stats_bf16")
                L.check(rt.lib.vcg_norm_finalize(mean.data_ptr(), var.data_ptr(), None, None, c, n, E.IN_EPS, scale.data_ptr(), shift.data_ptr(),
                                                 invstd.data_ptr(), None, None, 0.0, 0, rt.stream), "vcg_norm_finalize")
        L.check(rt.lib.vcg_norm_act_fwd_bf16(z.data_ptr(), n, c, h * w, scale.data_ptr(), shift.data_ptr(), 1 if stats is not None else 0,
                                             L.ACT_PRELU if alpha is not None else L.ACT_NONE, 0.0,
                                             alpha.data_ptr() if alpha is not None else None,
                                             res.data_ptr() if res is not None else None, y.data_ptr(), rt.stream),
                "vcg_norm_act_fwd_bf16")

    def _stem(self, x, w, bias, alpha, y):
        """the 9x9 3 -> 64 convolution of the fp32 NCHW frames x + bias (+ PReLU with the slopes alpha, or None) -> y bf16 NHWC"""
        rt = self.rt
        n, _, h, wd = x.shape
        d = L.ConvDesc(n, 3, h, wd, 64, h, wd, 9, 9, 1, 4, 4)
        L.check(rt.lib.vcg_conv9x9_from3_bf16_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), bias.data_ptr(),
                                                  alpha.data_ptr() if alpha is not None else None, y.data_ptr(), rt.stream),
                "vcg_conv9x9_from3_bf16_fwd")

    def _trunk(self, x, B, gate=None):
        """initial/conv, the residual blocks and the convolution behind them (+ long skip) on the buffers B; returns the buffer that holds
        the result.  gate(block's gate weights, block input, B["g"]): the attention engine's gate in front of a block's first convolution"""
        n, _, h, w = x.shape
        self._stem(x, *self.first, B["skip"])
        cur = B["skip"]                     # block input; outputs ping-pong between "a" and "c", "skip" is never overwritten
        for blk in self.trunk:
            w1, s1, h1, al, w2, s2, h2 = blk[-7:]
            out = B["a"] if cur is not B["a"] else B["c"]
            src = cur
            if gate is not None:
                gate(blk[0], cur, B["g"])
                src = B["g"]
            self._conv(src, w1, B["b"], s1, h1, L.ACT_PRELU, al, None, n, h, w)
            self._conv(B["b"], w2, out, s2, h2, L.ACT_NONE, None, cur, n, h, w)          # Add of the (ungated) block input
            cur = out
        wp, sp, hp = self.prefinal
        out = B["a"] if cur is not B["a"] else B["c"]
        self._conv(cur, wp, out, sp, hp, L.ACT_NONE, None, B["skip"], n, h, w)
        return out

    def _to3(self, src, y, out_kind=L.OUT_F32_NCHW, window=None):
        """the last convolution, Conv2D(3, 9, 'same') + tanh with self.final's packed kernel and bias, of the bf16 NHWC tensor src into
        the frames y (its first y.shape[0] images): the 64-channel entry point or the one that takes the channel count; the plain form
        for fp32 output of whole frames, the window form for uint8 output (the whole frame as one window) or for a given window =
        (row0, rows, y_row0, frame_rows)"""
        rt = self.rt
        wf, bias = self.final[:2]
        _, hh, ww, cin = src.shape
        d = L.ConvDesc(y.shape[0], cin, hh, ww, 3, hh, ww, 9, 9, 1, 4, 4)
        name = "vcg_conv9x9_c64to3_bf16_fwd" if cin == 64 else "vcg_conv9x9_to3_bf16_fwd"
        if window is None and out_kind == L.OUT_F32_NCHW:
            L.check(getattr(rt.lib, name)(ctypes.byref(d), src.data_ptr(), wf.data_ptr(), bias.data_ptr(), 1, y.data_ptr(), rt.stream), name)
        else:
            row0, rows, y_row0, frame_rows = window or (0, hh, 0, hh)
            L.check(getattr(rt.lib, name + "_window")(ctypes.byref(d), src.data_ptr(), wf.data_ptr(), bias.data_ptr(), 1, out_kind, y.data_ptr(),
                                                      row0, rows, y_row0, frame_rows, rt.stream), name + "_window")

    def forward(self, x, out_kind=L.OUT_F32_NCHW, band_rows=None):
        """x: device fp32 NCHW [n,3,h,w] in [-1,1] -> device fp32 NCHW [n,3,f*h,f*w], or with out_kind OUT_U8_NHWC device uint8 frames
        [n,f*h,f*w,3] (f = upscale_factor; buffer owned by the engine).  band_rows: see tail_plan"""
        n, _, h, w = x.shape
        ch, bands = self._plan(n, h, w, band_rows, out_kind)
        banded = len(bands) > 1 or out_kind != L.OUT_F32_NCHW
        B = self._trunk_buffers(n, h, w) if banded else self._buffers(n, h, w)
        out = self._trunk(x, B)
        if banded:
            return self._tail_bands(out, n, h, w, ch, bands, out_kind)
        us, y = B["us"], B["y"]
        ch = us[0].shape[0]
        for i in range(0, n, ch):
            c = min(ch, n - i)
            src, hh, ww = self._upsample(out[i:i + c], us, c, h, w)
            self._to3(src, y[i:i + c])
        return B["y"]

    def _upsample(self, src, us, c, hh, ww):
        """the up-sampling stages on c frames of hh x ww pixels (a whole image or a band: a band is a shorter image) into the buffers us;
        returns the last stage's output and its size"""
        rt, k, crop = self.rt, self.k, max(self.k - 2, 0) // 2           # TF-SAME crop of Conv2DTranspose(k, strides 2): k3 (0, 1), k5 (1, 2)
        for (wt, bt, slope, cin), up, u in zip(self.ups, self.up_layers, us):
            dt = L.ConvDesc(c, cin, hh, ww, 256, 2 * hh, 2 * ww, k, k, 2, crop, crop)
            if self._generic(up, 0):
                L.check(rt.lib.vcg_conv_transpose2d_nhwc_bf16_fwd(ctypes.byref(dt), src.data_ptr(), wt.data_ptr(), bt.data_ptr(), L.ACT_LRELU,
                                                                  slope, u.data_ptr(), rt.stream), "vcg_conv_transpose2d_nhwc_bf16_fwd")
            else:
                ept = L.EpilogueBf16(None, bt.data_ptr(), L.ACT_LRELU, slope, None, None)
                L.check(rt.lib.vcg_conv_transpose2d_bf16_fwd(ctypes.byref(dt), src.data_ptr(), wt.data_ptr(), u.data_ptr(), ctypes.byref(ept),
                                                             rt.stream), "vcg_conv_transpose2d_bf16_fwd")
            src, hh, ww = u, 2 * hh, 2 * ww
        return src, hh, ww

    def _tail_bands(self, out, n, h, w, ch, bands, out_kind):
        """the tail band by band: the band's rows of the trunk output in a compact buffer (a strided copy: 64 channels at low resolution),
        the up-sampling stages unchanged on the band, final/conv on the band's window into its rows of the frames"""
        T = self._band_buffers(n, h, w, ch, bands, out_kind)
        f, y = 2 ** len(self.ups), T["y"]
        for i in range(0, n, ch):
            c = min(ch, n - i)
            for b in bands:
                rows = b.end - b.start
                if rows == h:
                    src = out[i:i + c]
                else:
                    src = T["in"][:c * rows * w * 64].view(c, rows, w, 64)
                    src.copy_(out[i:i + c, b.start:b.end])
                us = [u[:c * 4 ** (s + 1) * rows * w * 256].view(c, 2 ** (s + 1) * rows, 2 ** (s + 1) * w, 256) for s, u in enumerate(T["us"])]
                src, hh, ww = self._upsample(src, us, c, rows, w)
                self._to3(src, y[i:i + c], out_kind, (b.row0, b.rows, b.y_row0, f * h))
        return y

    # ---- hipGraph ---------------------------------------------------------------------------------------------
    def capture(self, n, h, w, out_kind=L.OUT_F32_NCHW, band_rows=None):
        """record the pass for one input shape, output kind and band plan; ``replay(x)`` then costs one graph launch"""
        key = (n, h, w, out_kind) + self._plan(n, h, w, band_rows, out_kind)
        if key in self._graphs:
            return self._graphs[key]
        xin = torch.zeros(n, 3, h, w, dtype=torch.float32, device=self.rt.device)
        self.forward(xin, out_kind, band_rows)                  # warm-up: buffers exist, kernel attributes are set
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            y = self.forward(xin, out_kind, band_rows)
        self._graphs[key] = (g, xin, y)
        return self._graphs[key]

    def replay(self, x, band_rows=None):
        g, xin, y = self.capture(x.shape[0], x.shape[2], x.shape[3], L.OUT_F32_NCHW, band_rows)
        xin.copy_(x)
        g.replay()
        return y

    # ---- Keras-style entry point -------------------------------------------------------------------------------
    def predict(self, x, batch_size=32, band_rows=None):
        """x: numpy NHWC in [-1,1] (data.py:266-270) -> numpy NHWC float32, through the captured graph.  band_rows: low-res rows per
        band of the tail (tail_plan); None bands a frame only where its tail exceeds the 4 GiB of a launch"""
        rt = self.rt
        x = np.asarray(x)
        outs = []
        for i in range(0, x.shape[0], batch_size):
            xb = E.to_device_nchw(rt, x[i:i + batch_size])
            y = self.replay(xb, band_rows)
            outs.append(E.to_nhwc(rt, y).cpu().numpy())
        return np.concatenate(outs, 0)

    # ---- uint8 frames in, uint8 frames out ----------------------------------------------------------------------
    def upscale_frames(self, frames, batch_size=32, band_rows=None):
        """frames: uint8 [N,h,w,3] (numpy, torch, or a list of HxWx3 images) -> uint8 numpy [N,f*h,f*w,3]: the reference's
        convert_image_series_to_array -> predict -> convert_array_to_image (data.py:253-270, 358-363).  Per batch the uint8 frames go to
        the device (1 byte per sample), vcg_frames_u8_to_nchw writes the captured graph's input, the graph is replayed -- final/conv stores
        the uint8 NHWC frames -- and the uint8 result comes back.  A ragged last batch records its own graph, as in predict.
        Batch i+1's upload and batch i-1's download run under batch i's replay: two pinned host staging buffers and two device buffers
        per direction, one copy stream per direction, events only (1.16x the rate of copying synchronously on the compute stream at
        256 -> 512; scripts/bench_infer_bf16.py --u8, profiles/upscale_frames.txt).  The graph's input and output are touched by the
        compute stream alone (the conversion kernel writes the input, a device copy takes the output), in stream order.  The staging
        buffers of the last (batch, h, w) are kept until refresh()."""
        rt = self.rt
        if isinstance(frames, torch.Tensor):
            t = frames
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(frames)))
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
            raise ValueError("expected uint8 frames [N,h,w,3], got %s %s" % (t.dtype, tuple(t.shape)))
        n, h, w, _ = t.shape
        f = self._factor()
        out = np.empty((n, f * h, f * w, 3), dtype=np.uint8)
        if n == 0:
            return out
        bs = min(batch_size, n)
        key = (bs, h, w)
        if self._staging is None or self._staging["key"] != key:
            dev = rt.device
            self._staging = {"key": key,
                             "hin": [torch.empty(bs, h, w, 3, dtype=torch.uint8, pin_memory=True) for _ in range(2)],
                             "hout": [torch.empty(bs, f * h, f * w, 3, dtype=torch.uint8, pin_memory=True) for _ in range(2)],
                             "din": [torch.empty(bs, h, w, 3, dtype=torch.uint8, device=dev) for _ in range(2)],
                             "dout": [torch.empty(bs, f * h, f * w, 3, dtype=torch.uint8, device=dev) for _ in range(2)],
                             "up": torch.cuda.Stream(), "dn": torch.cuda.Stream()}
        S = self._staging
        starts = list(range(0, n, bs))
        for nb in {min(bs, n - i) for i in starts}:
            self.capture(nb, h, w, L.OUT_U8_NHWC, band_rows)             # graphs are recorded before the pipeline starts
        main = torch.cuda.current_stream()
        ev = lambda: [torch.cuda.Event(), torch.cuda.Event()]
        up_done, in_used, y_taken, dn_done = ev(), ev(), ev(), ev()
        for j in range(len(starts) + 1):
            if j < len(starts):
                i, s = starts[j], j % 2
                nb = min(bs, n - i)
                if j >= 2:
                    up_done[s].synchronize()                             # the staging buffer's previous upload has left it
                S["hin"][s][:nb].copy_(t[i:i + nb])
                with torch.cuda.stream(S["up"]):
                    if j >= 2:
                        S["up"].wait_event(in_used[s])                   # the conversion of batch j-2 has read din[s]
                    S["din"][s][:nb].copy_(S["hin"][s][:nb], non_blocking=True)
                    up_done[s].record(S["up"])
                g, xin, y = self.capture(nb, h, w, L.OUT_U8_NHWC, band_rows)
                main.wait_event(up_done[s])
                L.check(rt.lib.vcg_frames_u8_to_nchw(S["din"][s].data_ptr(), xin.data_ptr(), nb, h, w, 3, rt.stream), "vcg_frames_u8_to_nchw")
                in_used[s].record(main)
                g.replay()
                if j >= 2:
                    main.wait_event(dn_done[s])                          # the download of batch j-2 has read dout[s]
                S["dout"][s][:nb].copy_(y)
                y_taken[s].record(main)
                with torch.cuda.stream(S["dn"]):
                    S["dn"].wait_event(y_taken[s])
                    S["hout"][s][:nb].copy_(S["dout"][s][:nb], non_blocking=True)
                    dn_done[s].record(S["dn"])
            if j >= 1:
                i, s = starts[j - 1], (j - 1) % 2
                nb = min(bs, n - i)
                dn_done[s].synchronize()
                out[i:i + nb] = S["hout"][s][:nb].numpy()
        return out


class Bf16AttentionGenerator(Bf16Generator):
    """The same engine for ``make_upscaler_attention`` models (upscaling/upscaler/model.py:299-328; train_gan3.py's default
    ``-gm resnet-att``), filters 64 on RGB frames, BatchNormalization, kernel_size 3 or 5, upscale_factor 2 or 4, any res_block_num:

        initial/conv 9x9 3->64 + PReLU                          vcg_conv9x9_from3_bf16_fwd
        res blocks: sigmoid(conv(frames)) * m                   vcg_conv_in_gate_bf16_fwd (cin 3; the attention tensor is never stored)
                    conv + BN + PReLU, conv + BN + Add(m)       vcg_conv2d_bf16_fwd, the Add takes the UNGATED block input (model.py:48)
        after_res conv + BN + Add(long skip)                    vcg_conv2d_bf16_fwd
        up-sampling block i (scale s = 2**(i+1)):
            u = [nearest, bilinear](frames, s/2)                vcg_resize2d / vcg_copy_channels, fp32 NCHW, 6 channels (data only)
            sigmoid(conv(u)) * m                                vcg_conv_in_gate_bf16_fwd (cin 6)
            ConvT k s2 -> 128 + LeakyReLU(0.2)                  vcg_conv_transpose2d_nhwc_bf16_fwd
            + ConvT(s+1, strides s)(atanh(0.99999 frames))      vcg_input_convt_add_bf16, in place
        final/conv 9x9 128->3 + tanh                            vcg_conv9x9_to3_bf16_fwd (cin 128), or its window form for uint8 frames

    3 launches per residual block; _fold, _pack, capture / replay / predict / upscale_frames and the 4 GiB chunking of the tail are
    Bf16Generator's.  The tail is not banded: it reads fp32 NCHW frame data (the gates' inputs, to_add_input) whose row bands are not
    contiguous, and its largest tensor has 128 channels, so a whole 4K frame fits a launch."""
    TAIL_CHANNELS = 128
    SERVED = "bf16 inference of make_upscaler_attention is instantiated for filters=64 on 3-channel (RGB) frames, norm='batch', " \
             "kernel_size 3 or 5 and upscale_factor 2 or 4 (any res_block_num); use model.predict for other shapes"
    SERVED_TAIL = "bf16 inference of make_upscaler_attention runs the tail on whole frames (band_rows=None) whose largest tensor, " \
                  "f*h x f*w x 128 channels in bf16, fits a launch of 4 GiB (a 2160x3840 frame does); row bands are served for " \
                  "make_upscaler_orig models only"

    def __init__(self, model):
        cfg = getattr(model, "attention_generator", None)
        if cfg is None or not hasattr(model, "graph"):
            raise TypeError("Bf16AttentionGenerator serves make_upscaler_attention models")
        if cfg["filters"] != 64 or cfg["channels"] != 3 or cfg["norm"] != "batch" or cfg["kernel_size"] not in (3, 5) \
                or cfg["upscale_factor"] not in (2, 4):
            raise NotImplementedError(self.SERVED)
        self.k = cfg["kernel_size"]
        self.res_block_num, self.upscale_times = cfg["res_block_num"], {2: 1, 4: 2}[cfg["upscale_factor"]]
        self.legacy = False
        self.instance = False
        self.model = model
        self.rt = model.rt
        self.layers = {l.name: l for l in model.layers}
        self._graphs = {}
        self._bufs = {}
        self.refresh()

    @staticmethod
    def _generic(conv, transpose):
        """every transposed convolution (64 -> 128, 128 -> 128) and the 5x5 trunk run on the generic kernels"""
        return not transpose or conv.k != 3

    def _pack_gate(self, conv):
        out = E.pack_conv_in_gate_bf16(self.rt, conv.ps[conv.name + "/kernel"], conv.cin, conv.k, conv.k, conv.cout)
        if out is None:
            raise NotImplementedError(self.SERVED)
        return out, conv.ps[conv.name + "/bias"]

    def refresh(self):
        """(re)derive the packed bf16 weights and the folded BatchNormalization vectors from the model's parameters"""
        rt, ly = self.rt, self.layers
        ps = self.model.ps
        self.trunk = []
        for i in range(self.res_block_num):
            n = "res_block/%d" % i
            c1, n1, c2, n2 = ly[n + "/conv_pre"], ly[n + "/batch_norm_pre"], ly[n + "/conv_post"], ly[n + "/batch_norm_post"]
            s1, h1 = self._fold(c1, n1)
            s2, h2 = self._fold(c2, n2)
            self.trunk.append((self._pack_gate(ly[n + "/attention"]), self._pack(c1, 1), s1, h1, ps[n1.prelu_name + "/alpha"],
                               self._pack(c2, 1), s2, h2))
        ca = ly["after_res/conv"]
        sp, hp = self._fold(ca, ly["after_res/batch_norm"])
        self.prefinal = (self._pack(ca, 1), sp, hp)
        self.ups = []
        for i in range(self.upscale_times):
            n = "upscaling/%d/block" % i
            up, ta = ly[n + "/conv_transp"], ly[n + "/to_add_input_conv_transp"]
            self.ups.append((self._pack_gate(ly[n + "/attention"]), self._pack(up, 0), ps[up.name + "/bias"], float(up.alpha), up.cin, up.cout,
                             ps[ta.name + "/kernel"], ps[ta.name + "/bias"]))
        cf = ly["final/conv"]
        self.final = (E.pack_conv9x9_to3_bf16(rt, ps[cf.name + "/kernel"], cf.cin), ps[cf.name + "/bias"], cf.cin)
        c0 = ly["initial/conv"]
        self.first = (E.pack_first9x9_bf16(rt, ps[c0.name + "/kernel"]), ps[c0.name + "/bias"], ps["initial/prelu/alpha"])
        self._graphs.clear()          # recorded graphs hold the old parameter buffers
        self._staging = None          # upscale_frames' pinned and device staging buffers

    def _buffers(self, n, h, w):
        key = (n, h, w)
        if key not in self._bufs:
            dev = self.rt.device
            bf = lambda nn, c, hh, ww: torch.empty(nn, hh, ww, c, dtype=torch.bfloat16, device=dev)
            ch = self._tail_chunk(n, h, w)
            f = 2 ** len(self.ups)
            stages = []
            for s, up in enumerate(self.ups):
                r, cin, cout = 2 ** s, up[4], up[5]
                stages.append({"u": torch.empty(n, 6, r * h, r * w, dtype=torch.float32, device=dev),      # [nearest, bilinear] of the frames
                               "t": torch.empty(n, 3, r * h, r * w, dtype=torch.float32, device=dev) if r > 1 else None,
                               "g": bf(ch, cin, r * h, r * w), "y": bf(ch, cout, 2 * r * h, 2 * r * w)})
            self._bufs[key] = {"skip": bf(n, 64, h, w), "a": bf(n, 64, h, w), "b": bf(n, 64, h, w), "c": bf(n, 64, h, w), "g": bf(n, 64, h, w),
                               "stages": stages, "chunk": ch,
                               "y": torch.empty(n, 3, f * h, f * w, dtype=torch.float32, device=dev)}
        return self._bufs[key]

    def _plan(self, n, h, w, band_rows=None, out_kind=L.OUT_F32_NCHW):
        if band_rows is not None:
            raise NotImplementedError(self.SERVED_TAIL)
        one = band_plan(h, self.k, len(self.ups), None)
        if not _fits(one[0], w, len(self.ups), self.TAIL_CHANNELS, self.TAIL_LIMIT, out_kind != L.OUT_F32_NCHW):
            raise NotImplementedError(self.SERVED_TAIL)
        return self._tail_chunk(n, h, w), tuple(one)

    def _gate(self, gate, u, cin, m, y, n, h, w):
        (wg, bg), k, rt = gate, self.k, self.rt
        d = L.ConvDesc(n, cin, h, w, m.shape[3], h, w, k, k, 1, k // 2, k // 2)
        L.check(rt.lib.vcg_conv_in_gate_bf16_fwd(ctypes.byref(d), u.data_ptr(), wg.data_ptr(), bg.data_ptr(), m.data_ptr(), y.data_ptr(), rt.stream),
                "vcg_conv_in_gate_bf16_fwd")

    def forward(self, x, out_kind=L.OUT_F32_NCHW, band_rows=None):
        """x: device fp32 NCHW [n,3,h,w] in [-1,1] -> device fp32 NCHW [n,3,f*h,f*w], or with out_kind OUT_U8_NHWC device uint8 frames
        [n,f*h,f*w,3] (f = upscale_factor; buffer owned by the engine)"""
        rt = self.rt
        n, _, h, w = x.shape
        self._plan(n, h, w, band_rows, out_kind)          # refuses what the tail does not serve
        B = self._buffers(n, h, w)
        out = self._trunk(x, B, lambda gate, m, g: self._gate(gate, x, 3, m, g, n, h, w))
        # the gates' inputs: data derived from the frames alone, for the whole batch
        for s, st in enumerate(B["stages"]):
            r, hw = 2 ** s, h * w
            for off, bil in ((0, 0), (3, 1)):
                src = x
                if r > 1:
                    L.check(rt.lib.vcg_resize2d(x.data_ptr(), st["t"].data_ptr(), n * 3, h, w, r, bil, rt.stream), "vcg_resize2d")
                    src = st["t"]
                L.check(rt.lib.vcg_copy_channels(src.data_ptr(), st["u"].data_ptr(), n, 3, 0, 6, off, 3, r * r * hw, rt.stream), "vcg_copy_channels")
        k, crop = self.k, max(self.k - 2, 0) // 2           # TF-SAME crop of Conv2DTranspose(k, strides 2): k3 (0, 1), k5 (1, 2)
        ch, f = B["chunk"], 2 ** len(self.ups)
        if out_kind == L.OUT_U8_NHWC:
            if "y8" not in B:
                B["y8"] = torch.empty(n, f * h, f * w, 3, dtype=torch.uint8, device=rt.device)
            y = B["y8"]
        else:
            y = B["y"]
        for i in range(0, n, ch):
            c = min(ch, n - i)
            src, hh, ww = out[i:i + c], h, w
            for s, ((gate, wt, bt, slope, cin, cout, wa, ba), st) in enumerate(zip(self.ups, B["stages"])):
                scale = 2 ** (s + 1)
                self._gate(gate, st["u"][i:i + c], 6, src, st["g"], c, hh, ww)
                dt = L.ConvDesc(c, cin, hh, ww, cout, 2 * hh, 2 * ww, k, k, 2, crop, crop)
                L.check(rt.lib.vcg_conv_transpose2d_nhwc_bf16_fwd(ctypes.byref(dt), st["g"].data_ptr(), wt.data_ptr(), bt.data_ptr(), L.ACT_LRELU,
                                                                  slope, st["y"].data_ptr(), rt.stream), "vcg_conv_transpose2d_nhwc_bf16_fwd")
                da = L.ConvDesc(c, 3, h, w, cout, scale * h, scale * w, scale + 1, scale + 1, scale, 0, 0)
                L.check(rt.lib.vcg_input_convt_add_bf16(ctypes.byref(da), x[i:i + c].data_ptr(), wa.data_ptr(), ba.data_ptr(), st["y"].data_ptr(),
                                                        rt.stream), "vcg_input_convt_add_bf16")
                src, hh, ww = st["y"], 2 * hh, 2 * ww
            self._to3(src, y[i:i + c], out_kind)       # uint8: the whole frame as one window, final/conv stores the uint8 NHWC frames
        return y


class Bf16CycleGanGenerator(Bf16Generator):
    """The same engine for ``make_generator_cyclegan`` models (_graph.py; BASELINE.json north_star's generator shape, SURVEY.md section 8
    row a11), filters 64 on RGB frames, norm 'instance' or 'batch', kernel_size 3 or 5, n_downsample 1 or 2, upscale_factor 1, 2 or 4, any
    res_block_num:

        stem/conv 9x9 3->64 + bias                              vcg_conv9x9_from3_bf16_fwd without activation -> z
        down/i/conv k s2 (64 -> 128 -> 256) + bias              vcg_conv2d_nhwc_bf16_fwd[_stats] -> z
        res_block/i/conv_pre | conv_post k s1 + bias            the same
        up/i/conv_transp k s2 (halving, not below 64) + bias    vcg_conv_transpose2d_nhwc_bf16_fwd -> z
        the norm + PReLU (+ Add of the block input) behind every one of them: vcg_norm_act_fwd_bf16 on z, with
            instance norm: per-image scale / shift from the convolution's epilogue records (vcg_norm_finalize_partials) where its tiled
                           kernel serves the shape, otherwise from vcg_norm_stats_bf16 + vcg_norm_finalize -- the statistics of the
                           stored bf16 z either way;
            batch norm:    per-channel scale / shift of the moving statistics (vcg_bn_fold without bias: the bias is in z), made in refresh()
        head/conv 9x9 64->3 + tanh                              vcg_conv9x9_c64to3_bf16_fwd, or its window form over the whole frame for
                                                                uint8 frames

    Activations are bf16 NHWC, the weights are rounded to bf16 once in refresh(); biases, norm and PReLU parameters stay fp32.
    capture / replay / predict / upscale_frames are Bf16Generator's.  The generic kernels address the whole batch of a launch with 32-bit
    offsets, so the pass runs on chunks of frames whose largest tensor fits LAUNCH_LIMIT bytes, spread evenly (instance statistics are
    per image and inference BatchNormalization per pixel: chunking changes no value).  No row bands."""
    LAUNCH_LIMIT = TAIL_LIMIT          # bytes of a launch's largest tensor; a class attribute so that a test can lower it
    SERVED = "bf16 inference of make_generator_cyclegan is instantiated for filters=64 on 3-channel (RGB) frames, norm 'instance' or " \
             "'batch', kernel_size 3 or 5, n_downsample 1 or 2 and upscale_factor 1, 2 or 4 (any res_block_num); use model.predict for " \
             "other shapes"
    SERVED_SIZE = "bf16 inference of make_generator_cyclegan runs on whole frames (band_rows=None) whose largest tensor, f*h x f*w x 64 " \
                  "channels in bf16, fits a launch of 4 GiB; row bands are served for make_upscaler_orig models only"

    def __init__(self, model):
        cfg = getattr(model, "cyclegan_generator", None)
        if cfg is None or not hasattr(model, "graph"):
            raise TypeError("Bf16CycleGanGenerator serves make_generator_cyclegan models")
        if cfg["filters"] != 64 or cfg["channels"] != 3 or cfg["norm"] not in ("instance", "batch") or cfg["kernel_size"] not in (3, 5) \
                or cfg["n_downsample"] not in (1, 2) or cfg["upscale_factor"] not in (1, 2, 4):
            raise NotImplementedError(self.SERVED)
        self.k, self.n_downsample, self.res_block_num = cfg["kernel_size"], cfg["n_downsample"], cfg["res_block_num"]
        self.upscale_factor = cfg["upscale_factor"]
        self.legacy = False
        self.instance = cfg["norm"] == "instance"
        self.model = model
        self.rt = model.rt
        self.layers = {l.name: l for l in model.layers}
        self._graphs = {}
        self._bufs = {}
        self.refresh()

    def _factor(self):
        return self.upscale_factor

    # ---- parameters ------------------------------------------------------------------------------------------
    def _op(self, kind, conv, norm, out, residual=False):
        """one convolution and the norm (+ PReLU, + Add) behind it.  kind: 'stem' | 'conv' | 'convt'; out: the name of the stored result"""
        rt, ps, ly = self.rt, self.model.ps, self.layers
        cv, nm = ly[conv], ly[norm]
        if kind == "stem":
            w = E.pack_first9x9_bf16(rt, ps[conv + "/kernel"])
        else:               # the generic kernels' fragments: mode 0 for a Conv2D, mode 1 for a Conv2DTranspose (_pack)
            w = E.pack_conv_frag_bf16(rt, ps[conv + "/kernel"], cv.k * cv.k, cv.cout, cv.cin, 1 if kind == "convt" else 0)
        scale = shift = None
        if not self.instance:
            scale, shift = rt.empty(cv.cout), rt.empty(cv.cout)
            L.check(rt.lib.vcg_bn_fold(None, ps[norm + "/moving_mean"].data_ptr(), ps[norm + "/moving_variance"].data_ptr(),
                                       ps[norm + "/gamma"].data_ptr(), ps[norm + "/beta"].data_ptr(), cv.cout, E.BN_EPS, scale.data_ptr(),
                                       shift.data_ptr(), rt.stream), "vcg_bn_fold")
        alpha = ps[nm.prelu_name + "/alpha"] if nm.act == L.ACT_PRELU else None
        return {"kind": kind, "conv": conv, "layer": cv, "w": w, "bias": ps[conv + "/bias"], "scale": scale, "shift": shift, "alpha": alpha,
                "out": out, "residual": residual}

    def refresh(self):
        """(re)derive the packed bf16 weights and the BatchNormalization scale / shift vectors from the model's parameters"""
        ops = [self._op("stem", "stem/conv", "stem/norm", "stem/prelu")]
        for i in range(self.n_downsample):
            ops.append(self._op("conv", "down/%d/conv" % i, "down/%d/norm" % i, "down/%d/prelu" % i))
        for i in range(self.res_block_num):
            n = "res_block/%d" % i
            ops.append(self._op("conv", n + "/conv_pre", n + "/batch_norm_pre", n + "/prelu"))
            ops.append(self._op("conv", n + "/conv_post", n + "/batch_norm_post", n + "/final_add", residual=True))
        self.ups = []
        for i in range(self.n_downsample + {1: 0, 2: 1, 4: 2}[self.upscale_factor]):
            self.ups.append(self._op("convt", "up/%d/conv_transp" % i, "up/%d/norm" % i, "up/%d/prelu" % i))
        self.ops = ops + self.ups
        ps = self.model.ps
        self.final = (E.pack_conv9x9_c64to3_bf16(self.rt, ps["head/conv/kernel"]), ps["head/conv/bias"])
        self._graphs.clear()          # recorded graphs hold the old parameter buffers
        self._bufs.clear()            # (the plans name the operands of the ops above)
        self._staging = None          # upscale_frames' pinned and device staging buffers

    # ---- launch plan -----------------------------------------------------------------------------------------
    def _shapes(self, h, w):
        """[(cin, ih, iw, cout, oh, ow)] of self.ops for h x w frames"""
        if h % (1 << self.n_downsample) or w % (1 << self.n_downsample):
            raise ValueError("frames of %d x %d are not divisible by 2**n_downsample" % (h, w))
        out, c = [], 3
        for op in self.ops:
            cv = op["layer"]
            oh, ow = (2 * h, 2 * w) if op["kind"] == "convt" else cv.out_hw(h, w)[:2]
            out.append((c, h, w, cv.cout, oh, ow))
            c, h, w = cv.cout, oh, ow
        return out

    def _chunk(self, n, h, w):
        """frames per launch: as many as keep every tensor of the pass within LAUNCH_LIMIT bytes, spread evenly over the launches"""
        shapes = self._shapes(h, w)
        f = self._factor()
        per = max(max(ci * ih * iw, co * oh * ow) for (ci, ih, iw, co, oh, ow) in shapes[1:]) * 2
        per = max(per, shapes[0][3] * h * w * 2)
        # head/conv's descriptor covers one image, four rows above and four below it
        if per > self.LAUNCH_LIMIT or (f * h + 8) * f * w * 128 + 65536 > self.LAUNCH_LIMIT:
            raise NotImplementedError(self.SERVED_SIZE)
        ch = max(1, min(n, self.LAUNCH_LIMIT // per))
        launches = -(-n // ch)
        return -(-n // launches)

    def _plan(self, n, h, w, band_rows=None, out_kind=L.OUT_F32_NCHW):
        if band_rows is not None:
            raise NotImplementedError(self.SERVED_SIZE)
        return self._chunk(n, h, w), ()

    def _launches(self, c, h, w):
        """the pass for c frames of h x w pixels: per op its descriptor, buffers and -- decided here, once per layer shape -- whether the
        instance statistics come out of the convolution's epilogue (records > 0) or from a pass over z"""
        key = ("pass", c, h, w)
        if key in self._bufs:
            return self._bufs[key]
        rt, dev, pool = self.rt, self.rt.device, {}

        def buf(role, hh, ww, cc):
            if (role, hh, ww, cc) not in pool:
                pool[(role, hh, ww, cc)] = torch.empty(c, hh, ww, cc, dtype=torch.bfloat16, device=dev)
            return pool[(role, hh, ww, cc)]

        steps, cur, block_in, crop, maxrec = [], None, None, max(self.k - 2, 0) // 2, 0
        for op, (ci, ih, iw, co, oh, ow) in zip(self.ops, self._shapes(h, w)):
            cv, nrec = op["layer"], -1
            if op["kind"] == "stem":
                d = L.ConvDesc(c, 3, ih, iw, co, oh, ow, 9, 9, 1, 4, 4)
            elif op["kind"] == "convt":          # TF-SAME crop of Conv2DTranspose(k, strides 2): k3 (0, 1), k5 (1, 2)
                d = L.ConvDesc(c, ci, ih, iw, co, oh, ow, self.k, self.k, 2, crop, crop)
            else:
                d = cv.desc(c, ih, iw)
                if self.instance:
                    nrec = rt.lib.vcg_conv2d_nhwc_bf16_stats_records(ctypes.byref(d), L.STATS_INSTANCE)
                    maxrec = max(maxrec, nrec * co)
            if op["conv"].endswith("/conv_pre"):
                block_in = cur
            # outputs: a residual block's PReLU in "b", its sum in whichever of "a" / "c" does not hold the block input; everything else
            # in "a" of its own shape (two consecutive layers outside the trunk never share one)
            role = "b" if op["conv"].endswith("/conv_pre") else "a"
            if op["residual"] and block_in is buf("a", oh, ow, co):
                role = "c"
            y = buf(role, oh, ow, co)
            steps.append({"op": op, "d": d, "x": cur, "z": buf("z", oh, ow, co), "y": y, "nrec": nrec, "c": co, "hw": oh * ow,
                          "res": block_in if op["residual"] else None})
            cur = y
        P = {"steps": steps, "last": cur,
             "stats": torch.empty(5, c * 256, dtype=torch.float32, device=dev) if self.instance else None,
             "part": torch.empty(max(1, c * maxrec * 2), dtype=torch.float32, device=dev) if self.instance else None}
        self._bufs[key] = P
        return P

    def stats_records(self, n, h, w):
        """{convolution name: records per image of its epilogue statistics, or a negative number where a separate pass over z makes them}
        for the instance-norm layers of one launch of n frames (what the tests assert the covered paths with)"""
        return {s["op"]["conv"]: s["nrec"] for s in self._launches(n, h, w)["steps"] if s["op"]["kind"] == "conv"}

    # ---- one forward pass --------------------------------------------------------------------------------------
    def _norm(self, P, s):
        """the norm (+ PReLU, + Add) behind a convolution: z -> y"""
        op = s["op"]
        self._norm_act(s["z"], s["y"], P["stats"], op["alpha"], s["res"], s["nrec"], P["part"], op["scale"], op["shift"])

    def _conv_step(self, P, s, x):
        """the convolution (+ bias) of one step: its input (the frames x for the stem) -> z, with the statistics records where planned"""
        rt = self.rt
        op, d, z = s["op"], s["d"], s["z"]
        if op["kind"] == "stem":
            self._stem(x, op["w"], op["bias"], None, z)
        elif op["kind"] == "convt":
            L.check(rt.lib.vcg_conv_transpose2d_nhwc_bf16_fwd(ctypes.byref(d), s["x"].data_ptr(), op["w"].data_ptr(), op["bias"].data_ptr(),
                                                              L.ACT_NONE, 0.0, z.data_ptr(), rt.stream), "vcg_conv_transpose2d_nhwc_bf16_fwd")
        elif s["nrec"] > 0:
            L.check(rt.lib.vcg_conv2d_nhwc_bf16_fwd_stats(ctypes.byref(d), s["x"].data_ptr(), op["w"].data_ptr(), op["bias"].data_ptr(),
                                                          z.data_ptr(), P["part"].data_ptr(), rt.stream), "vcg_conv2d_nhwc_bf16_fwd_stats")
        else:
            L.check(rt.lib.vcg_conv2d_nhwc_bf16_fwd(ctypes.byref(d), s["x"].data_ptr(), op["w"].data_ptr(), op["bias"].data_ptr(),
                                                    L.ACT_NONE, 0.0, z.data_ptr(), rt.stream), "vcg_conv2d_nhwc_bf16_fwd")

    def _pass(self, x, y, out_kind, taps):
        """the pass on one chunk: x fp32 NCHW [c,3,h,w] -> y (its frames of the output buffer)"""
        c, _, h, w = x.shape
        P = self._launches(c, h, w)

        def tap(name, t):
            if taps is not None:
                taps[name] = torch.cat([taps[name], t.clone()], 0) if name in taps else t.clone()

        for s in P["steps"]:
            self._conv_step(P, s, x)
            tap(s["op"]["conv"], s["z"])
            self._norm(P, s)
            tap(s["op"]["out"], s["y"])
        self._to3(P["last"], y, out_kind)           # uint8: the whole frame as one window, head/conv stores the uint8 NHWC frames
        tap("head/conv", y)

    def forward(self, x, out_kind=L.OUT_F32_NCHW, band_rows=None, taps=None):
        """x: device fp32 NCHW [n,3,h,w] in [-1,1] -> device fp32 NCHW [n,3,f*h,f*w], or with out_kind OUT_U8_NHWC device uint8 frames
        [n,f*h,f*w,3] (f = upscale_factor; buffer owned by the engine).  taps: a dict that receives a clone of every tensor the pass
        stores, keyed by layer name ("stem/conv", "stem/prelu", ..., "res_block/0/final_add", ..., "head/conv"): a debugging hook for
        eager calls, never used inside a capture"""
        n, _, h, w = x.shape
        ch, _ = self._plan(n, h, w, band_rows, out_kind)
        f = self._factor()
        key = ("y", n, h, w, out_kind)
        if key not in self._bufs:
            self._bufs[key] = (torch.empty(n, f * h, f * w, 3, dtype=torch.uint8, device=self.rt.device) if out_kind == L.OUT_U8_NHWC
                               else torch.empty(n, 3, f * h, f * w, dtype=torch.float32, device=self.rt.device))
        y = self._bufs[key]
        for i in range(0, n, ch):
            self._pass(x[i:i + ch], y[i:i + ch], out_kind, taps)
        return y


class Bf16IncepResnetGenerator(Bf16Generator):
    """The same engine for ``make_upscaler_incep_resnet`` models (upscaling/upscaler/model.py:443-497; train_gan3.py's ``-gm inc-resnet``),
    filters 64 on RGB frames, upscale_factor a power of two >= 2, any number (0 included) of '3path' (kernel 3 or 5) and '2path' (kernel 3, 5
    or 7) blocks, c_block_kernel 3 or 5:

        initial/conv/9x9 3->64 + bias (no activation: the long skip)   vcg_conv9x9_from3_bf16_fwd
        3-path block (model.py:386-412), 5 launches:
            a/1, b/1, c/1: BN + PReLU of m on load, 1x1, + b/2's and c/2's BN + PReLU    vcg_incep_head_bf16_fwd  -> a1 (raw), b1, c1 (activated)
            b/2 kxk 32->32 + bias; c/2 kxk 32->48 + c/3's BN + PReLU; c/3 kxk 48->64 + bias   vcg_conv2d_nhwc_bf16_fwd_epilogue
            final/concat + final/1x1 + final/add                                         vcg_incep_join_bf16_fwd on (a1, b2, c3) and m
        2-path block (model.py:416-439), 4 launches:
            a/1, b/1 (32, 19 channels) + b/2's BN + PReLU                                vcg_incep_head_bf16_fwd
            b/2 1xk 19->25 + b/3's BN + PReLU; b/3 kx1 25->32 + bias                     vcg_conv2d_nhwc_bf16_fwd_epilogue
            final/concat + final/1x1 + final/add                                         vcg_incep_join_bf16_fwd on (a1, b3) and m
        prefinal/conv2d + batch_norm + Add(long skip)                                    vcg_conv2d_bf16_fwd (kernel = c_block_kernel)
        upscaling/i/block (64 -> 256 -> 256) and final/conv 9x9 256->3 + tanh            Bf16Generator's tail, kernel = c_block_kernel

    A tensor with one consumer is stored behind that consumer's BatchNormalization + PReLU (pre-activation mini-blocks, model.py:372-382);
    19-, 25- and 48-channel tensors are stored on 32 / 32 / 64 channels, zeros in the padding (include/vcg.h).  _fold, _pack, the tail with its
    row bands and uint8 frames, capture / replay / predict / upscale_frames are Bf16Generator's."""
    SERVED = "bf16 inference of make_upscaler_incep_resnet is instantiated for filters=64 on 3-channel (RGB) frames, upscale_factor a power " \
             "of two >= 2, block types '3path' (kernel 3 or 5) and '2path' (kernel 3, 5 or 7) in any number, and c_block_kernel 3 or 5; use " \
             "model.predict for other shapes"

    def __init__(self, model):
        cfg = getattr(model, "incep_resnet_generator", None)
        if cfg is None or not hasattr(model, "graph"):
            raise TypeError("Bf16IncepResnetGenerator serves make_upscaler_incep_resnet models")
        f = cfg["upscale_factor"]
        ok = cfg["filters"] == 64 and cfg["channels"] == 3 and isinstance(f, int) and f >= 2 and f & (f - 1) == 0 and cfg["c_block_kernel"] in (3, 5)
        self.groups = []
        for tag in ("a", "b", "c"):
            btype, num, kern = cfg[tag + "_block_type"], cfg[tag + "_block_num"], cfg[tag + "_block_kernel"]
            if num and (btype not in ("3path", "2path") or kern not in {"3path": (3, 5), "2path": (3, 5, 7)}[btype]):
                ok = False
            self.groups.append((tag.upper() if tag != "c" else "c", btype, num, kern))          # 'c' in lower case: model.py:479,481
        if not ok:
            raise NotImplementedError(self.SERVED)
        self.k = cfg["c_block_kernel"]
        self.legacy = False
        self.instance = False
        self.model = model
        self.rt = model.rt
        self.layers = {l.name: l for l in model.layers}
        self._graphs = {}
        self._bufs = {}
        self._taps = None
        self.refresh()

    # ---- parameters ------------------------------------------------------------------------------------------
    def _block(self, n, btype, k):
        """the launches of one block: head paths, middle layers, join sources; a tensor is named after the layer whose OUTPUT it is"""
        rt, ps = self.rt, self.model.ps
        conv_name = lambda mini, kh, kw: "%s/%s/%dx%d" % (n, mini, kh, kw)
        if btype == "3path":       # (mini-block, kernel, cout, its single consumer's mini-block or None, input buffer, output buffer)
            heads = [("a/1", 32, None, "hA"), ("b/1", 32, "b/2", "hB"), ("c/1", 32, "c/2", "hC")]
            mids = [("b/2", (k, k), 32, 32, None, "hB", "t32"), ("c/2", (k, k), 32, 48, "c/3", "hC", "t64"), ("c/3", (k, k), 48, 64, None, "t64", "u64")]
            srcs = [("hA", 32), ("t32", 32), ("u64", 64)]
        else:
            heads = [("a/1", 32, None, "hA"), ("b/1", 19, "b/2", "hB")]
            mids = [("b/2", (1, k), 19, 25, "b/3", "hB", "t32"), ("b/3", (k, 1), 25, 32, None, "t32", "hC")]
            srcs = [("hA", 32), ("hC", 32)]

        def epilogue(conv, nxt):
            """the layer's bias and, where its output has one consumer, that mini-block's BatchNormalization + PReLU"""
            if nxt is None:
                return E.incep_fold(rt, ps, self.layers[conv].cout, bias=conv) + (conv,)
            return E.incep_fold(rt, ps, self.layers[conv].cout, bias=conv, norm="%s/%s/batch_norm" % (n, nxt), prelu="%s/%s/prelu" % (n, nxt)) \
                + ("%s/%s/prelu" % (n, nxt),)

        blk = {"name": n, "heads": [], "mids": [], "srcs": []}
        for mini, cout, nxt, out in heads:
            conv = conv_name(mini, 1, 1)
            pre = E.incep_fold(rt, ps, 64, norm="%s/%s/batch_norm" % (n, mini), prelu="%s/%s/prelu" % (n, mini))
            blk["heads"].append({"cout": cout, "pre": pre, "w": E.pack_incep_frag_bf16(rt, ps[conv + "/kernel"], 1, 64, cout), "ep": epilogue(conv, nxt),
                                 "out": out})
        for mini, (kh, kw), cin, cout, nxt, src, out in mids:
            conv = conv_name(mini, kh, kw)
            blk["mids"].append({"kh": kh, "kw": kw, "cin": cin, "cout": cout, "w": E.pack_incep_frag_bf16(rt, ps[conv + "/kernel"], kh * kw, cin, cout),
                                "ep": epilogue(conv, nxt), "in": src, "out": out})
        total, k0 = sum(c for _, c in srcs), 0
        for src, c in srcs:
            blk["srcs"].append((src, c, E.pack_incep_frag_bf16(rt, ps[n + "/final/1x1/kernel"], 1, total, 64, k0, c)))
            k0 += c
        blk["bias"] = ps[n + "/final/1x1/bias"]
        return blk

    def refresh(self):
        """(re)derive the packed bf16 weights and the folded BatchNormalization vectors from the model's parameters"""
        rt, ly, ps = self.rt, self.layers, self.model.ps
        self.first = (E.pack_first9x9_bf16(rt, ps["initial/conv/9x9/kernel"]), ps["initial/conv/9x9/bias"], None)
        self.blocks = []
        for tag, btype, num, kern in self.groups:
            for index in range(num):
                self.blocks.append(self._block("inc_res_block/%s/%s/%d" % (tag, {"3path": "3p", "2path": "2p"}[btype], index), btype, kern))
        cp = ly["prefinal/conv2d"]
        self.prefinal = (self._pack(cp, 1),) + tuple(self._fold(cp, ly["prefinal/batch_norm"]))
        self.up_layers = []
        while "upscaling/%d/block/conv_transp" % len(self.up_layers) in ly:
            self.up_layers.append(ly["upscaling/%d/block/conv_transp" % len(self.up_layers)])
        self.ups = [(self._pack(up, 0), ps[up.name + "/bias"], float(up.alpha), up.cin) for up in self.up_layers]
        self.final = (E.pack_final9x9_bf16(rt, ps["final/conv/kernel"]), ps["final/conv/bias"])
        self._graphs.clear()          # recorded graphs hold the old parameter buffers
        self._staging = None          # upscale_frames' pinned and device staging buffers

    # ---- one forward pass ------------------------------------------------------------------------------------
    def _trunk_buffers(self, n, h, w):
        key = ("trunk", n, h, w)
        if key not in self._bufs:
            bf = lambda c: torch.empty(n, h, w, c, dtype=torch.bfloat16, device=self.rt.device)
            self._bufs[key] = {"skip": bf(64), "a": bf(64), "c": bf(64), "t64": bf(64), "u64": bf(64),
                               "hA": bf(32), "hB": bf(32), "hC": bf(32), "t32": bf(32)}
        return self._bufs[key]

    def _tap(self, name, t):
        if self._taps is not None:
            self._taps[name] = t.clone()

    def _run_block(self, blk, m, out, B, n, h, w):
        rt = self.rt
        paths = (L.IncepHeadPath * len(blk["heads"]))()
        hd = L.IncepHeadDesc(n, h, w, 64, len(blk["heads"]))
        for i, hp in enumerate(blk["heads"]):
            (isc, ish, ial), (osc, osh, oal, _) = hp["pre"], hp["ep"]
            hd.cout[i] = hp["cout"]
            paths[i] = L.IncepHeadPath(isc.data_ptr(), ish.data_ptr(), ial.data_ptr(), hp["w"].data_ptr(), osc.data_ptr(), osh.data_ptr(),
                                       oal.data_ptr() if oal is not None else None, B[hp["out"]].data_ptr())
        L.check(rt.lib.vcg_incep_head_bf16_fwd(ctypes.byref(hd), m.data_ptr(), paths, rt.stream), "vcg_incep_head_bf16_fwd")
        for hp in blk["heads"]:
            self._tap(hp["ep"][3], B[hp["out"]])
        for md in blk["mids"]:
            sc, sh, al, name = md["ep"]
            d = L.ConvDesc(n, md["cin"], h, w, md["cout"], h, w, md["kh"], md["kw"], 1, md["kh"] // 2, md["kw"] // 2)
            ep = L.EpilogueBf16(sc.data_ptr(), sh.data_ptr(), L.ACT_PRELU if al is not None else L.ACT_NONE, 0.0,
                                al.data_ptr() if al is not None else None, None)
            L.check(rt.lib.vcg_conv2d_nhwc_bf16_fwd_epilogue(ctypes.byref(d), B[md["in"]].data_ptr(), md["w"].data_ptr(), B[md["out"]].data_ptr(),
                                                             ctypes.byref(ep), rt.stream), "vcg_conv2d_nhwc_bf16_fwd_epilogue")
            self._tap(name, B[md["out"]])
        ns = len(blk["srcs"])
        jd = L.IncepJoinDesc(n, h, w, 64, ns)
        for i, (_, c, _) in enumerate(blk["srcs"]):
            jd.cin[i] = c
        z = (ctypes.c_void_p * ns)(*[B[s].data_ptr() for s, _, _ in blk["srcs"]])
        wf = (ctypes.c_void_p * ns)(*[wj.data_ptr() for _, _, wj in blk["srcs"]])
        L.check(rt.lib.vcg_incep_join_bf16_fwd(ctypes.byref(jd), z, wf, blk["bias"].data_ptr(), m.data_ptr(), out.data_ptr(), rt.stream),
                "vcg_incep_join_bf16_fwd")
        self._tap(blk["name"] + "/final/add", out)

    def _trunk(self, x, B, gate=None):
        n, _, h, w = x.shape
        self._stem(x, *self.first, B["skip"])
        self._tap("initial/conv/9x9", B["skip"])
        cur = B["skip"]                     # block input; outputs ping-pong between "a" and "c", "skip" is never overwritten
        for blk in self.blocks:
            out = B["a"] if cur is not B["a"] else B["c"]
            self._run_block(blk, cur, out, B, n, h, w)
            cur = out
        wp, sp, hp = self.prefinal
        out = B["a"] if cur is not B["a"] else B["c"]
        self._conv(cur, wp, out, sp, hp, L.ACT_NONE, None, B["skip"], n, h, w)
        self._tap("prefinal/tanh", out)
        return out

    def launches(self):
        """kernel launches of one pass on whole frames in one chunk: stem + 5 / 4 per block + prefinal + the tail's stages + final/conv"""
        return 1 + sum(1 + len(b["mids"]) + 1 for b in self.blocks) + 1 + len(self.ups) + 1

    def forward(self, x, out_kind=L.OUT_F32_NCHW, band_rows=None, taps=None):
        """Bf16Generator.forward; taps: a dict that receives a clone of every tensor the trunk stores, keyed by the name of the layer whose
        output it is -- a convolution's ("initial/conv/9x9", ".../a/1/1x1", ".../b/2/3x3") where the raw sum is stored, the consumer's PReLU
        (".../b/2/prelu") where the epilogue activates, ".../final/add", "prefinal/tanh" -- and, on the unbanded fp32 path in one chunk, the
        up-sampling stages' ("upscaling/i/block/conv_transp") and "final/conv": a debugging hook for eager calls, never used inside a capture"""
        self._taps = taps
        try:
            y = super().forward(x, out_kind, band_rows)
        finally:
            self._taps = None
        if taps is not None:
            n, _, h, w = x.shape
            B = self._bufs.get((n, h, w))
            if B is not None and y is B["y"] and B["us"][0].shape[0] == n:
                for i, u in enumerate(B["us"]):
                    taps["upscaling/%d/block/conv_transp" % i] = u.clone()
            taps["final/conv"] = y.clone()
        return y

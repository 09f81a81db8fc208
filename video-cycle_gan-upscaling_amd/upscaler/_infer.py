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
    final/conv 9x9 256->3 + tanh              vcg_conv9x9_to3_bf16_fwd (fp32 NCHW out)

The 5x5 trunk convolutions run on the same entry point (the generic kernels' plan, weights as their MFMA fragments), and the
up-sampling stages that convt3x3_c64 does not serve -- 5x5, and 3x3 on 256 channels -- on vcg_conv_transpose2d_nhwc_bf16_fwd,
one per stage (64->256, then 256->256).  22 launches for the k3 x2
topology, recorded once per input shape into a hipGraph and replayed per batch.  Activations are bf16 NHWC,
accumulation and the epilogue arithmetic fp32; the weights are rounded to bf16 once, when the engine is built or
``refresh()`` is called after a weight update.  The folded BatchNormalization parameters
(scale = gamma / sqrt(moving_var + 1e-3), shift = (bias - moving_mean) * scale + beta) are 64-element fp32 vectors
derived by vcg_axpby + vcg_norm_finalize when the engine is built or refreshed."""
import ctypes
import os

import numpy as np
import torch

from . import _engine as E
from . import _lib as L


class Bf16Generator:
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
        self.ups = [(self._pack(up, 0), up.ps[up.name + "/bias"], float(up.alpha), up.cin) for up in m.ups]
        self.up = self.ups[0][:3]
        self.final = (E.pack_final9x9_bf16(rt, m.c_fin.ps[m.c_fin.name + "/kernel"]), m.c_fin.ps[m.c_fin.name + "/bias"])
        self.first = (E.pack_first9x9_bf16(rt, m.c_init.ps[m.c_init.name + "/kernel"]), m.c_init.ps[m.c_init.name + "/bias"],
                      m.c_init.ps[m.a_init.prelu_name + "/alpha"])
        self._graphs.clear()          # recorded graphs hold the old parameter buffers

    # ---- one forward pass (22 launches) -----------------------------------------------------------------------
    def _buffers(self, n, h, w):
        key = (n, h, w)
        if key not in self._bufs:
            dev = self.rt.device
            bf = lambda c, hh, ww: torch.empty(n, hh, ww, c, dtype=torch.bfloat16, device=dev)
            ch = self._tail_chunk(n, h, w)
            f = 2 ** len(self.ups)
            # one bf16 NHWC buffer per up-sampling stage: [ch, 2h, 2w, 256], [ch, 4h, 4w, 256], ...
            us = [torch.empty(ch, 2 ** (s + 1) * h, 2 ** (s + 1) * w, 256, dtype=torch.bfloat16, device=dev) for s in range(len(self.ups))]
            self._bufs[key] = {"skip": bf(64, h, w),
                               "a": bf(64, h, w), "b": bf(64, h, w), "c": bf(64, h, w),
                               "u": us[0], "us": us,
                               "z": bf(64, h, w) if self.instance else None,
                               "stats": torch.empty(5, n * 64, dtype=torch.float32, device=dev) if self.instance else None,
                               "y": torch.empty(n, 3, f * h, f * w, dtype=torch.float32, device=dev)}
        return self._bufs[key]

    def _tail_chunk(self, n, h, w):
        """frames per launch of the up-sampling stages and final/conv.  Beyond the k3 x2 topology, a launch's largest tensor (the
        last stage's output, 2 * 256 bytes per pixel) stays below 4 GiB: the kernels' offsets are 32-bit inside an image, and final/conv's
        descriptor covers the whole launch"""
        if self.legacy:
            return n
        f = 2 ** len(self.ups)
        per = f * f * h * w * self.TAIL_CHANNELS * 2
        ch = max(1, min(n, 0xFFFFFFE0 // per))
        launches = -(-n // ch)
        return -(-n // launches)                 # the same number of launches, frames spread evenly (32 -> 16 + 16, not 31 + 1)

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
        z = self._buffers(n, h, wd)["z"]
        k = self.k
        d = L.ConvDesc(n, 64, h, wd, 64, h, wd, k, k, 1, k // 2, k // 2)
        ep = L.EpilogueBf16(None, bias.data_ptr(), L.ACT_NONE, 0.0, None, None)
        L.check(rt.lib.vcg_conv2d_bf16_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), z.data_ptr(), ctypes.byref(ep), rt.stream),
                "vcg_conv2d_bf16_fwd")
        st = self._buffers(n, h, wd)["stats"]
        mean, var, scale, shift, invstd = (st[i] for i in range(5))
        ws, wsn = rt.workspace(rt.lib.vcg_norm_stats_bf16_workspace_bytes(n, 64, h * wd, L.NORM_INSTANCE))
        L.check(rt.lib.vcg_norm_stats_bf16(z.data_ptr(), n, 64, h * wd, L.NORM_INSTANCE, mean.data_ptr(), var.data_ptr(), ws, wsn,
                                           rt.stream), "vcg_norm_stats_bf16")
        L.check(rt.lib.vcg_norm_finalize(mean.data_ptr(), var.data_ptr(), None, None, 64, n, E.IN_EPS, scale.data_ptr(), shift.data_ptr(),
                                         invstd.data_ptr(), None, None, 0.0, 0, rt.stream), "vcg_norm_finalize")
        L.check(rt.lib.vcg_norm_act_fwd_bf16(z.data_ptr(), n, 64, h * wd, scale.data_ptr(), shift.data_ptr(), 1, act, 0.0,
                                             alpha.data_ptr() if alpha is not None else None,
                                             res.data_ptr() if res is not None else None, y.data_ptr(), rt.stream),
                "vcg_norm_act_fwd_bf16")

    def forward(self, x):
        """x: device fp32 NCHW [n,3,h,w] in [-1,1] -> device fp32 NCHW [n,3,f*h,f*w] (f = upscale_factor; buffer owned by the engine)"""
        rt, m = self.rt, self.model
        n, _, h, w = x.shape
        B = self._buffers(n, h, w)
        w0, b0, a0 = self.first
        d0 = L.ConvDesc(n, 3, h, w, 64, h, w, 9, 9, 1, 4, 4)
        L.check(rt.lib.vcg_conv9x9_from3_bf16_fwd(ctypes.byref(d0), x.data_ptr(), w0.data_ptr(), b0.data_ptr(), a0.data_ptr(),
                                                  B["skip"].data_ptr(), rt.stream), "vcg_conv9x9_from3_bf16_fwd")
        cur = B["skip"]                     # block input; outputs ping-pong between "a" and "c", "skip" is never overwritten
        for (w1, s1, h1, al, w2, s2, h2) in self.trunk:
            out = B["a"] if cur is not B["a"] else B["c"]
            self._conv(cur, w1, B["b"], s1, h1, L.ACT_PRELU, al, None, n, h, w)
            self._conv(B["b"], w2, out, s2, h2, L.ACT_NONE, None, cur, n, h, w)
            cur = out
        wp, sp, hp = self.prefinal
        out = B["a"] if cur is not B["a"] else B["c"]
        self._conv(cur, wp, out, sp, hp, L.ACT_NONE, None, B["skip"], n, h, w)
        wf, bf_ = self.final
        k, crop = self.k, max(self.k - 2, 0) // 2           # TF-SAME crop of Conv2DTranspose(k, strides 2): k3 (0, 1), k5 (1, 2)
        us, y = B["us"], B["y"]
        ch = us[0].shape[0]
        for i in range(0, n, ch):
            c = min(ch, n - i)
            src, hh, ww = out[i:i + c], h, w
            for (wt, bt, slope, cin), up, u in zip(self.ups, m.ups, us):
                dt = L.ConvDesc(c, cin, hh, ww, 256, 2 * hh, 2 * ww, k, k, 2, crop, crop)
                if self._generic(up, 0):
                    L.check(rt.lib.vcg_conv_transpose2d_nhwc_bf16_fwd(ctypes.byref(dt), src.data_ptr(), wt.data_ptr(), bt.data_ptr(), L.ACT_LRELU,
                                                                      slope, u.data_ptr(), rt.stream), "vcg_conv_transpose2d_nhwc_bf16_fwd")
                else:
                    ept = L.EpilogueBf16(None, bt.data_ptr(), L.ACT_LRELU, slope, None, None)
                    L.check(rt.lib.vcg_conv_transpose2d_bf16_fwd(ctypes.byref(dt), src.data_ptr(), wt.data_ptr(), u.data_ptr(), ctypes.byref(ept),
                                                                 rt.stream), "vcg_conv_transpose2d_bf16_fwd")
                src, hh, ww = u, 2 * hh, 2 * ww
            df = L.ConvDesc(c, 256, hh, ww, 3, hh, ww, 9, 9, 1, 4, 4)
            L.check(rt.lib.vcg_conv9x9_to3_bf16_fwd(ctypes.byref(df), src.data_ptr(), wf.data_ptr(), bf_.data_ptr(), 1, y[i:i + c].data_ptr(),
                                                    rt.stream), "vcg_conv9x9_to3_bf16_fwd")
        return B["y"]

    # ---- hipGraph ---------------------------------------------------------------------------------------------
    def capture(self, n, h, w):
        """record the pass for one input shape; ``replay(x)`` then costs one graph launch"""
        key = (n, h, w)
        if key in self._graphs:
            return self._graphs[key]
        xin = torch.zeros(n, 3, h, w, dtype=torch.float32, device=self.rt.device)
        self.forward(xin)                  # warm-up: buffers exist, kernel attributes are set
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            y = self.forward(xin)
        self._graphs[key] = (g, xin, y)
        return self._graphs[key]

    def replay(self, x):
        g, xin, y = self.capture(*[x.shape[0], x.shape[2], x.shape[3]])
        xin.copy_(x)
        g.replay()
        return y

    # ---- Keras-style entry point -------------------------------------------------------------------------------
    def predict(self, x, batch_size=32):
        """x: numpy NHWC in [-1,1] (data.py:266-270) -> numpy NHWC float32, through the captured graph"""
        rt = self.rt
        x = np.asarray(x)
        outs = []
        for i in range(0, x.shape[0], batch_size):
            xb = E.to_device_nchw(rt, x[i:i + batch_size])
            y = self.replay(xb)
            outs.append(E.to_nhwc(rt, y).cpu().numpy())
        return np.concatenate(outs, 0)


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
        final/conv 9x9 128->3 + tanh                            vcg_conv9x9_to3_bf16_fwd (cin 128)

    3 launches per residual block; _fold, _pack, capture / replay / predict and the 4 GiB chunking of the tail are Bf16Generator's."""
    TAIL_CHANNELS = 128
    SERVED = "bf16 inference of make_upscaler_attention is instantiated for filters=64 on 3-channel (RGB) frames, norm='batch', " \
             "kernel_size 3 or 5 and upscale_factor 2 or 4 (any res_block_num); use model.predict for other shapes"

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

    def _gate(self, gate, u, cin, m, y, n, h, w):
        (wg, bg), k, rt = gate, self.k, self.rt
        d = L.ConvDesc(n, cin, h, w, m.shape[3], h, w, k, k, 1, k // 2, k // 2)
        L.check(rt.lib.vcg_conv_in_gate_bf16_fwd(ctypes.byref(d), u.data_ptr(), wg.data_ptr(), bg.data_ptr(), m.data_ptr(), y.data_ptr(), rt.stream),
                "vcg_conv_in_gate_bf16_fwd")

    def forward(self, x):
        """x: device fp32 NCHW [n,3,h,w] in [-1,1] -> device fp32 NCHW [n,3,f*h,f*w] (f = upscale_factor; buffer owned by the engine)"""
        rt = self.rt
        n, _, h, w = x.shape
        B = self._buffers(n, h, w)
        w0, b0, a0 = self.first
        d0 = L.ConvDesc(n, 3, h, w, 64, h, w, 9, 9, 1, 4, 4)
        L.check(rt.lib.vcg_conv9x9_from3_bf16_fwd(ctypes.byref(d0), x.data_ptr(), w0.data_ptr(), b0.data_ptr(), a0.data_ptr(),
                                                  B["skip"].data_ptr(), rt.stream), "vcg_conv9x9_from3_bf16_fwd")
        cur = B["skip"]                     # block input; outputs ping-pong between "a" and "c", "skip" is never overwritten
        for (gate, w1, s1, h1, al, w2, s2, h2) in self.trunk:
            out = B["a"] if cur is not B["a"] else B["c"]
            self._gate(gate, x, 3, cur, B["g"], n, h, w)
            self._conv(B["g"], w1, B["b"], s1, h1, L.ACT_PRELU, al, None, n, h, w)
            self._conv(B["b"], w2, out, s2, h2, L.ACT_NONE, None, cur, n, h, w)          # Add of the ungated block input
            cur = out
        wp, sp, hp = self.prefinal
        out = B["a"] if cur is not B["a"] else B["c"]
        self._conv(cur, wp, out, sp, hp, L.ACT_NONE, None, B["skip"], n, h, w)
        # the gates' inputs: data derived from the frames alone, for the whole batch
        for s, st in enumerate(B["stages"]):
            r, hw = 2 ** s, h * w
            for off, bil in ((0, 0), (3, 1)):
                src = x
                if r > 1:
                    L.check(rt.lib.vcg_resize2d(x.data_ptr(), st["t"].data_ptr(), n * 3, h, w, r, bil, rt.stream), "vcg_resize2d")
                    src = st["t"]
                L.check(rt.lib.vcg_copy_channels(src.data_ptr(), st["u"].data_ptr(), n, 3, 0, 6, off, 3, r * r * hw, rt.stream), "vcg_copy_channels")
        wf, bf_, cfin = self.final
        k, crop = self.k, max(self.k - 2, 0) // 2           # TF-SAME crop of Conv2DTranspose(k, strides 2): k3 (0, 1), k5 (1, 2)
        y, ch = B["y"], B["chunk"]
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
            df = L.ConvDesc(c, cfin, hh, ww, 3, hh, ww, 9, 9, 1, 4, 4)
            L.check(rt.lib.vcg_conv9x9_to3_bf16_fwd(ctypes.byref(df), src.data_ptr(), wf.data_ptr(), bf_.data_ptr(), 1, y[i:i + c].data_ptr(),
                                                    rt.stream), "vcg_conv9x9_to3_bf16_fwd")
        return y

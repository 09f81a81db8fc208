"""Device engine: parameter storage and layer forward/backward on top of the C ABI (include/vcg.h).

torch is used only for device memory (torch.empty), the current HIP stream and host<->device
copies; every arithmetic step is a libvcg_hip.so kernel.  Activations are fp32 NCHW.

Layer <-> reference call sites (upscaling/upscaler/model.py):
  Conv2D            :19,22,275,283,290,839-871     ConvT2D   :72
  NormAct           :20-25,276,284-285,840-841     Dense     :876-884
"""
import ctypes
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L

BN_EPS = 1e-3          # keras BatchNormalization defaults
BN_MOMENTUM = 0.99
IN_EPS = 1e-5          # instance norm (canonical CycleGAN value; no reference counterpart)


def same_pads(size, k, s):
    """TF SAME: out = ceil(in/s); total = max((out-1)*s+k-in, 0); before = total//2."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2, total - total // 2


class Runtime:
    """Per-process handle: library, device, grow-only workspace."""

    _inst = None

    def __init__(self):
        self.lib = L.load()
        self.device = L.require_gpu()
        self._ws = None
        self._ws_retired = []   # outgrown workspaces stay allocated: recorded hipGraphs keep writing through their pointers
        self.prof = None      # optional kernel-timing hook set by bench.py

    @classmethod
    def get(cls):
        if cls._inst is None:
            cls._inst = Runtime()
        return cls._inst

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def workspace(self, nbytes):
        """scratch for partial sums (wgrad / norm / loss reductions), shared by all layers on the stream.  It only grows,
        and an outgrown buffer is never freed: a captured train step or inference graph has its address baked into its
        kernel nodes and would otherwise write into memory the allocator may have handed to a live tensor.  Doubling
        keeps the retired buffers below the size of the current one in total."""
        nbytes = max(int(nbytes), 4096)
        if self._ws is None or self._ws.numel() < nbytes:
            if self._ws is not None:
                self._ws_retired.append(self._ws)
                nbytes = max(nbytes, 2 * self._ws.numel())
            self._ws = torch.empty(nbytes + 4096, dtype=torch.uint8, device=self.device)
        return self._ws.data_ptr(), self._ws.numel()

    def empty(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    def zeros(self, *shape):
        t = self.empty(*shape)
        L.check(self.lib.vcg_fill(t.data_ptr(), t.numel(), 0.0, self.stream), "vcg_fill")
        return t


def _ptr(t):
    return None if t is None else t.data_ptr()


class Timed:
    """Context manager used by bench.py to bracket launches of one kernel family with HIP events
    on the stream the kernels run on."""

    def __init__(self, rt, tag):
        self.rt, self.tag = rt, tag

    def __enter__(self):
        p = self.rt.prof
        if p is not None and self.tag in p.tags:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        else:
            self.e0 = None

    def __exit__(self, *a):
        if self.e0 is not None:
            self.e1.record()
            self.rt.prof.events.setdefault(self.tag, []).append((self.e0, self.e1))


# =================================================================================================
# parameter store: one flat fp32 buffer of trainables (+grads), one of non-trainable state
# =================================================================================================
class ParamStore:
    def __init__(self):
        self.specs = OrderedDict()   # name -> (shape, trainable, init)
        self.params = None
        self.state = None
        self.grads = None
        self.grads2 = None
        self.views = {}
        self.gviews = {}
        self.g2views = {}

    def declare(self, name, shape, trainable=True):
        if name in self.specs:
            raise ValueError("duplicate weight " + name)
        self.specs[name] = (tuple(int(s) for s in shape), trainable)

    def materialize(self, rt):
        nt = sum(int(np.prod(s)) for s, t in self.specs.values() if t)
        ns = sum(int(np.prod(s)) for s, t in self.specs.values() if not t)
        self.params = rt.zeros(max(nt, 1))
        self.grads = rt.zeros(max(nt, 1))
        self.grads2 = rt.zeros(max(nt, 1))
        self.state = rt.zeros(max(ns, 1))
        ot = os_ = 0
        self.offsets = {}
        for name, (shape, trainable) in self.specs.items():
            n = int(np.prod(shape))
            if trainable:
                self.views[name] = self.params[ot:ot + n].view(shape)
                self.gviews[name] = self.grads[ot:ot + n].view(shape)
                self.g2views[name] = self.grads2[ot:ot + n].view(shape)
                self.offsets[name] = ot
                ot += n
            else:
                self.views[name] = self.state[os_:os_ + n].view(shape)
                os_ += n
        self.n_trainable, self.n_state = nt, ns

    def __getitem__(self, name):
        return self.views[name]

    def grad(self, name, which=0):
        return (self.gviews if which == 0 else self.g2views)[name]

    def count_params(self):
        return sum(int(np.prod(s)) for s, _ in self.specs.values())

    def set_weights(self, weights):
        """weights: dict name -> array (Keras layouts).  Unknown / missing names raise."""
        for name, arr in weights.items():
            if name not in self.views:
                raise KeyError("unknown weight " + name)
            a = np.ascontiguousarray(np.asarray(arr, dtype=np.float32))
            if tuple(a.shape) != self.specs[name][0]:
                raise ValueError("shape mismatch for %s: %s vs %s" % (name, a.shape, self.specs[name][0]))
            self.views[name].copy_(torch.from_numpy(a))
        missing = [n for n in self.specs if n not in weights]
        return missing

    def get_weights(self):
        return OrderedDict((n, self.views[n].detach().cpu().numpy().copy()) for n in self.specs)


# =================================================================================================
# initialisers (Keras defaults)
# =================================================================================================
def glorot_uniform(rng, shape, fan_in, fan_out):
    limit = math.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-limit, limit, size=shape).astype(np.float32)


# =================================================================================================
# layers
# =================================================================================================
class Layer:
    def __init__(self, name):
        self.name = name
        self.rt = None
        self.ps = None
        self.caches = []        # the layer's PackedOperands

    def bind(self, rt, ps):
        self.rt, self.ps = rt, ps

    def init_weights(self, rng):
        return {}

    def refresh(self):
        """called after the parameters changed (optimizer step / set_weights)"""
        for c in self.caches:
            c.stale = True


class PackedOperand:
    """Device copy of a layer's kernel in the layout a kernel reads.  ``build(bufs)`` fills the buffers from the parameters (bufs None on
    first use: it allocates them) and returns them; it runs when the copy is asked for while stale, never on refresh() itself.

    The buffers keep their addresses for the life of the layer: get() stores what build returns only once and hands build the same
    buffers back ever after.  A captured train step has the pack launches and the kernels reading these addresses baked into its nodes;
    a buffer replaced after an optimizer step would leave the graph re-packing into, and reading from, freed memory."""

    def __init__(self, build, *layers):
        self.build, self.bufs, self.stale = build, None, True
        for l in layers:
            l.caches.append(self)

    def get(self):
        if self.stale:
            bufs = self.build(self.bufs)
            self.bufs = bufs if self.bufs is None else self.bufs
            self.stale = False
        return self.bufs


def act_bwd_bias(layer, y, dy, d, param_grads, which):
    """backward of a convolution's fused activation: dz = act'(y) * dy, the bias gradient (per-channel sum of dz) out of the same pass"""
    rt = layer.rt
    hw = d.oh * d.ow
    dz = rt.empty(*dy.shape)
    db = layer.ps.grad(layer.name + "/bias", which).data_ptr() if param_grads else None
    ws, wsn = rt.workspace(rt.lib.vcg_act_bwd_workspace_bytes(d.n, layer.cout, hw))
    L.check(rt.lib.vcg_act_bwd(y.data_ptr(), dy.data_ptr(), d.n, layer.cout, hw, layer.act, float(layer.alpha),
                               None, dz.data_ptr(), None, db, ws, wsn, rt.stream), "vcg_act_bwd[%s]" % layer.name)
    return dz


def kernel_transpose(rt, w, taps, a, b, out=None):
    """fp32 per-tap transpose of a kernel [taps][a][b] -> [taps][b][a] (the fp32 data-gradient / transposed-convolution operand)"""
    out = rt.empty(taps, b, a) if out is None else out
    L.check(rt.lib.vcg_kernel_transpose(w.data_ptr(), out.data_ptr(), taps, a, b, rt.stream), "vcg_kernel_transpose")
    return out


class Conv2D(Layer):
    """keras.layers.Conv2D(+fused bias/LeakyReLU/tanh epilogue).  padding: 'same' | 'valid' | int; k: int or (kh, kw)."""

    def __init__(self, name, cin, cout, k, stride=1, padding="same", act=L.ACT_NONE, alpha=0.0):
        super().__init__(name)
        self.kh, self.kw = (int(k[0]), int(k[1])) if isinstance(k, (tuple, list)) else (int(k), int(k))
        self.cin, self.cout, self.k, self.stride, self.padding = cin, cout, self.kh, stride, padding     # k: the square layers' size
        self.act, self.alpha = act, alpha
        # per-tap transposed kernel (kh,kw,out,in): the fp32 data gradient's second operand
        self._wt = PackedOperand(lambda out: kernel_transpose(self.rt, self.ps[self.name + "/kernel"], self.kh * self.kw, self.cin, self.cout, out), self)

    def declare(self, ps):
        ps.declare(self.name + "/kernel", (self.kh, self.kw, self.cin, self.cout))
        ps.declare(self.name + "/bias", (self.cout,))

    def init_weights(self, rng):
        t = self.kh * self.kw
        return {self.name + "/kernel": glorot_uniform(rng, (self.kh, self.kw, self.cin, self.cout), t * self.cin, t * self.cout),
                self.name + "/bias": np.zeros((self.cout,), np.float32)}

    def out_hw(self, h, w):
        kh, kw, s = self.kh, self.kw, self.stride
        if self.padding == "same":
            oh, pt, _ = same_pads(h, kh, s)
            ow, pl, _ = same_pads(w, kw, s)
        elif self.padding == "valid":
            oh, ow, pt, pl = (h - kh) // s + 1, (w - kw) // s + 1, 0, 0
        else:
            p = int(self.padding)
            oh, ow, pt, pl = (h + 2 * p - kh) // s + 1, (w + 2 * p - kw) // s + 1, p, p
        return oh, ow, pt, pl

    def desc(self, n, h, w):
        oh, ow, pt, pl = self.out_hw(h, w)
        return L.ConvDesc(n, self.cin, h, w, self.cout, oh, ow, self.kh, self.kw, self.stride, pt, pl)

    def forward(self, x, residual=None, tag=None):
        rt = self.rt
        n, _, h, w = x.shape
        d = self.desc(n, h, w)
        y = rt.empty(n, self.cout, d.oh, d.ow)
        ep = L.Epilogue(_ptr(self.ps[self.name + "/bias"]), self.act, float(self.alpha), None, _ptr(residual))
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv2d_fwd(ctypes.byref(d), x.data_ptr(), self.ps[self.name + "/kernel"].data_ptr(),
                                          y.data_ptr(), ctypes.byref(ep), rt.stream), "vcg_conv2d_fwd[%s]" % self.name)
        return y, (x, y if self.act != L.ACT_NONE else None, d)

    def forward_prelu(self, x, alpha, training=False, tag=None):
        """learning phase 0: conv + bias + the PReLU behind the layer (per-channel slopes ``alpha``) in one launch.  The training pass
        keeps the pre-activation on the tape and runs the two layers."""
        if training or self.act != L.ACT_NONE:
            raise NotImplementedError("Conv2D.forward_prelu: the predict pass of a layer without an activation of its own")
        rt = self.rt
        n, _, h, w = x.shape
        d = self.desc(n, h, w)
        y = rt.empty(n, self.cout, d.oh, d.ow)
        ep = L.Epilogue(_ptr(self.ps[self.name + "/bias"]), L.ACT_PRELU, 0.0, alpha.data_ptr(), None)
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv2d_fwd(ctypes.byref(d), x.data_ptr(), self.ps[self.name + "/kernel"].data_ptr(),
                                          y.data_ptr(), ctypes.byref(ep), rt.stream), "vcg_conv2d_fwd[%s]" % self.name)
        return y

    def forward_folded(self, x, norm, residual=None, folded=None, tag=None):
        """learning phase 0: conv + BatchNormalization (moving statistics) [+ PReLU / LeakyReLU] [+ Add] in ONE launch: the convolution's
        epilogue applies the normalisation's per-channel (scale, shift) behind its bias (vcg_conv2d_fwd_affine; the weights are not
        scaled, and the result has the bits of the separate launches).  norm: the NormAct behind this convolution (batch norm).
        folded: its (scale, shift) already derived (finalize_batch).  Where the layer's kernel has no such epilogue the convolution and
        vcg_norm_act_fwd run one after the other."""
        rt, ps = self.rt, self.ps
        if self.act != L.ACT_NONE or norm.norm != "batch":
            raise NotImplementedError("Conv2D.forward_folded: a convolution without activation in front of a BatchNormalization")
        n, _, h, w = x.shape
        d = self.desc(n, h, w)
        if folded is not None:
            scale, shift = folded
        else:
            scale, shift = finalize_batch(rt, [norm])[id(norm)]
        y = rt.empty(n, self.cout, d.oh, d.ow)
        ep = L.Epilogue(_ptr(ps[self.name + "/bias"]), norm.act, float(norm.alpha), norm._alpha_ptr(), _ptr(residual))
        with Timed(rt, tag):
            rc = rt.lib.vcg_conv2d_fwd_affine(ctypes.byref(d), x.data_ptr(), ps[self.name + "/kernel"].data_ptr(), y.data_ptr(), ctypes.byref(ep),
                                              scale.data_ptr(), shift.data_ptr(), rt.stream)
        if rc != L.E_UNSUPPORTED:
            L.check(rc, "vcg_conv2d_fwd_affine[%s]" % self.name)
            return y
        z, _ = self.forward(x, tag=tag)
        L.check(rt.lib.vcg_norm_act_fwd(z.data_ptr(), n, self.cout, d.oh * d.ow, scale.data_ptr(), shift.data_ptr(), 0, norm.act, float(norm.alpha),
                                        norm._alpha_ptr(), _ptr(residual), y.data_ptr(), rt.stream), "vcg_norm_act_fwd[%s]" % norm.name)
        return y

    def forward_stats(self, x, instance, tag=None):
        """forward (bias, no activation) whose epilogue leaves the statistics of the normalisation behind the layer: returns
        (y, ctx, (records, records per group, shift)) for NormAct.forward(stats=...), or stats None where the layer's kernel has no
        statistics epilogue (the normalisation then reads y itself)"""
        rt = self.rt
        n, _, h, w = x.shape
        d = self.desc(n, h, w)
        nrec = rt.lib.vcg_conv2d_stats_records(ctypes.byref(d), L.STATS_INSTANCE if instance else L.STATS_BATCH)
        if nrec <= 0 or self.act != L.ACT_NONE:
            y, ctx = self.forward(x, tag=tag)
            return y, ctx, None
        y = rt.empty(n, self.cout, d.oh, d.ow)
        total = nrec * (n if instance else 1)
        rec = rt.empty(total * 2 * self.cout)
        bias = self.ps[self.name + "/bias"]
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv2d_fwd_stats(ctypes.byref(d), x.data_ptr(), self.ps[self.name + "/kernel"].data_ptr(), bias.data_ptr(),
                                                y.data_ptr(), rec.data_ptr(), rt.stream), "vcg_conv2d_fwd_stats[%s]" % self.name)
        return y, (x, None, d), (rec, nrec, bias)

    def backward(self, ctx, dy, need_dx=True, param_grads=True, which=0, dx_residual=None, tag=None):
        rt = self.rt
        x, y, d = ctx
        n = d.n
        db_done = self.act != L.ACT_NONE
        if db_done:
            dy = act_bwd_bias(self, y, dy, d, param_grads, which)
        if param_grads:
            self._wgrad_fp32(d, x, dy, which, not db_done, tag)
        dx = None
        if need_dx:
            dx = rt.empty(n, self.cin, d.h, d.w)
            dd, dyd = d, dy
            if self.stride > 2:
                # sparse_512's stride-3 layers: the data gradient as a stride-1 correlation over the zero-dilated gradient
                s = self.stride
                dyd = rt.empty(n, self.cout, (d.oh - 1) * s + 1, (d.ow - 1) * s + 1)
                L.check(rt.lib.vcg_dilate2d(dy.data_ptr(), dyd.data_ptr(), n * self.cout, d.oh, d.ow, s, rt.stream), "vcg_dilate2d")
                dd = L.ConvDesc(n, self.cin, d.h, d.w, self.cout, dyd.shape[2], dyd.shape[3], self.kh, self.kw, 1, d.pad_top, d.pad_left)
            with Timed(rt, tag and tag + "_dgrad"):
                L.check(rt.lib.vcg_conv2d_dgrad(ctypes.byref(dd), dyd.data_ptr(), self.ps[self.name + "/kernel"].data_ptr(),
                                                self._wt.get().data_ptr(), dx.data_ptr(), _ptr(dx_residual), rt.stream),
                        "vcg_conv2d_dgrad[%s]" % self.name)
        return dx

    def _wgrad_fp32(self, d, x, dy, which, with_bias, tag):
        """fp32 weight gradient of the convolution d from fp32 NCHW x and dy (with_bias: and the bias gradient, the per-channel sum of dy)"""
        rt = self.rt
        ws, wsn = rt.workspace(rt.lib.vcg_conv2d_wgrad_workspace_bytes(ctypes.byref(d)))
        with Timed(rt, tag and tag + "_wgrad"):
            L.check(rt.lib.vcg_conv2d_wgrad(ctypes.byref(d), x.data_ptr(), dy.data_ptr(), self.ps.grad(self.name + "/kernel", which).data_ptr(),
                                            self.ps.grad(self.name + "/bias", which).data_ptr() if with_bias else None, ws, wsn, rt.stream),
                    "vcg_conv2d_wgrad[%s]" % self.name)


class ConvT2D(Layer):
    """keras.layers.Conv2DTranspose(strides=2, padding='same') + fused LeakyReLU (model.py:72-73)."""

    def __init__(self, name, cin, cout, k, act=L.ACT_NONE, alpha=0.0):
        super().__init__(name)
        self.cin, self.cout, self.k, self.act, self.alpha = cin, cout, k, act, alpha
        # per-tap transposed kernel (k,k,in,out)
        self._wt = PackedOperand(lambda out: kernel_transpose(self.rt, self.ps[self.name + "/kernel"], k * k, cout, cin, out), self)

    def declare(self, ps):
        ps.declare(self.name + "/kernel", (self.k, self.k, self.cout, self.cin))
        ps.declare(self.name + "/bias", (self.cout,))

    def init_weights(self, rng):
        k = self.k
        return {self.name + "/kernel": glorot_uniform(rng, (k, k, self.cout, self.cin), k * k * self.cout, k * k * self.cin),
                self.name + "/bias": np.zeros((self.cout,), np.float32)}

    def desc(self, n, h, w):
        crop = max(self.k - 2, 0) // 2
        return L.ConvDesc(n, self.cin, h, w, self.cout, 2 * h, 2 * w, self.k, self.k, 2, crop, crop)

    def forward(self, x, tag=None):
        rt = self.rt
        n, _, h, w = x.shape
        d = self.desc(n, h, w)
        y = rt.empty(n, self.cout, d.oh, d.ow)
        ep = L.Epilogue(_ptr(self.ps[self.name + "/bias"]), self.act, float(self.alpha), None, None)
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv_transpose2d_fwd(ctypes.byref(d), x.data_ptr(), self._wt.get().data_ptr(), y.data_ptr(),
                                                    ctypes.byref(ep), rt.stream), "vcg_conv_transpose2d_fwd[%s]" % self.name)
        return y, (x, y if self.act != L.ACT_NONE else None, d)

    def backward(self, ctx, dy, need_dx=True, param_grads=True, which=0, tag=None):
        rt = self.rt
        x, y, d = ctx
        db_done = self.act != L.ACT_NONE
        if db_done:
            dy = act_bwd_bias(self, y, dy, d, param_grads, which)
        if param_grads:
            need = rt.lib.vcg_conv_transpose2d_wgrad_workspace_bytes(ctypes.byref(d))
            ws, wsn = rt.workspace(need)
            with Timed(rt, tag and tag + "_wgrad"):
                L.check(rt.lib.vcg_conv_transpose2d_wgrad(ctypes.byref(d), x.data_ptr(), dy.data_ptr(),
                                                          self.ps.grad(self.name + "/kernel", which).data_ptr(),
                                                          None if db_done else self.ps.grad(self.name + "/bias", which).data_ptr(),
                                                          ws, wsn, rt.stream), "vcg_conv_transpose2d_wgrad[%s]" % self.name)
        dx = None
        if need_dx:
            dx = rt.empty(d.n, self.cin, d.h, d.w)
            with Timed(rt, tag and tag + "_dgrad"):
                L.check(rt.lib.vcg_conv_transpose2d_dgrad(ctypes.byref(d), dy.data_ptr(),
                                                          self.ps[self.name + "/kernel"].data_ptr(), dx.data_ptr(), None,
                                                          rt.stream), "vcg_conv_transpose2d_dgrad[%s]" % self.name)
        return dx


class ConvTDilated(ConvT2D):
    """keras.layers.Conv2DTranspose(strides=s, padding='same') for any stride, as the data gradient of the stride-1 convolution its
    Keras kernel (kh, kw, out, in) is the HWIO kernel of, evaluated over the zero-dilated input: the ``to_add_input`` branch of the x4
    attention generator (kernel 5, strides 4, model.py:95).  That branch transposes a function of the network INPUT, so only the
    forward pass and the parameter gradients exist here; asking for the input gradient raises."""

    def __init__(self, name, cin, cout, k, stride):
        super().__init__(name, cin, cout, k, L.ACT_NONE, 0.0)
        if k < stride:
            raise NotImplementedError("Conv2DTranspose with kernel_size < strides")
        self.stride = stride
        self._ones = None

    def _descs(self, n, h, w):
        s, k = self.stride, self.k
        hd, wd = (h - 1) * s + 1, (w - 1) * s + 1
        crop = (k - s) // 2                                   # 'same': the full transposed convolution, cropped crop / k - s - crop
        # the virtual convolution: [cout, h*s, w*s] -> [cin, hd, wd], stride 1, pads (crop, crop)
        return hd, wd, L.ConvDesc(n, self.cout, h * s, w * s, self.cin, hd, wd, k, k, 1, crop, crop)

    def forward(self, x, tag=None):
        rt = self.rt
        n, _, h, w = x.shape
        hd, wd, d = self._descs(n, h, w)
        xd = rt.empty(n, self.cin, hd, wd)
        L.check(rt.lib.vcg_dilate2d(x.data_ptr(), xd.data_ptr(), n * self.cin, h, w, self.stride, rt.stream), "vcg_dilate2d")
        z = rt.empty(n, self.cout, d.h, d.w)
        L.check(rt.lib.vcg_conv2d_dgrad(ctypes.byref(d), xd.data_ptr(), self.ps[self.name + "/kernel"].data_ptr(), self._wt.get().data_ptr(), z.data_ptr(),
                                        None, rt.stream), "vcg_conv2d_dgrad[%s]" % self.name)
        if self._ones is None:
            self._ones = filled_like(rt, self.ps[self.name + "/bias"], 1.0)
        y = rt.empty(*z.shape)                                 # + bias: y = 1 * z + bias[c]
        L.check(rt.lib.vcg_norm_act_fwd(z.data_ptr(), n, self.cout, d.h * d.w, self._ones.data_ptr(), self.ps[self.name + "/bias"].data_ptr(), 0,
                                        L.ACT_NONE, 0.0, None, None, y.data_ptr(), rt.stream), "vcg_norm_act_fwd[%s]" % self.name)
        return y, (xd, d)

    def backward(self, ctx, dy, need_dx=True, param_grads=True, which=0, tag=None):
        rt = self.rt
        xd, d = ctx
        if need_dx:
            raise NotImplementedError("Conv2DTranspose(strides=%d): the input gradient is not built (the reference applies it to the network input)"
                                      % self.stride)
        if param_grads:
            ws, wsn = rt.workspace(max(rt.lib.vcg_conv2d_wgrad_workspace_bytes(ctypes.byref(d)),
                                       rt.lib.vcg_channel_sum_workspace_bytes(d.n, self.cout, d.h * d.w)))
            # dL/dW[tap][out][in] = sum dy[out][i + tap - crop] * xd[in][i]: the weight gradient of the virtual convolution with x := dy, dy := xd
            L.check(rt.lib.vcg_conv2d_wgrad(ctypes.byref(d), dy.data_ptr(), xd.data_ptr(), self.ps.grad(self.name + "/kernel", which).data_ptr(), None,
                                            ws, wsn, rt.stream), "vcg_conv2d_wgrad[%s]" % self.name)
            L.check(rt.lib.vcg_channel_sum(dy.data_ptr(), d.n, self.cout, d.h * d.w, self.ps.grad(self.name + "/bias", which).data_ptr(), ws, wsn,
                                           rt.stream), "vcg_channel_sum[%s]" % self.name)
        return None


def finalize_batch(rt, norms):
    """{id(norm): (scale, shift)} of the fp32 batch-norm NormActs of a learning-phase-0 pass from their moving statistics: one
    vcg_norm_finalize_batch launch per 48 layers of equal width (what NormAct.forward(training=False) derives per layer)"""
    out = {}
    by_c = {}
    for nm in norms:
        by_c.setdefault(nm.c, []).append(nm)
    for c, group in by_c.items():
        for at in range(0, len(group), 48):
            part = group[at:at + 48]
            n = len(part)
            buf = rt.empty(2, n, c)
            col = lambda key: (ctypes.c_void_p * n)(*[nm.ps[nm.name + key].data_ptr() for nm in part])
            L.check(rt.lib.vcg_norm_finalize_batch(col("/moving_mean"), col("/moving_variance"), col("/gamma"), col("/beta"), n, c, BN_EPS,
                                                   buf[0].data_ptr(), buf[1].data_ptr(), rt.stream), "vcg_norm_finalize_batch")
            for i, nm in enumerate(part):
                out[id(nm)] = (buf[0, i], buf[1, i])
    return out


class NormAct(Layer):
    """[BatchNormalization | instance norm | identity] -> [PReLU | LeakyReLU | none] -> [+ residual].

    norm: 'batch' (Keras BN, gamma/beta/moving stats), 'instance' (non-affine), None.
    act: ACT_NONE / ACT_LRELU / ACT_PRELU; PReLU owns a per-channel alpha named ``prelu_name``."""

    def __init__(self, name, c, norm="batch", act=L.ACT_NONE, alpha=0.0, prelu_name=None):
        super().__init__(name)
        self.c, self.norm, self.act, self.alpha, self.prelu_name = c, norm, act, alpha, prelu_name

    def declare(self, ps):
        if self.norm == "batch":
            ps.declare(self.name + "/gamma", (self.c,))
            ps.declare(self.name + "/beta", (self.c,))
            ps.declare(self.name + "/moving_mean", (self.c,), trainable=False)
            ps.declare(self.name + "/moving_variance", (self.c,), trainable=False)
        if self.act == L.ACT_PRELU:
            ps.declare(self.prelu_name + "/alpha", (self.c,))

    def init_weights(self, rng):
        w = {}
        if self.norm == "batch":
            w[self.name + "/gamma"] = np.ones((self.c,), np.float32)
            w[self.name + "/beta"] = np.zeros((self.c,), np.float32)
            w[self.name + "/moving_mean"] = np.zeros((self.c,), np.float32)
            w[self.name + "/moving_variance"] = np.ones((self.c,), np.float32)
        if self.act == L.ACT_PRELU:
            w[self.prelu_name + "/alpha"] = np.zeros((self.c,), np.float32)
        return w

    def _alpha_ptr(self):
        return self.ps[self.prelu_name + "/alpha"].data_ptr() if self.act == L.ACT_PRELU else None

    def needs_stats(self, training):
        """does forward(x, training) compute statistics of x (so that a producer's epilogue may hand them over)"""
        return self.norm is not None and bool(training or self.norm == "instance")

    # what NormActBf16 replaces: the entry points over the activation tensor, its shape decoding and allocation, and _finalize_partials
    STATS, ACT_FWD, ACT_BWD = "vcg_norm_stats", "vcg_norm_act_fwd", "vcg_norm_act_bwd"

    def _dims(self, x):
        """(n, c, h*w) of fp32 NCHW or 2-D [n, c]"""
        if x.dim() == 4:
            n, c, h, w = x.shape
            return n, c, h * w
        n, c = x.shape
        return n, c, 1

    def _like(self, x):
        return self.rt.empty(*x.shape)

    def _finalize_partials(self, stats, rows, c, count, gamma, beta, eps, mean, scale, shift, invstd, mm, mv, unbiased_n):
        """(records, records per group, shift) of Conv2D.forward_stats -> mean / scale / shift / invstd (+ moving statistics)"""
        buf, nrec, kshift = stats
        L.check(self.rt.lib.vcg_norm_finalize_partials_shifted(buf.data_ptr(), nrec, rows, c, count, kshift.data_ptr(), gamma, beta, eps,
                                                               mean.data_ptr(), scale.data_ptr(), shift.data_ptr(), invstd.data_ptr(), mm, mv,
                                                               BN_MOMENTUM, unbiased_n, self.rt.stream),
                "vcg_norm_finalize_partials_shifted[%s]" % self.name)

    def forward(self, x, training, residual=None, update_moving=True, stats=None):
        """stats: what the producing convolution's forward_stats left behind -- one finalize-from-partials launch then replaces the
        statistics pass over x and vcg_norm_finalize"""
        rt, ps = self.rt, self.ps
        lib = rt.lib
        n, c, hw = self._dims(x)
        y = self._like(x)
        saved = None
        act_fwd = getattr(lib, self.ACT_FWD)
        if self.norm is None:
            L.check(act_fwd(x.data_ptr(), n, c, hw, None, None, 0, self.act, float(self.alpha),
                            self._alpha_ptr(), _ptr(residual), y.data_ptr(), rt.stream), self.ACT_FWD)
            return y, (x, None, None, (n, c, hw))
        inst = self.norm == "instance"
        rows = n if inst else 1
        mode = L.NORM_INSTANCE if inst else L.NORM_BATCH
        scale, shift, invstd = rt.empty(rows * c), rt.empty(rows * c), rt.empty(rows * c)
        gamma = None if inst else ps[self.name + "/gamma"].data_ptr()
        beta = None if inst else ps[self.name + "/beta"].data_ptr()
        eps = IN_EPS if inst else BN_EPS
        if training or inst:
            mean = rt.empty(rows * c)
            mm = mv = None
            if not inst and update_moving:
                mm, mv = ps[self.name + "/moving_mean"].data_ptr(), ps[self.name + "/moving_variance"].data_ptr()
            # Keras' TF backend: fused path (4-D) reports the Bessel-corrected variance to the moving
            # average, the 2-D path (Dense BN) the biased one
            ub = (n * hw) if (x.dim() == 4 and not inst) else 0
            if stats is not None:
                self._finalize_partials(stats, rows, c, float(hw if inst else n * hw), gamma, beta, eps, mean, scale, shift, invstd, mm, mv, ub)
            else:
                var = rt.empty(rows * c)
                ws, wsn = rt.workspace(getattr(lib, self.STATS + "_workspace_bytes")(n, c, hw, mode))
                L.check(getattr(lib, self.STATS)(x.data_ptr(), n, c, hw, mode, mean.data_ptr(), var.data_ptr(), ws, wsn, rt.stream),
                        "%s[%s]" % (self.STATS, self.name))
                L.check(lib.vcg_norm_finalize(mean.data_ptr(), var.data_ptr(), gamma, beta, c, rows, eps, scale.data_ptr(), shift.data_ptr(),
                                              invstd.data_ptr(), mm, mv, BN_MOMENTUM, ub, rt.stream), "vcg_norm_finalize")
            saved = (mean, invstd)
        else:
            L.check(lib.vcg_norm_finalize(ps[self.name + "/moving_mean"].data_ptr(),
                                          ps[self.name + "/moving_variance"].data_ptr(), gamma, beta, c, 1, BN_EPS,
                                          scale.data_ptr(), shift.data_ptr(), invstd.data_ptr(), None, None, 0.0, 0,
                                          rt.stream), "vcg_norm_finalize")
        L.check(act_fwd(x.data_ptr(), n, c, hw, scale.data_ptr(), shift.data_ptr(), 1 if inst else 0, self.act,
                        float(self.alpha), self._alpha_ptr(), _ptr(residual), y.data_ptr(), rt.stream),
                "%s[%s]" % (self.ACT_FWD, self.name))
        return y, (x, saved, mode, (n, c, hw))

    def backward(self, ctx, dy, param_grads=True, which=0):
        """returns dx; the residual branch's gradient is dy itself (caller handles it)."""
        rt, ps = self.rt, self.ps
        lib = rt.lib
        x, saved, mode, (n, c, hw) = ctx
        dx = self._like(x)
        dalpha = ps.grad(self.prelu_name + "/alpha", which).data_ptr() if (self.act == L.ACT_PRELU and param_grads) else None
        if self.norm is None:
            ws, wsn = rt.workspace(lib.vcg_act_bwd_workspace_bytes(n, c, hw))
            L.check(lib.vcg_act_bwd(x.data_ptr(), dy.data_ptr(), n, c, hw, self.act, float(self.alpha), self._alpha_ptr(),
                                    dx.data_ptr(), dalpha, None, ws, wsn, rt.stream), "vcg_act_bwd[%s]" % self.name)
            return dx
        if saved is None:
            raise RuntimeError("backward through inference-mode normalisation is not defined")
        mean, invstd = saved
        inst = self.norm == "instance"
        gamma = None if inst else ps[self.name + "/gamma"].data_ptr()
        beta = None if inst else ps[self.name + "/beta"].data_ptr()
        dgamma = dbeta = None
        if not inst and param_grads:
            dgamma = ps.grad(self.name + "/gamma", which).data_ptr()
            dbeta = ps.grad(self.name + "/beta", which).data_ptr()
        ws, wsn = rt.workspace(getattr(lib, self.ACT_BWD + "_workspace_bytes")(n, c, hw, mode))
        L.check(getattr(lib, self.ACT_BWD)(x.data_ptr(), dy.data_ptr(), n, c, hw, mode, mean.data_ptr(), invstd.data_ptr(), gamma,
                                           beta, self.act, float(self.alpha), self._alpha_ptr(), 1, dx.data_ptr(), dgamma, dbeta,
                                           dalpha, ws, wsn, rt.stream), "%s[%s]" % (self.ACT_BWD, self.name))
        return dx


class Dense(Layer):
    def __init__(self, name, cin, cout):
        super().__init__(name)
        self.cin, self.cout = cin, cout

    def declare(self, ps):
        ps.declare(self.name + "/kernel", (self.cin, self.cout))
        ps.declare(self.name + "/bias", (self.cout,))

    def init_weights(self, rng):
        return {self.name + "/kernel": glorot_uniform(rng, (self.cin, self.cout), self.cin, self.cout),
                self.name + "/bias": np.zeros((self.cout,), np.float32)}

    def forward(self, x):
        rt = self.rt
        b = x.shape[0]
        y = rt.empty(b, self.cout)
        L.check(rt.lib.vcg_dense_fwd(x.data_ptr(), self.ps[self.name + "/kernel"].data_ptr(),
                                     self.ps[self.name + "/bias"].data_ptr(), y.data_ptr(), b, self.cin, self.cout, rt.stream),
                "vcg_dense_fwd[%s]" % self.name)
        return y, (x,)

    def backward(self, ctx, dy, need_dx=True, param_grads=True, which=0):
        rt = self.rt
        (x,) = ctx
        b = x.shape[0]
        if param_grads:
            L.check(rt.lib.vcg_dense_wgrad(x.data_ptr(), dy.data_ptr(), self.ps.grad(self.name + "/kernel", which).data_ptr(),
                                           self.ps.grad(self.name + "/bias", which).data_ptr(), b, self.cin, self.cout,
                                           rt.stream), "vcg_dense_wgrad[%s]" % self.name)
        dx = None
        if need_dx:
            dx = rt.empty(b, self.cin)
            L.check(rt.lib.vcg_dense_dgrad(dy.data_ptr(), self.ps[self.name + "/kernel"].data_ptr(), dx.data_ptr(), b, self.cin,
                                           self.cout, rt.stream), "vcg_dense_dgrad[%s]" % self.name)
        return dx


# =================================================================================================
# bf16-storage trunk layers (BASELINE.json configs C3/C4: bf16 activations, fp32 master weights / gradients /
# statistics).  Activations are bf16 NHWC torch tensors [n,h,w,64]; parameter names and layouts are those of Conv2D /
# NormAct, so a model built with them exchanges weights with the fp32 one and with the reference.
# =================================================================================================
def to_bf16_nhwc(rt, x_nchw):
    n, c, h, w = x_nchw.shape
    y = torch.empty(n, h, w, c, dtype=torch.bfloat16, device=rt.device)
    L.check(rt.lib.vcg_f32_nchw_to_bf16_nhwc(x_nchw.data_ptr(), y.data_ptr(), n, c, h, w, rt.stream), "vcg_f32_nchw_to_bf16_nhwc")
    return y


def from_bf16_nhwc(rt, x_nhwc):
    n, h, w, c = x_nhwc.shape
    y = rt.empty(n, c, h, w)
    L.check(rt.lib.vcg_bf16_nhwc_to_f32_nchw(x_nhwc.data_ptr(), y.data_ptr(), n, c, h, w, rt.stream), "vcg_bf16_nhwc_to_f32_nchw")
    return y


# ---- a fp32 kernel tensor w as the operand a bf16 kernel reads.  out: the buffer of an earlier call to fill again (a layer's
# PackedOperand); None allocates one (the inference engines of _infer.py, which take fresh buffers at every refresh) ----
def _bf16(rt, *shape):
    return torch.empty(*shape, dtype=torch.bfloat16, device=rt.device)


def _bytes(rt, nbytes):
    return torch.empty(nbytes, dtype=torch.uint8, device=rt.device)


def pack_first9x9_bf16(rt, w, out=None):
    """Conv2D (9,9,3,64) for vcg_conv9x9_from3_bf16_fwd[_train]"""
    out = _bytes(rt, L.FIRST9X9_WFRAG_BYTES) if out is None else out
    L.check(rt.lib.vcg_pack_first9x9_bf16(w.data_ptr(), out.data_ptr(), rt.stream), "vcg_pack_first9x9_bf16")
    return out


def pack_final9x9_bf16(rt, w, out=None):
    """Conv2D (9,9,256,3) for vcg_conv9x9_to3_bf16_fwd"""
    out = _bytes(rt, L.FINAL9X9_WFRAG_BYTES) if out is None else out
    L.check(rt.lib.vcg_pack_final9x9_bf16(w.data_ptr(), out.data_ptr(), rt.stream), "vcg_pack_final9x9_bf16")
    return out


def pack_conv9x9_to3_bf16(rt, w, cin, out=None):
    """Conv2D (9,9,cin,3) for vcg_conv9x9_to3_bf16_fwd on another channel count than 256"""
    out = _bytes(rt, rt.lib.vcg_conv9x9_to3_bf16_wfrag_bytes(cin)) if out is None else out
    L.check(rt.lib.vcg_pack_conv9x9_to3_bf16(w.data_ptr(), cin, out.data_ptr(), rt.stream), "vcg_pack_conv9x9_to3_bf16")
    return out


def pack_conv9x9_c64to3_bf16(rt, w, out=None):
    """Conv2D (9,9,64,3) for vcg_conv9x9_c64to3_bf16_fwd[_window]"""
    out = _bytes(rt, rt.lib.vcg_conv9x9_c64to3_bf16_wfrag_bytes()) if out is None else out
    L.check(rt.lib.vcg_pack_conv9x9_c64to3_bf16(w.data_ptr(), out.data_ptr(), rt.stream), "vcg_pack_conv9x9_c64to3_bf16")
    return out


def pack_conv_kernel_bf16(rt, w, taps, a, b, transpose, flip, out=None):
    """[tap][a][b] bf16 (include/vcg.h: vcg_pack_conv_kernel_bf16), what the 3x3 64-channel kernels read"""
    out = _bf16(rt, taps, a, b) if out is None else out
    L.check(rt.lib.vcg_pack_conv_kernel_bf16(w.data_ptr(), taps, a, b, transpose, flip, out.data_ptr(), rt.stream), "vcg_pack_conv_kernel_bf16")
    return out


def pack_conv_frag_bf16(rt, w, taps, mdim, kdim, mode, out=None):
    """the generic kernels' MFMA fragments; mode 0: a Keras Conv2D kernel for its forward, 1: for its data gradient, 2: that with the taps
    reversed (include/vcg.h: vcg_pack_conv_frag_bf16)"""
    out = _bf16(rt, taps, mdim, kdim) if out is None else out
    L.check(rt.lib.vcg_pack_conv_frag_bf16(w.data_ptr(), taps, mdim, kdim, mode, out.data_ptr(), rt.stream), "vcg_pack_conv_frag_bf16")
    return out


def pack_incep_frag_bf16(rt, w, taps, cin_total, cout, k0=0, kcount=None, out=None):
    """rows [k0, k0 + kcount) of the input-channel axis of a Keras (kh,kw,cin_total,cout) kernel as the generic kernels' fragments, both
    channel axes padded with zeros to multiples of 32 (include/vcg.h: vcg_pack_incep_frag_bf16)"""
    kcount = cin_total if kcount is None else kcount
    out = _bytes(rt, rt.lib.vcg_incep_frag_bf16_bytes(taps, kcount, cout)) if out is None else out
    L.check(rt.lib.vcg_pack_incep_frag_bf16(w.data_ptr(), taps, cin_total, cout, k0, kcount, out.data_ptr(), rt.stream), "vcg_pack_incep_frag_bf16")
    return out


def incep_fold(rt, ps, c, bias=None, norm=None, prelu=None):
    """(scale, shift, alpha) of c channels padded with zeros to a multiple of 32: the bias named `bias`, folded with the inference-mode
    BatchNormalization named `norm`, and the PReLU slopes named `prelu` (each optional; include/vcg.h: vcg_incep_fold)"""
    cp = rt.lib.vcg_incep_padded_channels(c)
    scale, shift, alpha = rt.empty(cp), rt.empty(cp), rt.empty(cp) if prelu else None
    p = lambda name: ps[name].data_ptr() if name else None
    L.check(rt.lib.vcg_incep_fold(p(bias and bias + "/bias"), p(norm and norm + "/moving_mean"), p(norm and norm + "/moving_variance"),
                                  p(norm and norm + "/gamma"), p(norm and norm + "/beta"), p(prelu and prelu + "/alpha"), c, BN_EPS,
                                  scale.data_ptr(), shift.data_ptr(), _ptr(alpha), rt.stream), "vcg_incep_fold")
    return scale, shift, alpha


def pack_conv_frag_bf16_pair(rt, w, taps, cin, cout, out=None):
    """modes 0 and 1 of a Keras (k,k,cin,cout) kernel in one launch -> (forward, data gradient)"""
    wf, wd = (_bf16(rt, taps, cout, cin), _bf16(rt, taps, cin, cout)) if out is None else out
    L.check(rt.lib.vcg_pack_conv_frag_bf16_pair(w.data_ptr(), taps, cin, cout, wf.data_ptr(), wd.data_ptr(), rt.stream), "vcg_pack_conv_frag_bf16_pair")
    return wf, wd


def pack_conv3ch_bf16(rt, w, kh, kw, cout, out=None):
    """Conv2D (kh,kw,3,cout) for vcg_conv3ch_bf16_fwd"""
    out = _bytes(rt, rt.lib.vcg_conv3ch_bf16_wfrag_bytes(kh, kw, cout)) if out is None else out
    L.check(rt.lib.vcg_pack_conv3ch_bf16(w.data_ptr(), kh, kw, cout, out.data_ptr(), rt.stream), "vcg_pack_conv3ch_bf16")
    return out


def pack_conv_in_gate_bf16(rt, w, cin, kh, kw, cout, out=None):
    """Conv2D (kh,kw,cin,cout) for vcg_conv_in_gate_bf16_fwd / _bwd; None where that kernel does not serve the shape"""
    nbytes = rt.lib.vcg_conv_in_gate_bf16_wfrag_bytes(cin, kh, kw, cout)
    if nbytes == 0:
        return None
    out = _bytes(rt, nbytes) if out is None else out
    L.check(rt.lib.vcg_pack_conv_in_gate_bf16(w.data_ptr(), cin, kh, kw, cout, out.data_ptr(), rt.stream), "vcg_pack_conv_in_gate_bf16")
    return out


class TrunkConvBf16(Conv2D):
    """what the generator's 64 -> 64 'same' trunk convolutions on bf16 NHWC share (Conv3x3Bf16, Conv5x5Bf16): the learning-phase-0 forward
    with the normalisation folded in and the data gradient, both on vcg_conv2d_bf16_fwd.  A subclass packs (forward, data gradient)
    operands in _pack(out) and has its own training forward and weight gradient."""

    def __init__(self, name, cin, cout, k):
        if cin != 64 or cout != 64:
            raise NotImplementedError("the bf16 %dx%d trunk convolution is instantiated for 64 -> 64 channels" % (k, k))
        super().__init__(name, cin, cout, k)
        self._pk = PackedOperand(self._pack, self)

    def forward_folded(self, x, norm, residual=None, tag=None, folded=None):
        """learning phase 0: conv + BatchNormalization (moving statistics) [+ PReLU] [+ Add] in ONE launch -- the normalisation is an
        affine map per channel, folded with the bias into the epilogue's scale / shift (vcg_bn_fold); the pre-normalisation tensor is
        never stored.  norm: the NormActBf16 behind this convolution (batch norm).  folded: (scale, shift) already derived (fold_batch)."""
        rt, ps = self.rt, self.ps
        n, h, w, _ = x.shape
        if folded is not None:
            scale, shift = folded
        else:
            scale, shift = rt.empty(64), rt.empty(64)
            L.check(rt.lib.vcg_bn_fold(ps[self.name + "/bias"].data_ptr(), ps[norm.name + "/moving_mean"].data_ptr(),
                                       ps[norm.name + "/moving_variance"].data_ptr(), ps[norm.name + "/gamma"].data_ptr(),
                                       ps[norm.name + "/beta"].data_ptr(), 64, BN_EPS, scale.data_ptr(), shift.data_ptr(), rt.stream), "vcg_bn_fold")
        wf, _ = self._pk.get()
        y = _bf16(rt, n, h, w, 64)
        d = self.desc(n, h, w)
        ep = L.EpilogueBf16(scale.data_ptr(), shift.data_ptr(), norm.act, float(norm.alpha), norm._alpha_ptr(), _ptr(residual), None, L.STATS_NONE)
        with Timed(rt, tag and residual is not None and tag + "_res" or tag):
            L.check(rt.lib.vcg_conv2d_bf16_fwd(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), y.data_ptr(), ctypes.byref(ep), rt.stream),
                    "vcg_conv2d_bf16_fwd[%s]" % self.name)
        return y

    def _dgrad(self, d, dy, dx_residual, tag):
        """dx = the same convolution over dy with the data-gradient pack; dx_residual (a gradient joining at the layer's input) is the
        epilogue's residual operand, added in fp32 before the one rounding to bf16"""
        rt = self.rt
        _, wd = self._pk.get()
        dx = _bf16(rt, d.n, d.h, d.w, 64)
        ep = L.EpilogueBf16(None, None, L.ACT_NONE, 0.0, None, _ptr(dx_residual), None, L.STATS_NONE)
        with Timed(rt, tag and tag + ("_dgrad_res" if dx_residual is not None else "_dgrad")):
            L.check(rt.lib.vcg_conv2d_bf16_fwd(ctypes.byref(d), dy.data_ptr(), wd.data_ptr(), dx.data_ptr(), ctypes.byref(ep), rt.stream),
                    "vcg_conv2d_bf16_fwd[%s dgrad]" % self.name)
        return dx


class Conv3x3Bf16(TrunkConvBf16):
    """Conv2D(64, 3, 'same') on bf16 NHWC: forward and data gradient on vcg_conv2d_bf16_fwd (the latter with the kernel
    packed tap-flipped and transposed), weight / bias gradient on vcg_conv2d_bf16_wgrad (fp32, into the master gradient)."""

    def __init__(self, name, cin=64, cout=64):
        super().__init__(name, cin, cout, 3)

    def _pack(self, out):
        w = self.ps[self.name + "/kernel"]
        wf, wd = out or (None, None)
        return (pack_conv_kernel_bf16(self.rt, w, 9, 64, 64, 1, 0, wf),       # [tap][co][ci]
                pack_conv_kernel_bf16(self.rt, w, 9, 64, 64, 0, 1, wd))       # [tap'][ci][co]

    def _run(self, x, d, tag, stats=None, stats_mode=L.STATS_NONE):
        """y = conv(x) + bias [+ the statistics partials of y]"""
        rt = self.rt
        wf, _ = self._pk.get()
        y = _bf16(rt, d.n, d.h, d.w, 64)
        ep = L.EpilogueBf16(None, self.ps[self.name + "/bias"].data_ptr(), L.ACT_NONE, 0.0, None, None, _ptr(stats), stats_mode)
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv2d_bf16_fwd(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), y.data_ptr(), ctypes.byref(ep), rt.stream),
                    "vcg_conv2d_bf16_fwd[%s]" % self.name)
        return y

    def forward(self, x, tag=None):
        n, h, w, _ = x.shape
        d = self.desc(n, h, w)
        return self._run(x, d, tag), (x, d)

    def forward_stats(self, x, instance, tag=None):
        """forward that also leaves the statistics partials of its output for the normalisation behind it (model.py:20,23,284 in
        training mode): returns (y, ctx, stats) with stats = (records buffer, records per group) or None when the kernel serving
        this shape has no statistics epilogue (the caller then runs the separate statistics pass)"""
        rt = self.rt
        n, h, w, _ = x.shape
        mode = L.STATS_INSTANCE if instance else L.STATS_BATCH
        d = self.desc(n, h, w)
        nrec = rt.lib.vcg_conv2d_bf16_stats_records(ctypes.byref(d), mode)
        if nrec <= 0:
            y, ctx = self.forward(x, tag)
            return y, ctx, None
        buf = rt.empty((n if instance else 1) * nrec * 2 * 64)
        return self._run(x, d, tag, buf, mode), (x, d), (buf, nrec)

    def backward(self, ctx, dy, need_dx=True, param_grads=True, which=0, dx_residual=None, tag=None):
        """dx_residual: a gradient that joins at this layer's input (the block's skip branch), added in the epilogue"""
        rt = self.rt
        x, d = ctx
        if param_grads:
            ws, wsn = rt.workspace(rt.lib.vcg_conv2d_bf16_wgrad_workspace_bytes(ctypes.byref(d)))
            with Timed(rt, tag and tag + "_wgrad"):
                L.check(rt.lib.vcg_conv2d_bf16_wgrad(ctypes.byref(d), x.data_ptr(), dy.data_ptr(), self.ps.grad(self.name + "/kernel", which).data_ptr(),
                                                     self.ps.grad(self.name + "/bias", which).data_ptr(), ws, wsn, rt.stream),
                        "vcg_conv2d_bf16_wgrad[%s]" % self.name)
        return self._dgrad(d, dy, dx_residual, tag) if need_dx else None


class PackGroup3x3:
    """the bf16 operand copies (forward + data-gradient pack) of ALL 3x3 64 -> 64 convolutions of a model, re-derived by one launch
    (vcg_pack_conv3x3_c64_bf16_batch) the first time any of them is needed after a parameter change -- the trunk's 2 x 19 launches of 4.7 us
    per optimizer step otherwise"""

    def __init__(self, layers):
        self.layers = list(layers)
        self.all = PackedOperand(self._pack_all, *self.layers)          # stale as soon as any member is refreshed
        for i, l in enumerate(self.layers):
            # the member's own operand: its slices of the group's buffer, valid once the group is packed
            l.caches.remove(l._pk)
            l._pk = PackedOperand(lambda views, i=i: self._member(i, views), l)

    def _member(self, i, views):
        buf = self.all.get()
        return views or (buf[i, 0], buf[i, 1])

    def _pack_all(self, buf):
        rt = self.layers[0].rt
        n = len(self.layers)
        buf = _bf16(rt, n, 2, 9, 64, 64) if buf is None else buf
        arr = (ctypes.c_void_p * n)(*[l.ps[l.name + "/kernel"].data_ptr() for l in self.layers])
        L.check(rt.lib.vcg_pack_conv3x3_c64_bf16_batch(arr, n, buf.data_ptr(), rt.stream), "vcg_pack_conv3x3_c64_bf16_batch")
        return buf


def fold_batch(rt, pairs):
    """(scale, shift) [len(pairs)][64] of the (Conv3x3Bf16, NormActBf16) pairs of a learning-phase-0 pass: one vcg_bn_fold_batch launch"""
    n = len(pairs)
    out = rt.empty(2, n, 64)
    col = lambda f: (ctypes.c_void_p * n)(*[f(cv, nm) for cv, nm in pairs])
    L.check(rt.lib.vcg_bn_fold_batch(col(lambda cv, nm: cv.ps[cv.name + "/bias"].data_ptr()),
                                     col(lambda cv, nm: cv.ps[nm.name + "/moving_mean"].data_ptr()),
                                     col(lambda cv, nm: cv.ps[nm.name + "/moving_variance"].data_ptr()),
                                     col(lambda cv, nm: cv.ps[nm.name + "/gamma"].data_ptr()),
                                     col(lambda cv, nm: cv.ps[nm.name + "/beta"].data_ptr()), n, 64, BN_EPS, out[0].data_ptr(), out[1].data_ptr(),
                                     rt.stream), "vcg_bn_fold_batch")
    return {id(cv): (out[0, i], out[1, i]) for i, (cv, nm) in enumerate(pairs)}


def conv_nhwc_bf16_fwd(layer, x, tag, instance=None):
    """y = conv(x) + bias on vcg_conv2d_nhwc_bf16_fwd, for a layer whose _pk holds (forward, data gradient) fragments.  instance True /
    False: on vcg_conv2d_nhwc_bf16_fwd_stats, which also leaves the statistics partials of y for the instance / batch normalisation
    behind the layer -- where the tiled kernel serves the shape; where it does not, the plain forward (the caller then runs the separate
    statistics pass).  Returns (y, d, stats) with stats = (records buffer, records per group) or None."""
    rt = layer.rt
    n, h, w, _ = x.shape
    d = layer.desc(n, h, w)
    nrec = 0
    if instance is not None:
        nrec = rt.lib.vcg_conv2d_nhwc_bf16_stats_records(ctypes.byref(d), L.STATS_INSTANCE if instance else L.STATS_BATCH)
    wf, _ = layer._pk.get()
    y = _bf16(rt, n, d.oh, d.ow, layer.cout)
    bias = layer.ps[layer.name + "/bias"].data_ptr()
    if nrec <= 0:
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv2d_nhwc_bf16_fwd(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), bias, L.ACT_NONE, 0.0, y.data_ptr(), rt.stream),
                    "vcg_conv2d_nhwc_bf16_fwd[%s]" % layer.name)
        return y, d, None
    buf = rt.empty((n if instance else 1) * nrec * 2 * layer.cout)
    with Timed(rt, tag):
        L.check(rt.lib.vcg_conv2d_nhwc_bf16_fwd_stats(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), bias, y.data_ptr(), buf.data_ptr(), rt.stream),
                "vcg_conv2d_nhwc_bf16_fwd_stats[%s]" % layer.name)
    return y, d, (buf, nrec)


def conv_nhwc_bf16_wgrad(layer, d, x, dy, which, tag):
    """weight / bias gradient (fp32, into the master gradient) of the convolution d from bf16 NHWC x and dy on vcg_conv2d_nhwc_bf16_wgrad"""
    rt = layer.rt
    ws, wsn = rt.workspace(rt.lib.vcg_conv2d_nhwc_bf16_wgrad_workspace_bytes(ctypes.byref(d)))
    with Timed(rt, tag and tag + "_wgrad"):
        L.check(rt.lib.vcg_conv2d_nhwc_bf16_wgrad(ctypes.byref(d), x.data_ptr(), dy.data_ptr(), layer.ps.grad(layer.name + "/kernel", which).data_ptr(),
                                                  layer.ps.grad(layer.name + "/bias", which).data_ptr(), ws, wsn, rt.stream),
                "vcg_conv2d_nhwc_bf16_wgrad[%s]" % layer.name)


def conv3ch_bf16_wgrad(layer, d, x, dz, which, tag, need=None, entry="vcg_conv3ch_bf16_wgrad", query="vcg_conv3ch_bf16_wgrad_workspace_bytes"):
    """weight / bias gradient of a layer on the 3-channel fp32 NCHW frames x from the bf16 NHWC gradient dz: vcg_conv3ch_bf16_wgrad (frames
    and gradient as bf16 MFMA operands), or at odd widths -- the kernel then asks for no workspace -- the fp32 kernel on an fp32 NCHW copy
    of dz, which is returned (None otherwise).  need: the workspace size where the caller has already asked for it.  entry: the entry point
    and its size query, of the same contract for another input (vcg_conv_in_gate_up_bf16_wgrad: the 6-channel input of the up-sampling gates)."""
    rt = layer.rt
    need = getattr(rt.lib, query)(ctypes.byref(d)) if need is None else need
    if not need:
        dz32 = from_bf16_nhwc(rt, dz)
        layer._wgrad_fp32(d, x, dz32, which, True, tag)
        return dz32
    ws, wsn = rt.workspace(need)
    with Timed(rt, tag and tag + "_wgrad"):
        L.check(getattr(rt.lib, entry)(ctypes.byref(d), x.data_ptr(), dz.data_ptr(), layer.ps.grad(layer.name + "/kernel", which).data_ptr(),
                                       layer.ps.grad(layer.name + "/bias", which).data_ptr(), ws, wsn, rt.stream),
                "%s[%s]" % (entry, layer.name))
    return None


class Conv2DBf16(Conv2D):
    """keras.layers.Conv2D on bf16 NHWC activations, the discriminators' shapes (3x3 / 4x4, stride 1 / 2, channel counts that
    are multiples of 64 -- what the bf16 weight gradient serves): forward and data gradient on vcg_conv2d_nhwc_bf16_* (weights re-laid out as MFMA operand
    fragments after every optimizer step), weight gradient on vcg_conv2d_nhwc_bf16_wgrad; fp32 master weights, gradients and
    bias.  Same parameter names / layouts as Conv2D: a bf16 model exchanges weights with the fp32 one and with the reference."""

    def __init__(self, name, cin, cout, k, stride=1, padding="same", act=L.ACT_NONE, alpha=0.0):
        if act != L.ACT_NONE:
            raise NotImplementedError("Conv2DBf16 carries no fused activation (the layers it serves are followed by a normalisation)")
        if cin % 64 or cout % 64 or k not in (3, 4) or stride not in (1, 2):
            # vcg_conv2d_nhwc_bf16_fwd/_dgrad take more (5x5, stride 3, multiples of 32); the bf16 weight gradient
            # (bf16_gwgrad.hip: gw_plan) serves 3x3 / 4x4, stride 1 / 2, channel multiples of 64 -- a layer is built only if it can train
            raise NotImplementedError("Conv2DBf16 serves 3x3 / 4x4 kernels, stride 1 / 2, channel counts that are multiples of 64")
        super().__init__(name, cin, cout, k, stride, padding, act, alpha)
        self._pk = PackedOperand(lambda out: pack_conv_frag_bf16_pair(self.rt, self.ps[self.name + "/kernel"], k * k, cin, cout, out), self)

    def forward(self, x, residual=None, tag=None):
        y, d, _ = conv_nhwc_bf16_fwd(self, x, tag)
        return y, (x, None, d)

    def forward_stats(self, x, instance, tag=None):
        """forward + per-tile statistics partials of the output (see Conv3x3Bf16.forward_stats)"""
        y, d, stats = conv_nhwc_bf16_fwd(self, x, tag, instance)
        return y, (x, None, d), stats

    def backward(self, ctx, dy, need_dx=True, param_grads=True, which=0, dx_residual=None, tag=None, input_lrelu_slope=None):
        """input_lrelu_slope: the layer's input is the OUTPUT of a LeakyReLU with this slope; dx is then multiplied by its derivative, i.e. it
        is the gradient in front of that activation (the producing layer's backward then needs no activation pass).
        dx_residual: a bf16 NHWC gradient that joins at this layer's input (a residual block's skip branch at conv_pre), added in fp32 before
        the one rounding to bf16 (vcg_conv2d_nhwc_bf16_dgrad_add: 3x3, stride 1)"""
        rt = self.rt
        x, _, d = ctx
        if dx_residual is not None and need_dx:
            if dx_residual.dtype != torch.bfloat16 or tuple(dx_residual.shape) != tuple(x.shape):
                raise TypeError("Conv2DBf16[%s]: dx_residual must be a bf16 NHWC tensor of the input's shape" % self.name)
            if self.k != 3 or self.stride != 1 or input_lrelu_slope is not None:
                raise NotImplementedError("Conv2DBf16[%s]: a joining gradient is served for 3x3 stride-1 layers without an input mask" % self.name)
        if param_grads:
            conv_nhwc_bf16_wgrad(self, d, x, dy, which, tag)
        if not need_dx:
            return None
        _, wd = self._pk.get()
        dx = torch.empty_like(x)
        if dx_residual is not None:
            with Timed(rt, tag and tag + "_dgrad_res"):
                L.check(rt.lib.vcg_conv2d_nhwc_bf16_dgrad_add(ctypes.byref(d), dy.data_ptr(), wd.data_ptr(), dx_residual.data_ptr(), dx.data_ptr(),
                                                              rt.stream), "vcg_conv2d_nhwc_bf16_dgrad_add[%s]" % self.name)
            return dx
        with Timed(rt, tag and tag + "_dgrad"):
            L.check(rt.lib.vcg_conv2d_nhwc_bf16_dgrad(ctypes.byref(d), dy.data_ptr(), wd.data_ptr(),
                                                      x.data_ptr() if input_lrelu_slope is not None else None, float(input_lrelu_slope or 0.0),
                                                      dx.data_ptr(), rt.stream), "vcg_conv2d_nhwc_bf16_dgrad[%s]" % self.name)
        return dx


class Conv5x5Bf16(TrunkConvBf16):
    """Conv2D(64, 5, 'same') on bf16 NHWC, 64 -> 64: the trunk convolution of the reference's default generator (kernel_size=5,
    model.py:267) with the interface UpscalerOrig uses on Conv3x3Bf16.  Training forward on vcg_conv2d_nhwc_bf16_fwd[_stats] (the
    statistics partials of the normalisation behind it out of the epilogue), learning phase 0 on vcg_conv2d_bf16_fwd's 5x5 form with the
    folded BatchNormalization / PReLU / Add epilogue (the launch _infer.py makes).  The data gradient is that same entry point on the
    kernel packed tap-reversed and transposed (vcg_pack_conv_frag_bf16 mode 2); a gradient joining at the layer's input (dx_residual) is its
    residual operand, added in fp32 before the one rounding to bf16.  Weight / bias gradient on vcg_conv2d_nhwc_bf16_wgrad (5x5: two
    tap groups per block pair)."""

    def __init__(self, name, cin=64, cout=64):
        super().__init__(name, cin, cout, 5)

    def _pack(self, out):
        w = self.ps[self.name + "/kernel"]
        wf, wd = out or (None, None)
        return pack_conv_frag_bf16(self.rt, w, 25, 64, 64, 0, wf), pack_conv_frag_bf16(self.rt, w, 25, 64, 64, 2, wd)

    def forward(self, x, tag=None):
        y, d, _ = conv_nhwc_bf16_fwd(self, x, tag)
        return y, (x, d)

    def forward_stats(self, x, instance, tag=None):
        """forward + per-tile statistics partials of the output (see Conv3x3Bf16.forward_stats); None where the tiled kernel does not
        serve the shape (the caller then runs the separate statistics pass)"""
        y, d, stats = conv_nhwc_bf16_fwd(self, x, tag, instance)
        return y, (x, d), stats

    def backward(self, ctx, dy, need_dx=True, param_grads=True, which=0, dx_residual=None, tag=None):
        """dx_residual: a gradient that joins at this layer's input (the block's skip branch), added in the epilogue"""
        x, d = ctx
        if param_grads:
            conv_nhwc_bf16_wgrad(self, d, x, dy, which, tag)
        return self._dgrad(d, dy, dx_residual, tag) if need_dx else None


class InitialConv9x9Bf16(Conv2D):
    """initial/conv + initial/prelu (model.py:275-276) as the entry into the bf16 layout: Conv2D(64, 9, 'same') + bias + PReLU from the
    fp32 NCHW frames to bf16 NHWC in one launch (vcg_conv9x9_from3_bf16_fwd[_train]: bf16 copies of frames and kernel as MFMA operands,
    fp32 accumulation).  In training the value in front of the PReLU is stored too; backward adds the gradients meeting at the output
    (trunk + long skip, both bf16 NHWC), applies the activation's derivative and the slope gradient in one pass
    (vcg_prelu_bwd_nhwc_bf16_to_bf16) whose bf16 NHWC result feeds the bf16 weight-gradient kernel of the 3-channel layers (vcg_conv3ch_bf16_wgrad).  Declares the
    Conv2D's parameters; the PReLU slope belongs to the NormAct layer behind it (same names as the fp32 model)."""

    def __init__(self, name, cin, cout, k):
        if cin != 3 or cout != 64 or k != 9:
            raise NotImplementedError("the bf16 initial convolution is instantiated for 9x9, 3 -> 64 channels")
        super().__init__(name, cin, cout, k)
        self._pk = PackedOperand(lambda out: pack_first9x9_bf16(self.rt, self.ps[self.name + "/kernel"], out), self)

    def forward_prelu(self, x, alpha, training, tag=None):
        """x fp32 NCHW frames, alpha: the PReLU slopes [64] -> (y bf16 NHWC, ctx)"""
        rt = self.rt
        n, _, h, w = x.shape
        d = self.desc(n, h, w)
        wf = self._pk.get()
        y = torch.empty(n, h, w, self.cout, dtype=torch.bfloat16, device=rt.device)
        bias = self.ps[self.name + "/bias"].data_ptr()
        with Timed(rt, tag):
            if training:
                z = torch.empty_like(y)
                L.check(rt.lib.vcg_conv9x9_from3_bf16_fwd_train(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), bias, alpha.data_ptr(), y.data_ptr(),
                                                                z.data_ptr(), rt.stream), "vcg_conv9x9_from3_bf16_fwd_train")
            else:
                z = None
                L.check(rt.lib.vcg_conv9x9_from3_bf16_fwd(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), bias, alpha.data_ptr(), y.data_ptr(), rt.stream),
                        "vcg_conv9x9_from3_bf16_fwd")
        return y, (x, z, d)

    def backward_prelu(self, ctx, d1, d2, alpha, dalpha, which=0, tag=None):
        """d1 (+ d2 or None): bf16 NHWC gradients at the PReLU's output; writes the kernel / bias gradients and dalpha [64]"""
        rt, lib = self.rt, self.rt.lib
        x, z, d = ctx
        if z is None:
            raise RuntimeError("backward through an inference-mode forward")
        hw = d.h * d.w
        nrec = lib.vcg_prelu_bwd_nhwc_bf16_records(d.n, hw)
        L.check(min(nrec, 0), "vcg_prelu_bwd_nhwc_bf16_records")
        rec = rt.empty(nrec * self.cout)
        need = lib.vcg_conv3ch_bf16_wgrad_workspace_bytes(ctypes.byref(d))
        if need:
            # dz stays bf16 NHWC: the weight gradient multiplies it as an MFMA operand (vcg_conv3ch_bf16_wgrad)
            dz = torch.empty(d.n, d.h, d.w, self.cout, dtype=torch.bfloat16, device=rt.device)
            L.check(lib.vcg_prelu_bwd_nhwc_bf16_to_bf16(d1.data_ptr(), _ptr(d2), z.data_ptr(), alpha.data_ptr(), d.n, self.cout, hw, dz.data_ptr(),
                                                        rec.data_ptr(), rt.stream), "vcg_prelu_bwd_nhwc_bf16_to_bf16")
            L.check(lib.vcg_sum_records(rec.data_ptr(), nrec, self.cout, 1.0, dalpha.data_ptr(), rt.stream), "vcg_sum_records[%s]" % self.name)
            conv3ch_bf16_wgrad(self, d, x, dz, which, tag, need)
            return
        # odd widths: the fp32 weight-gradient kernel on the fp32 NCHW form of dz
        dz = rt.empty(d.n, self.cout, d.h, d.w)
        L.check(lib.vcg_prelu_bwd_nhwc_bf16(d1.data_ptr(), _ptr(d2), z.data_ptr(), alpha.data_ptr(), d.n, self.cout, hw, dz.data_ptr(),
                                            rec.data_ptr(), rt.stream), "vcg_prelu_bwd_nhwc_bf16")
        L.check(lib.vcg_sum_records(rec.data_ptr(), nrec, self.cout, 1.0, dalpha.data_ptr(), rt.stream), "vcg_sum_records[%s]" % self.name)
        self._wgrad_fp32(d, x, dz, which, True, tag)


class FirstConvBf16(Conv2D):
    """A critic's first layer -- Conv2D on the 3-channel fp32 NCHW frames -- writing bf16 NHWC directly (vcg_conv3ch_bf16_fwd: bf16 copies of
    frames and kernel as MFMA operands, fp32 accumulation, + bias [+ LeakyReLU]): simple_512 / thin_512 block 1 (3x3 'same', model.py:839;
    its BatchNormalization follows on bf16) and the PatchGAN's 4x4 stride-2 layer + LeakyReLU(0.2).  backward takes the bf16 NHWC gradient
    IN FRONT of the activation (the next layer's data gradient applies the LeakyReLU mask: Conv2DBf16.backward(mask=...)); weight gradient on
    vcg_conv3ch_bf16_wgrad (frames and gradient as bf16 MFMA operands), data gradient on vcg_conv3ch_bf16_dgrad."""

    def __init__(self, name, cin, cout, k, stride=1, padding="same", act=L.ACT_NONE, alpha=0.0):
        if cin != 3 or cout % 64 or cout > 512 or (k, stride) not in ((3, 1), (4, 2)) or act not in (L.ACT_NONE, L.ACT_LRELU):
            raise NotImplementedError("FirstConvBf16 serves Conv2D(64m, 3, strides 1) / Conv2D(64m, 4, strides 2) on 3 input channels")
        super().__init__(name, cin, cout, k, stride, padding, act, alpha)
        # next to Conv2D's _wt, which only the fp32 data-gradient fallback of backward asks for
        self._pk = PackedOperand(lambda out: pack_conv3ch_bf16(self.rt, self.ps[self.name + "/kernel"], k, k, cout, out), self)

    def forward(self, x, residual=None, tag=None):
        rt = self.rt
        n, _, h, w = x.shape
        d = self.desc(n, h, w)
        wf = self._pk.get()
        y = torch.empty(n, d.oh, d.ow, self.cout, dtype=torch.bfloat16, device=rt.device)
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv3ch_bf16_fwd(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), self.ps[self.name + "/bias"].data_ptr(),
                                                float(self.alpha) if self.act == L.ACT_LRELU else 1.0, y.data_ptr(), rt.stream),
                    "vcg_conv3ch_bf16_fwd[%s]" % self.name)
        return y, (x, y, d)

    def backward(self, ctx, dz, need_dx=True, param_grads=True, which=0, dx_residual=None, tag=None):
        """dz: bf16 NHWC gradient in front of the activation"""
        rt = self.rt
        x, _, d = ctx
        dz32 = conv3ch_bf16_wgrad(self, d, x, dz, which, tag) if param_grads else None
        if not need_dx:
            return None
        dx = rt.empty(d.n, self.cin, d.h, d.w)
        need = rt.lib.vcg_conv3ch_bf16_dgrad_workspace_bytes(ctypes.byref(d))
        ws, wsn = rt.workspace(need)
        with Timed(rt, tag and tag + "_dgrad"):
            rc = rt.lib.vcg_conv3ch_bf16_dgrad(ctypes.byref(d), dz.data_ptr(), self.ps[self.name + "/kernel"].data_ptr(), dx.data_ptr(), ws, wsn, rt.stream)
            if rc == L.E_UNSUPPORTED:       # other pads / channel counts: the fp32 data-gradient kernel on the fp32 copy of dz
                dz32 = from_bf16_nhwc(rt, dz) if dz32 is None else dz32
                rc = rt.lib.vcg_conv2d_dgrad(ctypes.byref(d), dz32.data_ptr(), self.ps[self.name + "/kernel"].data_ptr(), self._wt.get().data_ptr(),
                                             dx.data_ptr(), None, rt.stream)
            L.check(rc, "vcg_conv3ch_bf16_dgrad[%s]" % self.name)
        return dx


class FrozenConvReluBf16(Conv2D):
    """Conv2D(f, 3, 'same') + ReLU of a FROZEN network on bf16 NHWC activations -- fifteen of the sixteen layers of the VGG19 feature
    extractor behind the perceptual losses (model.py:101-157): forward on vcg_conv2d_nhwc_bf16_fwd with the ReLU in its epilogue
    (VCG_ACT_LRELU, slope 0), data gradient on vcg_conv2d_nhwc_bf16_dgrad, which also applies the ReLU derivative of the layer that FEEDS this
    one (mask = this layer's input).  No weight gradient exists, so none is asked for: backward is the data gradient only.  The fragments
    are packed when the weights are set (refresh), never inside a step: a recorded train step holds no pack launch of a frozen layer.
    Conv2D's parameter names and layouts: the model exchanges weights with the fp32 one."""

    def __init__(self, name, cin, cout):
        if cin % 32 or cout % 32:
            raise NotImplementedError("FrozenConvReluBf16 serves 3x3 stride-1 'same' layers on channel counts that are multiples of 32")
        super().__init__(name, cin, cout, 3, act=L.ACT_LRELU, alpha=0.0)
        self._pk = PackedOperand(lambda out: pack_conv_frag_bf16_pair(self.rt, self.ps[self.name + "/kernel"], 9, cin, cout, out), self)

    def refresh(self):
        super().refresh()
        if self.rt is not None:
            self._pk.get()

    def forward(self, x, tag=None):
        """x bf16 NHWC -> relu(conv(x) + bias) bf16 NHWC"""
        rt = self.rt
        n, h, w, _ = x.shape
        d = self.desc(n, h, w)
        wf, _ = self._pk.get()
        y = _bf16(rt, n, h, w, self.cout)
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv2d_nhwc_bf16_fwd(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), self.ps[self.name + "/bias"].data_ptr(), L.ACT_LRELU, 0.0,
                                                    y.data_ptr(), rt.stream), "vcg_conv2d_nhwc_bf16_fwd[%s]" % self.name)
        return y

    def backward_data(self, dz, relu_input=None, tag=None):
        """dz: bf16 NHWC gradient in front of this layer's ReLU.  relu_input: the layer's input where that is the ReLU output of another
        convolution -- the result is then the gradient in front of THAT ReLU; None where the input is a pooled tensor."""
        rt = self.rt
        n, h, w, _ = dz.shape
        d = self.desc(n, h, w)
        _, wd = self._pk.get()
        dx = _bf16(rt, n, h, w, self.cin)
        with Timed(rt, tag and tag + "_dgrad"):
            L.check(rt.lib.vcg_conv2d_nhwc_bf16_dgrad(ctypes.byref(d), dz.data_ptr(), wd.data_ptr(), _ptr(relu_input), 0.0, dx.data_ptr(), rt.stream),
                    "vcg_conv2d_nhwc_bf16_dgrad[%s]" % self.name)
        return dx


class FrozenFirstConvReluBf16(Conv2D):
    """block1_conv1 of that extractor: Conv2D(64, 3, 'same') + ReLU from the fp32 NCHW frames to bf16 NHWC on vcg_conv3ch_bf16_fwd
    (lrelu_slope 0), data gradient from the bf16 NHWC gradient in front of the ReLU to the fp32 NCHW frames on vcg_conv3ch_bf16_dgrad.
    Frozen like FrozenConvReluBf16: packed at refresh, no weight gradient."""

    def __init__(self, name, cin, cout):
        if cin != 3 or cout != 64:
            raise NotImplementedError("FrozenFirstConvReluBf16 serves Conv2D(64, 3) on 3 input channels")
        super().__init__(name, cin, cout, 3, act=L.ACT_LRELU, alpha=0.0)
        self._pk = PackedOperand(lambda out: pack_conv3ch_bf16(self.rt, self.ps[self.name + "/kernel"], 3, 3, cout, out), self)

    def refresh(self):
        super().refresh()
        if self.rt is not None:
            self._pk.get()

    def forward(self, x, tag=None):
        rt = self.rt
        n, _, h, w = x.shape
        d = self.desc(n, h, w)
        y = _bf16(rt, n, h, w, self.cout)
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv3ch_bf16_fwd(ctypes.byref(d), x.data_ptr(), self._pk.get().data_ptr(), self.ps[self.name + "/bias"].data_ptr(), 0.0,
                                                y.data_ptr(), rt.stream), "vcg_conv3ch_bf16_fwd[%s]" % self.name)
        return y

    def backward_data(self, dz, tag=None):
        rt = self.rt
        n, h, w, _ = dz.shape
        d = self.desc(n, h, w)
        dx = rt.empty(n, self.cin, h, w)
        ws, wsn = rt.workspace(rt.lib.vcg_conv3ch_bf16_dgrad_workspace_bytes(ctypes.byref(d)))
        with Timed(rt, tag and tag + "_dgrad"):
            L.check(rt.lib.vcg_conv3ch_bf16_dgrad(ctypes.byref(d), dz.data_ptr(), self.ps[self.name + "/kernel"].data_ptr(), dx.data_ptr(), ws, wsn,
                                                  rt.stream), "vcg_conv3ch_bf16_dgrad[%s]" % self.name)
        return dx


class ConvCout1Bf16(Conv2D):
    """Conv2D(1, k) on bf16 NHWC activations -- the 70x70 PatchGAN's last layer (512 -> 1, 4x4, zero padding 1) in the bf16 configs:
    forward, data gradient and weight gradient on vcg_conv2d_cout1_nhwc_bf16_* straight from / to the bf16 NHWC tensor (fp32
    weights, fp32 accumulation, fp32 [n,1,oh,ow] output).  Same parameter names / layouts as Conv2D."""

    def __init__(self, name, cin, cout, k, stride=1, padding="same", act=L.ACT_NONE, alpha=0.0):
        if cout != 1 or stride != 1 or act != L.ACT_NONE or k not in (3, 4) or cin % 8 or cin > 512:
            raise NotImplementedError("ConvCout1Bf16 serves Conv2D(1, 3|4, stride 1) on up to 512 channels (multiples of 8), no activation")
        super().__init__(name, cin, cout, k, stride, padding, act, alpha)

    def forward(self, x, residual=None, tag=None):
        rt = self.rt
        n, h, w, _ = x.shape
        d = self.desc(n, h, w)
        y = rt.empty(n, 1, d.oh, d.ow)
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv2d_cout1_nhwc_bf16_fwd(ctypes.byref(d), x.data_ptr(), self.ps[self.name + "/kernel"].data_ptr(),
                                                          self.ps[self.name + "/bias"].data_ptr(), y.data_ptr(), rt.stream),
                    "vcg_conv2d_cout1_nhwc_bf16_fwd[%s]" % self.name)
        return y, (x, None, d)

    def backward(self, ctx, dy, need_dx=True, param_grads=True, which=0, dx_residual=None, tag=None):
        rt = self.rt
        x, _, d = ctx
        if param_grads:
            ws, wsn = rt.workspace(rt.lib.vcg_conv2d_cout1_nhwc_bf16_wgrad_workspace_bytes(ctypes.byref(d)))
            with Timed(rt, tag and tag + "_wgrad"):
                L.check(rt.lib.vcg_conv2d_cout1_nhwc_bf16_wgrad(ctypes.byref(d), x.data_ptr(), dy.data_ptr(),
                                                                self.ps.grad(self.name + "/kernel", which).data_ptr(),
                                                                self.ps.grad(self.name + "/bias", which).data_ptr(), ws, wsn, rt.stream),
                        "vcg_conv2d_cout1_nhwc_bf16_wgrad[%s]" % self.name)
        if not need_dx:
            return None
        dx = torch.empty_like(x)
        with Timed(rt, tag and tag + "_dgrad"):
            L.check(rt.lib.vcg_conv2d_cout1_nhwc_bf16_dgrad(ctypes.byref(d), dy.data_ptr(), self.ps[self.name + "/kernel"].data_ptr(),
                                                            dx.data_ptr(), rt.stream), "vcg_conv2d_cout1_nhwc_bf16_dgrad[%s]" % self.name)
        return dx


def bf16_to_f32(rt, x):
    """flat precision change, shape kept (Flatten of NHWC is its memory order)"""
    y = rt.empty(*x.shape)
    L.check(rt.lib.vcg_bf16_to_f32(x.data_ptr(), y.data_ptr(), x.numel(), rt.stream), "vcg_bf16_to_f32")
    return y


def f32_to_bf16(rt, x):
    y = torch.empty(*x.shape, dtype=torch.bfloat16, device=rt.device)
    L.check(rt.lib.vcg_f32_to_bf16(x.data_ptr(), y.data_ptr(), x.numel(), rt.stream), "vcg_f32_to_bf16")
    return y


class ConvTBf16(ConvT2D):
    """upsampling_block (model.py:70-75) on bf16 NHWC: Conv2DTranspose(k, strides 2) + bias + LeakyReLU for k in {3, 5}, 64 or 256 input
    channels (the first and the later stages of an x4 generator) and k = 3 on 128 (256 -> 128 -> 64 of make_generator_cyclegan, whose
    stages have no activation of their own), out-channels a multiple of 64.  Forward on
    vcg_conv_transpose2d_nhwc_bf16_fwd.  Backward takes the gradient dz in front of the layer's own activation (the bf16 data gradient of
    final/conv applies the LeakyReLU derivative itself): weight gradient on vcg_conv_transpose2d_nhwc_bf16_wgrad, bias gradient =
    per-channel sum of dz (from the producer's records, or vcg_norm_stats_bf16's shifted sums), data gradient = the stride-2 convolution
    of dz with the kernel read as (in = out-channels, out = in-channels) on vcg_conv2d_nhwc_bf16_fwd."""

    def __init__(self, name, cin, cout, k, act=L.ACT_NONE, alpha=0.0):
        if k not in (3, 5) or (cin not in (64, 256) and (cin, k) != (128, 3)) or cout % 64 or cout <= 0 or act not in (L.ACT_NONE, L.ACT_LRELU):
            raise NotImplementedError("the generic bf16 transposed convolution serves 3x3 / 5x5 on 64 or 256 and 3x3 on 128 input channels, -> 64m "
                                      "channels, no activation or LeakyReLU")
        super().__init__(name, cin, cout, k, act, alpha)
        self._pk = PackedOperand(self._pack, self)

    def _pack(self, out):
        # Keras' (kh,kw,out,in) kernel is the Conv2D kernel (kh,kw,in'=out,out'=in) of the stride-2 convolution dz -> dx: the forward
        # is that convolution's data gradient (mode 1), the layer's data gradient its forward (mode 0)
        w = self.ps[self.name + "/kernel"]
        wp, wg = out or (None, None)
        return self._pack_fwd(w, wp), pack_conv_frag_bf16(self.rt, w, self.k * self.k, self.cin, self.cout, 0, wg)

    def _pack_fwd(self, w, out):
        return pack_conv_frag_bf16(self.rt, w, self.k * self.k, self.cout, self.cin, 1, out)

    def forward(self, x, tag=None):
        rt = self.rt
        n, h, w, _ = x.shape
        wp, _ = self._pk.get()
        y = torch.empty(n, 2 * h, 2 * w, self.cout, dtype=torch.bfloat16, device=rt.device)
        d = self.desc(n, h, w)
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv_transpose2d_nhwc_bf16_fwd(ctypes.byref(d), x.data_ptr(), wp.data_ptr(), self.ps[self.name + "/bias"].data_ptr(),
                                                              self.act, float(self.alpha), y.data_ptr(), rt.stream),
                    "vcg_conv_transpose2d_nhwc_bf16_fwd[%s]" % self.name)
        return y, (x, y, d)

    def backward(self, ctx, dz, need_dx=True, param_grads=True, which=0, tag=None, dz_channel_sums=None, input_lrelu_slope=None):
        """dz: bf16 NHWC gradient in front of the LeakyReLU.  Returns dx as bf16 NHWC.  dz_channel_sums: (records, count) left by the kernel
        that produced dz (FinalConv9x9Bf16.backward).  input_lrelu_slope: the layer's input is the OUTPUT of a LeakyReLU with this slope
        (the up-sampling stage below); dx is then multiplied by its derivative (vcg_lrelu_bwd_bf16), i.e. it is that stage's dz."""
        rt, lib = self.rt, self.rt.lib
        x, _, d = ctx
        _, wg = self._pk.get()
        if param_grads:
            ws, wsn = rt.workspace(lib.vcg_conv_transpose2d_nhwc_bf16_wgrad_workspace_bytes(ctypes.byref(d)))
            with Timed(rt, tag and tag + "_wgrad"):
                L.check(lib.vcg_conv_transpose2d_nhwc_bf16_wgrad(ctypes.byref(d), x.data_ptr(), dz.data_ptr(),
                                                                 self.ps.grad(self.name + "/kernel", which).data_ptr(), ws, wsn, rt.stream),
                        "vcg_conv_transpose2d_nhwc_bf16_wgrad[%s]" % self.name)
            gb = self.ps.grad(self.name + "/bias", which)
            if dz_channel_sums is not None:
                rec, nrec = dz_channel_sums
                L.check(lib.vcg_sum_records(rec.data_ptr(), nrec, self.cout, 1.0, gb.data_ptr(), rt.stream), "vcg_sum_records[%s]" % self.name)
            else:
                # sum of dz over (n, h, w) = its per-channel mean x count (the shifted sums of vcg_norm_stats_bf16)
                hw = d.oh * d.ow
                mean, var = rt.empty(self.cout), rt.empty(self.cout)
                ws, wsn = rt.workspace(lib.vcg_norm_stats_bf16_workspace_bytes(d.n, self.cout, hw, L.NORM_BATCH))
                L.check(lib.vcg_norm_stats_bf16(dz.data_ptr(), d.n, self.cout, hw, L.NORM_BATCH, mean.data_ptr(), var.data_ptr(), ws, wsn, rt.stream),
                        "vcg_norm_stats_bf16[%s]" % self.name)
                axpby(rt, mean, gb, float(d.n * hw), 0.0)
        if not need_dx:
            return None
        # dx[ci][i] = sum dz[co][2i + k - crop] W[k][co][ci]: a stride-2 convolution over dz (pad = the crop)
        dd = L.ConvDesc(d.n, self.cout, d.oh, d.ow, self.cin, d.h, d.w, self.k, self.k, 2, d.pad_top, d.pad_left)
        dx = torch.empty_like(x)
        with Timed(rt, tag and tag + "_dgrad"):
            L.check(lib.vcg_conv2d_nhwc_bf16_fwd(ctypes.byref(dd), dz.data_ptr(), wg.data_ptr(), None, L.ACT_NONE, 0.0, dx.data_ptr(), rt.stream),
                    "vcg_conv2d_nhwc_bf16_fwd[%s dgrad]" % self.name)
            if input_lrelu_slope is not None:
                L.check(lib.vcg_lrelu_bwd_bf16(dx.data_ptr(), x.data_ptr(), float(input_lrelu_slope), dx.data_ptr(), dx.numel(), rt.stream),
                        "vcg_lrelu_bwd_bf16[%s]" % self.name)
        return dx


class ConvT3x3Bf16(ConvTBf16):
    """The up-sampling stage of the k3 x2 topology, Conv2DTranspose(3, strides 2) 64 -> 64m + bias + LeakyReLU: a ConvTBf16 whose forward
    runs on the kernel built for this shape, vcg_conv_transpose2d_bf16_fwd, reading the kernel as [tap][out][in] bf16."""

    def __init__(self, name, cin, cout, k, act=L.ACT_NONE, alpha=0.0):
        if k != 3 or cin != 64 or cout % 64:
            raise NotImplementedError("the bf16 transposed convolution is instantiated for 3x3, 64 -> 64m channels")
        super().__init__(name, cin, cout, k, act, alpha)

    def _pack_fwd(self, w, out):
        return pack_conv_kernel_bf16(self.rt, w, 9, self.cout, self.cin, 0, 0, out)

    def forward(self, x, tag=None):
        rt = self.rt
        n, h, w, _ = x.shape
        wp, _ = self._pk.get()
        y = _bf16(rt, n, 2 * h, 2 * w, self.cout)
        d = self.desc(n, h, w)
        ep = L.EpilogueBf16(None, self.ps[self.name + "/bias"].data_ptr(), self.act, float(self.alpha), None, None)
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv_transpose2d_bf16_fwd(ctypes.byref(d), x.data_ptr(), wp.data_ptr(), y.data_ptr(), ctypes.byref(ep), rt.stream),
                    "vcg_conv_transpose2d_bf16_fwd[%s]" % self.name)
        return y, (x, y, d)


class UpConvTBf16(ConvTBf16):
    """conv_transp of upsampling_block_attention (model.py:91-92) on bf16 NHWC: Conv2DTranspose(128, k, strides 2) + bias + LeakyReLU(0.2)
    on the 64 (first block) or 128 (second block) gated channels, k 3 or 5 -- ConvTBf16's kernels at shapes of its own.  The Add of
    to_add_input follows (ToAddInputBf16): its backward hands this layer dz, the gradient in front of the LeakyReLU, and the channel sums
    of dz, so backward is ConvTBf16's with dz_channel_sums."""

    def __init__(self, name, cin, cout, k, act=L.ACT_LRELU, alpha=0.2):
        if k not in (3, 5) or cin not in (64, 128) or cout != 128 or act != L.ACT_LRELU:
            raise NotImplementedError("the bf16 transposed convolution of the attention generator's up-sampling blocks serves 3x3 / 5x5, 64 or 128 "
                                      "-> 128 channels with LeakyReLU")
        ConvT2D.__init__(self, name, cin, cout, k, act, alpha)
        self._pk = PackedOperand(self._pack, self)


class ToAddInputBf16(ConvT2D):
    """to_add_input and add_input of upsampling_block_attention (model.py:94-97) on the bf16 path: y = bf16(y_act + bias +
    Conv2DTranspose(cout, s+1, strides s, 'same')(atanh(0.99999 frames))) with the atanh, the transposed convolution on three channels and
    the Add in one launch (vcg_input_convt_add_bf16_to; in learning phase 0 in place on y_act, vcg_input_convt_add_bf16).  Owns
    to_add_input_conv_transp/kernel (s+1,s+1,cout,3) and /bias under the fp32 model's names, used as fp32.  backward
    (vcg_input_convt_add_bf16_bwd) reads the gradient dY at the block's output once and returns dz -- the gradient in front of the
    LeakyReLU that produced y_act -- with its channel sums (the transposed convolution's bias gradient) for UpConvTBf16.backward, and
    leaves this layer's own weight and bias gradient.  The frames are the network input: no gradient goes to them."""

    def __init__(self, name, cin, cout, stride, slope=0.2):
        if cin != 3 or stride not in (2, 4) or cout % 8 or stride * stride * cout // 8 > 256:
            raise NotImplementedError("the bf16 to_add_input is instantiated for 3 input channels, strides 2 or 4 (kernel strides + 1) and "
                                      "8m channels, strides^2 m <= 256")
        super().__init__(name, cin, cout, stride + 1, L.ACT_NONE, 0.0)
        self.stride, self.slope = stride, slope

    def desc(self, n, h, w):
        s = self.stride
        return L.ConvDesc(n, 3, h, w, self.cout, s * h, s * w, s + 1, s + 1, s, 0, 0)

    def forward(self, x, y_act, training=True, tag=None):
        """x: the fp32 NCHW frames [n,3,h,w]; y_act: bf16 NHWC [n,s h,s w,cout], kept (training) or overwritten with the sum"""
        rt = self.rt
        n, c, h, w = x.shape
        d = self.desc(n, h, w)
        if c != 3 or y_act.dtype != torch.bfloat16 or tuple(y_act.shape) != (n, d.oh, d.ow, self.cout):
            raise TypeError("ToAddInputBf16[%s]: x fp32 NCHW frames [n,3,h,w], y_act bf16 NHWC [n,%dh,%dw,%d]" % (self.name, self.stride, self.stride, self.cout))
        y = torch.empty_like(y_act) if training else y_act
        with Timed(rt, tag):
            L.check(rt.lib.vcg_input_convt_add_bf16_to(ctypes.byref(d), x.data_ptr(), self.ps[self.name + "/kernel"].data_ptr(),
                                                       self.ps[self.name + "/bias"].data_ptr(), y_act.data_ptr(), y.data_ptr(), rt.stream),
                    "vcg_input_convt_add_bf16_to[%s]" % self.name)
        return y, (x, y_act if training else None, d)

    def backward(self, ctx, dy, which=0, tag=None):
        """dy: bf16 NHWC gradient at the block's output.  Returns (dz, (channel sums of dz, 1)): UpConvTBf16.backward's dz and dz_channel_sums"""
        rt = self.rt
        x, y_act, d = ctx
        if y_act is None:
            raise RuntimeError("ToAddInputBf16[%s]: the forward pass ran in learning phase 0 and kept no activation" % self.name)
        if dy.dtype != torch.bfloat16 or tuple(dy.shape) != tuple(y_act.shape):
            raise TypeError("ToAddInputBf16[%s]: the gradient is a bf16 NHWC tensor of the output's shape" % self.name)
        dz, sums = torch.empty_like(dy), rt.empty(self.cout)
        ws, wsn = rt.workspace(rt.lib.vcg_input_convt_add_bf16_bwd_ws_bytes(ctypes.byref(d)))
        with Timed(rt, tag and tag + "_bwd"):
            L.check(rt.lib.vcg_input_convt_add_bf16_bwd(ctypes.byref(d), x.data_ptr(), dy.data_ptr(), y_act.data_ptr(), float(self.slope), dz.data_ptr(),
                                                        self.ps.grad(self.name + "/kernel", which).data_ptr(),
                                                        self.ps.grad(self.name + "/bias", which).data_ptr(), sums.data_ptr(), ws, wsn, rt.stream),
                    "vcg_input_convt_add_bf16_bwd[%s]" % self.name)
        return dz, (sums, 1)


class Conv9x9To3Bf16(Conv2D):
    """Conv2D(3, 9, 'same') + tanh on a bf16 NHWC input with CIN channels, fp32 NCHW output: final/conv (model.py:290-291) on 256 channels
    and head/conv of make_generator_cyclegan on 64.  Forward on the entry point FWD over the operand PACK_FWD lays out; data gradient on
    vcg_conv9x9_to3_bf16_dgrad with the kernel packed by vcg_pack_conv9x9_3ch_bf16(w, CIN, 1) into DGRAD_PACK_BYTES (the 3 -> 64 kernel of
    the first layer with the roles swapped, once per 64 channels); weight gradient on vcg_conv9x9_to3_bf16_wgrad (even widths; odd ones take
    the fp32 kernel on an fp32 NCHW copy of the input).  INPUT_ACT: whether backward serves input_lrelu_slope and want_channel_sums."""
    CIN = FWD = PACK_FWD = DGRAD_PACK_BYTES = REFUSAL = DGRAD_LABEL = INPUT_ACT = None
    WGRAD, WGRAD_QUERY = "vcg_conv9x9_to3_bf16_wgrad", "vcg_conv9x9_to3_bf16_wgrad_workspace_bytes"           # the weight gradient's entry point and its size query

    def __init__(self, name, cin, cout, k, act=L.ACT_TANH):
        if cin != self.CIN or cout != 3 or k != 9:
            raise NotImplementedError(self.REFUSAL)
        super().__init__(name, cin, cout, k, 1, "same", act)
        self._pk = PackedOperand(self._pack, self)

    def _pack(self, out):
        rt, w = self.rt, self.ps[self.name + "/kernel"]
        wf, wd = out or (None, _bytes(rt, self.DGRAD_PACK_BYTES))
        wf = self.PACK_FWD(rt, w, wf)
        L.check(rt.lib.vcg_pack_conv9x9_3ch_bf16(w.data_ptr(), self.CIN, 1, wd.data_ptr(), rt.stream), "vcg_pack_conv9x9_3ch_bf16")      # data gradient
        return wf, wd

    def forward(self, x, residual=None, tag=None):
        rt = self.rt
        n, h, w, _ = x.shape
        wf, _ = self._pk.get()
        d = self.desc(n, h, w)
        y = rt.empty(n, 3, h, w)
        with Timed(rt, tag):
            L.check(getattr(rt.lib, self.FWD)(ctypes.byref(d), x.data_ptr(), wf.data_ptr(), self.ps[self.name + "/bias"].data_ptr(),
                                              1 if self.act == L.ACT_TANH else 0, y.data_ptr(), rt.stream), self.FWD)
        return y, (x, y, d)

    def backward(self, ctx, dy, need_dx=True, param_grads=True, which=0, dx_residual=None, tag=None, input_lrelu_slope=None, want_channel_sums=False):
        """dy fp32 NCHW; returns dx as bf16 NHWC; with input_lrelu_slope it is already the gradient in front of the LeakyReLU whose output
        x is.  want_channel_sums: returns (dx, (records, count)) -- per-channel sums of dx out of the kernel's epilogue (the producing
        layer's bias gradient, ConvT3x3Bf16.backward)"""
        rt = self.rt
        x, y, d = ctx
        n = d.n
        if dx_residual is not None:
            raise NotImplementedError("%s[%s]: no gradient joins at the head's input" % (type(self).__name__, self.name))
        if (input_lrelu_slope is not None or want_channel_sums) and not self.INPUT_ACT:
            raise NotImplementedError("%s[%s]: no activation mask or channel sums in the data gradient" % (type(self).__name__, self.name))
        db_done = self.act != L.ACT_NONE
        if db_done:
            dy = act_bwd_bias(self, y, dy, d, param_grads, which)
        if param_grads and d.w % 2 == 0:
            # bf16 weight gradient straight from the bf16 NHWC input (transposed LDS reads); dz enters as a bf16 MFMA operand
            ws, wsn = rt.workspace(max(getattr(rt.lib, self.WGRAD_QUERY)(ctypes.byref(d)),
                                       rt.lib.vcg_channel_sum_workspace_bytes(n, 3, d.oh * d.ow)))
            with Timed(rt, tag and tag + "_wgrad"):
                L.check(getattr(rt.lib, self.WGRAD)(ctypes.byref(d), x.data_ptr(), dy.data_ptr(), self.ps.grad(self.name + "/kernel", which).data_ptr(),
                                                    ws, wsn, rt.stream), "%s[%s]" % (self.WGRAD, self.name))
            if not db_done:
                L.check(rt.lib.vcg_channel_sum(dy.data_ptr(), n, 3, d.oh * d.ow, self.ps.grad(self.name + "/bias", which).data_ptr(), ws, wsn,
                                               rt.stream), "vcg_channel_sum[%s]" % self.name)
        elif param_grads:
            # odd widths: the fp32 kernel on an fp32 NCHW copy of the input (exact conversion)
            self._wgrad_fp32(d, from_bf16_nhwc(rt, x), dy, which, not db_done, tag)
        if not need_dx:
            return None
        _, wd = self._pk.get()
        dx = torch.empty_like(x)
        mask = x.data_ptr() if input_lrelu_slope is not None else None
        if want_channel_sums:
            nrec = rt.lib.vcg_conv9x9_to3_bf16_dgrad_chsum_records(ctypes.byref(d))
            L.check(min(nrec, 0), "vcg_conv9x9_to3_bf16_dgrad_chsum_records")
            rec = rt.empty(nrec * self.cin)
            with Timed(rt, tag and tag + "_dgrad"):
                L.check(rt.lib.vcg_conv9x9_to3_bf16_dgrad_chsum(ctypes.byref(d), dy.data_ptr(), wd.data_ptr(), mask, float(input_lrelu_slope or 0.0),
                                                                dx.data_ptr(), rec.data_ptr(), rt.stream), "vcg_conv9x9_to3_bf16_dgrad_chsum")
            return dx, (rec, nrec)
        with Timed(rt, tag and tag + "_dgrad"):
            L.check(rt.lib.vcg_conv9x9_to3_bf16_dgrad(ctypes.byref(d), dy.data_ptr(), wd.data_ptr(), mask, float(input_lrelu_slope or 0.0),
                                                      dx.data_ptr(), rt.stream), self.DGRAD_LABEL % {"name": self.name})
        return dx


class FinalConv9x9Bf16(Conv9x9To3Bf16):
    """final/conv (model.py:290-291) behind the 256-channel up-sampling stage; its data gradient also applies the derivative of the
    LeakyReLU that produced the input and can leave the per-channel sums of the result"""
    CIN, FWD, PACK_FWD, DGRAD_PACK_BYTES, INPUT_ACT = 256, "vcg_conv9x9_to3_bf16_fwd", staticmethod(pack_final9x9_bf16), 4 * L.FIRST9X9_WFRAG_BYTES, True
    REFUSAL, DGRAD_LABEL = "the bf16 final convolution is instantiated for 9x9, 256 -> 3 channels", "vcg_conv9x9_to3_bf16_dgrad"


class HeadConv9x9C64Bf16(Conv9x9To3Bf16):
    """head/conv of make_generator_cyclegan behind the last 64-channel up-sampling stage, which has no activation of its own"""
    CIN, FWD, PACK_FWD, DGRAD_PACK_BYTES, INPUT_ACT = 64, "vcg_conv9x9_c64to3_bf16_fwd", staticmethod(pack_conv9x9_c64to3_bf16), L.FIRST9X9_WFRAG_BYTES, False
    REFUSAL, DGRAD_LABEL = "the bf16 head convolution is instantiated for 9x9, 64 -> 3 channels", "vcg_conv9x9_to3_bf16_dgrad[%(name)s]"


class FinalConv9x9C128Bf16(Conv9x9To3Bf16):
    """final/conv of make_upscaler_attention (model.py:326) behind the 128-channel up-sampling blocks, whose last layer is the Add of
    to_add_input: no activation mask in the data gradient.  Forward on vcg_conv9x9_to3_bf16_fwd (cin 128), weight gradient on
    vcg_conv9x9_c128to3_bf16_wgrad."""
    CIN, FWD, DGRAD_PACK_BYTES, INPUT_ACT = 128, "vcg_conv9x9_to3_bf16_fwd", 2 * L.FIRST9X9_WFRAG_BYTES, False
    PACK_FWD = staticmethod(lambda rt, w, out=None: pack_conv9x9_to3_bf16(rt, w, 128, out))
    REFUSAL, DGRAD_LABEL = "the bf16 final convolution of the attention generator is instantiated for 9x9, 128 -> 3 channels", "vcg_conv9x9_to3_bf16_dgrad[%(name)s]"
    WGRAD, WGRAD_QUERY = "vcg_conv9x9_c128to3_bf16_wgrad", "vcg_conv9x9_c128to3_bf16_wgrad_ws_bytes"



class StemConv9x9Bf16(InitialConv9x9Bf16):
    """stem/conv of make_generator_cyclegan as a graph node: Conv2D(64, 9, 'same') + bias from the fp32 NCHW frames to bf16 NHWC
    (vcg_conv9x9_from3_bf16_fwd without activation; the stem/norm node follows and computes its statistics with the separate pass).
    backward takes the bf16 NHWC gradient the norm's backward returns: weight / bias gradient on vcg_conv3ch_bf16_wgrad (odd widths: the
    fp32 kernel on an fp32 NCHW copy of it).  The input is the network input: no data gradient."""

    def forward(self, x, residual=None, tag=None):
        rt = self.rt
        n, _, h, w = x.shape
        d = self.desc(n, h, w)
        z = torch.empty(n, h, w, self.cout, dtype=torch.bfloat16, device=rt.device)
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv9x9_from3_bf16_fwd(ctypes.byref(d), x.data_ptr(), self._pk.get().data_ptr(), self.ps[self.name + "/bias"].data_ptr(),
                                                      None, z.data_ptr(), rt.stream), "vcg_conv9x9_from3_bf16_fwd[%s]" % self.name)
        return z, (x, None, d)

    def forward_stats(self, x, instance, tag=None):
        z, ctx = self.forward(x, tag=tag)
        return z, ctx, None

    def backward(self, ctx, dz, need_dx=True, param_grads=True, which=0, dx_residual=None, tag=None):
        x, _, d = ctx
        if need_dx:
            raise NotImplementedError("StemConv9x9Bf16[%s] reads the network input: no data gradient" % self.name)
        if param_grads:
            conv3ch_bf16_wgrad(self, d, x, dz, which, tag)
        return None


class GateConvBf16(Conv2D):
    """The input-driven gate of residual_block_attention (model.py:33-36) as one layer on bf16 NHWC: Conv2D(64, k, 'same') of the fp32 NCHW
    frames u + sigmoid + Multiply with the block input m.  forward: y = bf16(sigmoid(conv(u) + bias) * m) on vcg_conv_in_gate_bf16_fwd;
    backward: vcg_conv_in_gate_bf16_bwd recomputes the sigmoid from the frames and writes dm (with the gradient joining at m added before
    the one rounding) and da, from which vcg_conv3ch_bf16_wgrad takes the gate's weight / bias gradient (odd widths: the fp32 kernel on an
    fp32 NCHW copy of da).  The attention tensor is never stored; the context is (u, m).  Declares the Conv2D's parameters under the
    fp32 model's names (res_block/i/attention/kernel, /bias).  The frames are the network input: no gradient goes to u.
    CIN, COUTS: the shapes the class serves; BWD, WGRAD, WGRAD_QUERY: the entry points of its backward."""
    CIN, COUTS, BWD, WGRAD, WGRAD_QUERY = 3, (64,), "vcg_conv_in_gate_bf16_bwd", "vcg_conv3ch_bf16_wgrad", "vcg_conv3ch_bf16_wgrad_workspace_bytes"
    REFUSAL = "the bf16 gate is instantiated for 3x3 / 5x5, 3 -> 64 channels"

    def __init__(self, name, cin=3, cout=64, k=3):
        if cin != self.CIN or cout not in self.COUTS or k not in (3, 5):
            raise NotImplementedError(self.REFUSAL)
        super().__init__(name, cin, cout, k)
        self._pk = PackedOperand(lambda out: pack_conv_in_gate_bf16(self.rt, self.ps[self.name + "/kernel"], cin, k, k, cout, out), self)

    def _check(self, u, m):
        n, c, h, w = u.shape
        if c != self.CIN or m.dtype != torch.bfloat16 or tuple(m.shape) != (n, h, w, self.cout):
            raise TypeError("%s[%s]: u fp32 NCHW [n,%d,h,w], m bf16 NHWC [n,h,w,%d]" % (type(self).__name__, self.name, self.CIN, self.cout))
        return self.desc(n, h, w)

    def forward(self, u, m, tag=None):
        rt = self.rt
        d = self._check(u, m)
        y = torch.empty_like(m)
        with Timed(rt, tag):
            L.check(rt.lib.vcg_conv_in_gate_bf16_fwd(ctypes.byref(d), u.data_ptr(), self._pk.get().data_ptr(), self.ps[self.name + "/bias"].data_ptr(),
                                                     m.data_ptr(), y.data_ptr(), rt.stream), "vcg_conv_in_gate_bf16_fwd[%s]" % self.name)
        return y, (u, m)

    def backward(self, ctx, dy, which=0, dx_residual=None, tag=None):
        """dy: bf16 NHWC gradient at the gate's output; dx_residual: a bf16 NHWC gradient that joins at m (the block's Add) -> dm"""
        rt = self.rt
        u, m = ctx
        d = self._check(u, m)
        for t in (dy, dx_residual):
            if t is not None and (t.dtype != torch.bfloat16 or tuple(t.shape) != tuple(m.shape)):
                raise TypeError("%s[%s]: gradients are bf16 NHWC tensors of m's shape" % (type(self).__name__, self.name))
        dm, da = torch.empty_like(m), torch.empty_like(m)
        with Timed(rt, tag and tag + "_bwd"):
            L.check(getattr(rt.lib, self.BWD)(ctypes.byref(d), u.data_ptr(), self._pk.get().data_ptr(), self.ps[self.name + "/bias"].data_ptr(),
                                              m.data_ptr(), dy.data_ptr(), _ptr(dx_residual), dm.data_ptr(), da.data_ptr(), rt.stream),
                    "%s[%s]" % (self.BWD, self.name))
        conv3ch_bf16_wgrad(self, d, u, da, which, tag, entry=self.WGRAD, query=self.WGRAD_QUERY)
        return dm


class UpGateConvBf16(GateConvBf16):
    """The gate of upsampling_block_attention (model.py:80-90) on bf16 NHWC: u is the fp32 NCHW Concatenate of the nearest and the bilinear
    resize of the frames (6 channels, data only), cout the 64 or 128 channels of the tensor it gates.  Forward on the same
    vcg_conv_in_gate_bf16_fwd; backward on vcg_conv_in_gate_up_bf16_bwd and vcg_conv_in_gate_up_bf16_wgrad (odd widths: the fp32 kernel on
    an fp32 NCHW copy of da).  Parameters under the fp32 model's names (upscaling/i/block/attention/kernel, /bias)."""
    CIN, COUTS, BWD, WGRAD, WGRAD_QUERY = 6, (64, 128), "vcg_conv_in_gate_up_bf16_bwd", "vcg_conv_in_gate_up_bf16_wgrad", "vcg_conv_in_gate_up_bf16_wgrad_ws_bytes"
    REFUSAL = "the bf16 up-sampling gate is instantiated for 3x3 / 5x5, 6 -> 64 or 128 channels"

    def __init__(self, name, cin=6, cout=128, k=3):
        super().__init__(name, cin, cout, k)


class NormActBf16(NormAct):
    """NormAct on bf16 NHWC (same parameters / names): statistics, affine and activation arithmetic in fp32."""
    STATS, ACT_FWD, ACT_BWD = "vcg_norm_stats_bf16", "vcg_norm_act_fwd_bf16", "vcg_norm_act_bwd_bf16"

    def __init__(self, name, c, norm="batch", act=L.ACT_NONE, alpha=0.0, prelu_name=None):
        if norm not in ("batch", "instance"):
            raise ValueError(norm)
        super().__init__(name, c, norm, act, alpha, prelu_name)

    def _dims(self, x):
        n, h, w, c = x.shape
        return n, c, h * w

    def _like(self, x):
        return torch.empty_like(x)

    def _finalize_partials(self, stats, rows, c, count, gamma, beta, eps, mean, scale, shift, invstd, mm, mv, unbiased_n):
        """(records, records per group) of Conv3x3Bf16 / Conv5x5Bf16 / Conv2DBf16.forward_stats"""
        buf, nrec = stats
        L.check(self.rt.lib.vcg_norm_finalize_partials(buf.data_ptr(), nrec, rows, c, count, gamma, beta, eps, mean.data_ptr(), scale.data_ptr(),
                                                       shift.data_ptr(), invstd.data_ptr(), mm, mv, BN_MOMENTUM, unbiased_n, self.rt.stream),
                "vcg_norm_finalize_partials[%s]" % self.name)


# =================================================================================================
# layout helpers at the API edge
# =================================================================================================
def to_device_nchw(rt, x):
    """numpy / torch NHWC float array -> device fp32 NCHW (vcg_nhwc_to_nchw)."""
    if isinstance(x, torch.Tensor):
        t = x.to(device=rt.device, dtype=torch.float32).contiguous()
    else:
        a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
        t = torch.from_numpy(a).to(rt.device)
    if t.dim() != 4:
        raise ValueError("expected a 4-D NHWC batch, got shape %s" % (tuple(t.shape),))
    n, h, w, c = t.shape
    out = rt.empty(n, c, h, w)
    L.check(rt.lib.vcg_nhwc_to_nchw(t.data_ptr(), out.data_ptr(), n, h, w, c, rt.stream), "vcg_nhwc_to_nchw")
    return out


def to_nhwc(rt, t):
    """device NCHW -> device NHWC (vcg_nchw_to_nhwc)."""
    n, c, h, w = t.shape
    out = rt.empty(n, h, w, c)
    L.check(rt.lib.vcg_nchw_to_nhwc(t.data_ptr(), out.data_ptr(), n, h, w, c, rt.stream), "vcg_nchw_to_nhwc")
    return out


def maxpool2x2(rt, x):
    """MaxPooling2D((2,2)) forward: fp32 NCHW -> [n,c,h//2,w//2]"""
    n, c, h, w = x.shape
    y = rt.empty(n, c, h // 2, w // 2)
    L.check(rt.lib.vcg_maxpool2x2_fwd(x.data_ptr(), y.data_ptr(), n, c, h, w, rt.stream), "vcg_maxpool2x2_fwd")
    return y


def maxpool2x2_bwd(rt, x, dy):
    n, c, h, w = x.shape
    dx = rt.empty(n, c, h, w)
    L.check(rt.lib.vcg_maxpool2x2_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), n, c, h, w, rt.stream), "vcg_maxpool2x2_bwd")
    return dx


def maxpool2x2_nhwc_bf16(rt, x):
    """MaxPooling2D((2,2)) forward on bf16 NHWC -> [n,h//2,w//2,c]"""
    n, h, w, c = x.shape
    y = _bf16(rt, n, h // 2, w // 2, c)
    L.check(rt.lib.vcg_maxpool2x2_nhwc_bf16_fwd(x.data_ptr(), y.data_ptr(), n, h, w, c, rt.stream), "vcg_maxpool2x2_nhwc_bf16_fwd")
    return y


def maxpool2x2_relu_nhwc_bf16_bwd(rt, y_prepool, dy):
    """gradient in front of the ReLU whose output y_prepool the pooling read, from the gradient dy at the pooling's output (bf16 NHWC)"""
    n, h, w, c = y_prepool.shape
    dz = torch.empty_like(y_prepool)
    L.check(rt.lib.vcg_maxpool2x2_relu_nhwc_bf16_bwd(y_prepool.data_ptr(), dy.data_ptr(), dz.data_ptr(), n, h, w, c, rt.stream),
            "vcg_maxpool2x2_relu_nhwc_bf16_bwd")
    return dz


def feature_loss_bf16(rt, f_true, f_pred, kind, grad_scale, out=None):
    """(mean squared / absolute difference [1] fp32, bf16 gradient of grad_scale x it in front of the ReLU that produced f_pred) of two bf16
    feature tensors (vcg_feature_loss_bf16); ``out``: a 1-element fp32 view to write the value to"""
    if f_true.shape != f_pred.shape or f_true.dtype != torch.bfloat16 or f_pred.dtype != torch.bfloat16:
        raise TypeError("feature_loss_bf16 takes two bf16 tensors of one shape")
    val, dz = (rt.empty(1) if out is None else out), torch.empty_like(f_pred)
    ws, wsn = rt.workspace(rt.lib.vcg_feature_loss_bf16_ws_bytes(f_pred.numel()))
    L.check(rt.lib.vcg_feature_loss_bf16(f_true.data_ptr(), f_pred.data_ptr(), f_pred.numel(), L.LOSS_MSE if kind == "mse" else L.LOSS_MAE,
                                         float(grad_scale), val.data_ptr(), dz.data_ptr(), ws, wsn, rt.stream), "vcg_feature_loss_bf16")
    return val, dz


def mean_scalar(rt, t, out=None):
    """device scalar tensor holding mean(t) (vcg_mean_reduce); ``out``: a 1-element fp32 view to write it to."""
    if out is None:
        out = rt.empty(1)
    ws, wsn = rt.workspace(rt.lib.vcg_mean_reduce_workspace_bytes(t.numel()))
    L.check(rt.lib.vcg_mean_reduce(t.data_ptr(), t.numel(), out.data_ptr(), ws, wsn, rt.stream), "vcg_mean_reduce")
    return out


def head_act_fwd(rt, z, kind):
    """discriminator output activation (model.py:885-892); kind: _lib.HEAD_*"""
    y = rt.empty(*z.shape)
    L.check(rt.lib.vcg_head_act_fwd(z.data_ptr(), y.data_ptr(), z.numel(), kind, rt.stream), "vcg_head_act_fwd")
    return y


def head_act_bwd(rt, z, dy, kind):
    dz = rt.empty(*z.shape)
    L.check(rt.lib.vcg_head_act_bwd(z.data_ptr(), dy.data_ptr(), dz.data_ptr(), z.numel(), kind, rt.stream), "vcg_head_act_bwd")
    return dz


def gan_loss(rt, mean_a, mean_b, mean_scale, kind, loss_out, da, ga, db=None, gb=0.0):
    """loss_out = act((mean_a - mean_b) * mean_scale); da[:] = act' * ga, db[:] = act' * gb -- all on the device"""
    L.check(rt.lib.vcg_gan_loss(mean_a.data_ptr(), _ptr(mean_b), float(mean_scale), kind, _ptr(loss_out), _ptr(da),
                                da.numel() if da is not None else 0, float(ga), _ptr(db), db.numel() if db is not None else 0,
                                float(gb), rt.stream), "vcg_gan_loss")


def filled_like(rt, t, value):
    out = rt.empty(*t.shape)
    L.check(rt.lib.vcg_fill(out.data_ptr(), out.numel(), float(value), rt.stream), "vcg_fill")
    return out


def axpby(rt, x, y, a, b):
    """y = a*x + b*y"""
    L.check(rt.lib.vcg_axpby(x.data_ptr(), y.data_ptr(), y.numel(), float(a), float(b), rt.stream), "vcg_axpby")

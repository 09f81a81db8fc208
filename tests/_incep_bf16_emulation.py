"""The bf16-emulating forward of make_upscaler_incep_resnet (oracle.generators.upscaler_incep_resnet, upscaling/upscaler/model.py:443-497)
on oracle.keras_ops: what ``Bf16IncepResnetGenerator`` computes, with its roundings marked.  Inference only (BatchNormalization on its
moving statistics).

Rounding points (``bf16=True``):
  * rounded as operands: the frames as initial/conv/9x9 reads them; every convolution kernel; the head's u_p = PReLU(BN(m)) of the block
    input m, per path (a/1, b/1, c/1);
  * rounded when stored: every tensor a launch writes -- initial/conv/9x9's output; each path tensor, behind its single consumer's
    BatchNormalization + PReLU where it has one (b/1 -> b/2/prelu, c/1 -> c/2/prelu, c/2 -> c/3/prelu, 2-path b/2 -> b/3/prelu), raw where
    it feeds the concatenation (a/1, 3-path b/2 and c/3, 2-path b/3); each block output final/add = m + bias + 1x1; the prefinal Add
    (named prefinal/tanh); the tail as in Bf16Generator: every up-sampling stage behind its LeakyReLU;
  * kept unrounded (fp32 on the device): biases, BatchNormalization and PReLU parameters, all epilogue arithmetic, final/conv's output.

``IncepBf16Net`` is an ``oracle.generators.Net`` whose layer methods round at those points, so the emulation is the oracle's own function
``upscaler_incep_resnet`` run on it; with ``bf16=False`` nothing is rounded and it IS the oracle (tests/test_incep_emulation_cpu.py).  The
oracle adds the block input, the long skip and the LeakyReLU outside the Net: the layer in front of them returns the value that makes the
oracle's own `+` / LeakyReLU produce the stored (rounded) tensor (s - gen, resp. s / 0.2 on the negative side: exact in fp64 up to 1e-16).

``taps``: receives every stored tensor (NCHW) under the name the engine's ``forward(x, taps=...)`` uses.

``layer_plan`` lists, in the order of the pass, every stored tensor with the fp64 function that makes it from EARLIER stored tensors: the
teacher-forced reference of one launch (the CPU test runs it on the emulation's own taps, the GPU tests on the device's)."""
import math

import torch

from oracle import generators as OG, keras_ops as K


def _r(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _bn(w, name, x):
    return K.batchnorm(x, w[name + "/gamma"], w[name + "/beta"], w[name + "/moving_mean"], w[name + "/moving_variance"], False)[0]


def _conv(w, name, x):
    return K.conv2d(x, _r(w[name + "/kernel"]), w[name + "/bias"], 1, "same")


class IncepBf16Net(OG.Net):
    def __init__(self, w, bf16=True, taps=None):
        super().__init__(w, False)
        self.r = _r if bf16 else (lambda t: t)
        self.bf16, self.taps, self.gen, self.skip = bf16, taps, None, None

    def keep(self, name, t):
        if self.taps is not None:
            self.taps[name] = t
        return t

    @staticmethod
    def _raw_store(n):
        """is convolution n's output stored as it is (it feeds the concatenation), not behind a consumer's BN + PReLU"""
        if "/a/1/" in n:
            return True
        return ("/b/2/" in n or "/c/3/" in n) if "/3p/" in n else "/b/3/" in n

    def conv2d(self, x, filters, k, stride=1, name=None):
        n = self._name(name, "conv2d")
        if n == "initial/conv/9x9":
            x = self.r(x)
        y = K.conv2d(x, self.r(self.w[n + "/kernel"]), self.w[n + "/bias"], stride, "same")
        if n == "initial/conv/9x9":
            self.skip = self.keep(n, self.r(y))
            return self.skip
        if n.endswith("/final/1x1"):
            s = self.keep(n[:-len("1x1")] + "add", self.r(self.gen + y))
            return s - self.gen if self.bf16 else y
        if n.startswith("inc_res_block/") and self._raw_store(n):
            return self.keep(n, self.r(y))
        return y                          # b/1, c/1, c/2, the 2-path b/2: stored behind the next PReLU; prefinal/conv2d; final/conv

    def bn(self, x, name=None):
        if name.endswith("/a/1/batch_norm"):
            self.gen = x                  # the block input: the first thing a block does (model.py:392, 422)
        y = super().bn(x, name)
        if name == "prefinal/batch_norm":
            s = self.keep("prefinal/tanh", self.r(self.skip + y))
            return s - self.skip if self.bf16 else y
        return y

    def prelu(self, x, name=None):
        y = self.r(super().prelu(x, name))
        if not name.endswith(("/a/1/prelu", "/b/1/prelu", "/c/1/prelu")):          # (those are the head's operands u_p, never stored)
            self.keep(name, y)
        return y

    def conv2d_transpose(self, x, filters, k, stride=2, name=None):
        n = self._name(name, "conv2d_transpose")
        y = K.conv2d_transpose_same(x, self.r(self.w[n + "/kernel"]), self.w[n + "/bias"], stride)
        s = self.keep(n, self.r(K.leaky_relu(y, 0.2)))
        return torch.where(s >= 0, s, s / 0.2) if self.bf16 else y


def incep_forward_emulated(w, x_nhwc, bf16=True, taps=None, **kw):
    """[N,h,w,3] -> [N,h*f,w*f,3]; kw: upscaler_incep_resnet's keywords"""
    y = OG.upscaler_incep_resnet(IncepBf16Net(w, bf16, taps), x_nhwc, **kw)
    if taps is not None:
        taps["final/conv"] = y.permute(0, 3, 1, 2)
    return y


def block_names(a_block_type="3path", a_block_num=5, a_block_kernel=3, b_block_type="2path", b_block_num=10, b_block_kernel=7,
                c_block_type="2path", c_block_num=5, c_block_kernel=3, **_):
    """[(block name, block type, kernel)] in the order of the pass"""
    out = []
    for tag, btype, num, kern in (("A", a_block_type, a_block_num, a_block_kernel), ("B", b_block_type, b_block_num, b_block_kernel),
                                  ("c", c_block_type, c_block_num, c_block_kernel)):
        out += [("inc_res_block/%s/%s/%d" % (tag, {"3path": "3p", "2path": "2p"}[btype], i), btype, kern) for i in range(num)]
    return out


# ---- one launch each: fp64 functions of stored (bf16-valued) tensors, results unrounded --------------------------------------------------
def f_head(w, n, mini, nxt, m):
    """path `mini` of block n's head from the block input m; nxt: the mini-block whose BN + PReLU the epilogue applies, or None"""
    p = "%s/%s" % (n, mini)
    y = _conv(w, p + "/1x1", _r(K.prelu(_bn(w, p + "/batch_norm", m), w[p + "/prelu/alpha"])))
    return y if nxt is None else K.prelu(_bn(w, "%s/%s/batch_norm" % (n, nxt), y), w["%s/%s/prelu/alpha" % (n, nxt)])


def f_mid(w, n, mini, kh, kw, nxt, src):
    y = _conv(w, "%s/%s/%dx%d" % (n, mini, kh, kw), src)
    return y if nxt is None else K.prelu(_bn(w, "%s/%s/batch_norm" % (n, nxt), y), w["%s/%s/prelu/alpha" % (n, nxt)])


def f_join(w, n, srcs, m):
    return m + _conv(w, n + "/final/1x1", torch.cat(srcs, 1))


def layer_plan(w, x_nhwc, upscale_factor=4, **kw):
    """[(name of the stored tensor, fn(taps) -> its fp64 value from the tensors stored before it)]"""
    x = x_nhwc.permute(0, 3, 1, 2)
    plan = [("initial/conv/9x9", lambda t: _conv(w, "initial/conv/9x9", _r(x)))]
    cur = "initial/conv/9x9"
    for n, btype, k in block_names(**kw):
        P = lambda s, n=n: "%s/%s" % (n, s)
        if btype == "3path":
            heads = [("a/1", None, P("a/1/1x1")), ("b/1", "b/2", P("b/2/prelu")), ("c/1", "c/2", P("c/2/prelu"))]
            mids = [("b/2", k, k, None, P("b/2/prelu"), P("b/2/%dx%d" % (k, k))), ("c/2", k, k, "c/3", P("c/2/prelu"), P("c/3/prelu")),
                    ("c/3", k, k, None, P("c/3/prelu"), P("c/3/%dx%d" % (k, k)))]
            srcs = [P("a/1/1x1"), P("b/2/%dx%d" % (k, k)), P("c/3/%dx%d" % (k, k))]
        else:
            heads = [("a/1", None, P("a/1/1x1")), ("b/1", "b/2", P("b/2/prelu"))]
            mids = [("b/2", 1, k, "b/3", P("b/2/prelu"), P("b/3/prelu")), ("b/3", k, 1, None, P("b/3/prelu"), P("b/3/%dx1" % k))]
            srcs = [P("a/1/1x1"), P("b/3/%dx1" % k)]
        for mini, nxt, out in heads:
            plan.append((out, lambda t, n=n, mini=mini, nxt=nxt, cur=cur: f_head(w, n, mini, nxt, t[cur])))
        for mini, kh, kw_, nxt, src, out in mids:
            plan.append((out, lambda t, n=n, mini=mini, kh=kh, kw_=kw_, nxt=nxt, src=src: f_mid(w, n, mini, kh, kw_, nxt, t[src])))
        plan.append((P("final/add"), lambda t, n=n, srcs=srcs, cur=cur: f_join(w, n, [t[s] for s in srcs], t[cur])))
        cur = P("final/add")
    plan.append(("prefinal/tanh", lambda t, cur=cur: t["initial/conv/9x9"] + _bn(w, "prefinal/batch_norm", _conv(w, "prefinal/conv2d", t[cur]))))
    cur = "prefinal/tanh"
    for i in range(int(math.log(upscale_factor, 2))):
        name = "upscaling/%d/block/conv_transp" % i
        plan.append((name, lambda t, name=name, cur=cur: K.leaky_relu(K.conv2d_transpose_same(t[cur], _r(w[name + "/kernel"]), w[name + "/bias"], 2), 0.2)))
        cur = name
    plan.append(("final/conv", lambda t, cur=cur: torch.tanh(_conv(w, "final/conv", t[cur]))))
    return plan

"""The memory contract of include/vcg.h, kernel by kernel: every entry point is called straight through the C ABI with each
buffer inside a guarded arena (tests/_arena.py) and a workspace of EXACTLY the byte count its *_workspace_bytes query returns
(record buffers: exactly records x the documented layout; packed weights: exactly the documented byte counts).

For every row of the table:
  (a) workspace / records / packed weights at their exact size          (d) no NaN in any output documented as written
  (b) the call returns VCG_OK                                            (e) the result matches an fp64 reference within the bound
  (c) the guards of every arena are intact afterwards                    (f) rows with a workspace run twice, the workspace prefilled
                                                                             with 0xFF and with 0x3F: all outputs bit-identical
and a row with a workspace is also called with ws_bytes = need - 1: VCG_E_WORKSPACE, every output arena left at its 0xFF prefill.

Input arenas carry NaN guards (an out-of-range element that reaches a result shows as a NaN), output arenas are prefilled with NaN
("overwritten" must overwrite).  Bounds: a kernel that has a test elsewhere keeps that test's bound against the same kind of
reference (fp32 conv / dense 1e-3 max-norm; bf16 outputs 2^-8 against fp64 on the same bf16-rounded operands plus the
ulp-scaled check < 1; fp32-accumulated gradients and statistics 1e-4 / 1e-5 / 2e-5); kernels with their first direct test here
and the fp32 norm rows (statistics, finalize, forward, backward) are bounded at 1e-5 (element-wise kernels element-wise, sums and the
norm rows in the max-norm), unless the same expression evaluated by torch in
fp32 on the CPU is itself further than 2.5e-6 from the fp64 reference -- then 4x that measured distance (written into the report).

Limit of the method: a load past the end of a buffer that the kernel discards by a select stays invisible.  Only out-of-range
reads that reach a result, and all out-of-range writes within 64 KiB of the buffer, are caught.
"""
import ctypes
import functools
import math
import zlib

import pytest
import torch

import _arena as A
from conftest import report

pytestmark = pytest.mark.gpu

OK, E_WORKSPACE, E_UNSUPPORTED = 0, -4, -3
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
TOL_BF16 = 2.0 ** -8


# ---------------------------------------------------------------------------------------------------------------------------------
# the harness
# ---------------------------------------------------------------------------------------------------------------------------------
class Spec:
    """one table row: inputs {name: cpu tensor}, outputs {name: (shape, dtype)}, call(p, ws, wsn, stream) -> rc with p = {name: pointer},
    ws = exact workspace bytes (None: the entry point takes none), checks = [(output name, reference, kind, bound)] or callables
    outs -> [(label, err, bound)]"""

    def __init__(self, inputs, outputs, call, checks, ws=None, note=""):
        self.inputs, self.outputs, self.call, self.checks, self.ws, self.note = inputs, outputs, call, checks, ws, note


def _max_err(got, ref):
    return float((got.double() - ref).abs().max() / (ref.abs().max() + 1e-30))


def _elem_err(got, ref):
    return float(((got.double() - ref).abs() / (ref.abs() + 1e-6)).max())


def _ulp_scaled(got, ref):
    return float(((got.double() - ref).abs() / (ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max())).max())


def first_test_bound(expr, args, metric):
    """1e-5, unless expr evaluated in fp32 by torch on the CPU is itself further than 2.5e-6 from its fp64 value: then 4x that"""
    r64 = expr(*[a.double() for a in args])
    r32 = expr(*[a.float() for a in args])
    if not isinstance(r64, (tuple, list)):
        r64, r32 = [r64], [r32]
    out = []
    for a, b in zip(r32, r64):
        d = metric(a, b)
        out.append(1e-5 if d <= 2.5e-6 else 4.0 * d)
    return r64, out


def _run_once(rt, spec, ins, ws_fill, ws_bytes=None):
    outs = {k: A.output_arena(shape, dt, rt.device, name=k) for k, (shape, dt) in spec.outputs.items()}
    need = spec.ws if ws_bytes is None else ws_bytes
    ws = A.workspace_arena(need, rt.device, fill=ws_fill) if spec.ws is not None else None
    p = {k: a.ptr for k, a in ins.items()}
    p.update({k: a.ptr for k, a in outs.items()})
    rc = spec.call(p, ws.ptr if ws is not None else None, need if ws is not None else 0, rt.stream)
    torch.cuda.current_stream().synchronize()
    for a in list(ins.values()) + list(outs.values()) + ([ws] if ws is not None else []):
        a.check()                                                       # (c)
    return rc, outs


def run_spec(rt, name, spec):
    ins = {k: A.input_arena(t, rt.device, name=k) for k, t in spec.inputs.items()}
    rc, outs = _run_once(rt, spec, ins, A.NAN_BYTE)
    assert rc == OK, "%s returned %d" % (name, rc)                      # (b)
    got = {k: a.view(a.dtype, a.shape).cpu() for k, a in outs.items()}
    if spec.ws is not None:                                             # (f)
        rc2, outs2 = _run_once(rt, spec, ins, A.JUNK_BYTE)
        assert rc2 == OK
        for k in outs:
            assert torch.equal(outs[k].payload, outs2[k].payload), "%s: output %s depends on the workspace's contents" % (name, k)
        if spec.ws > 0:
            rc3, outs3 = _run_once(rt, spec, ins, A.NAN_BYTE, ws_bytes=spec.ws - 1)
            assert rc3 == E_WORKSPACE, "%s with ws_bytes = need - 1 returned %d" % (name, rc3)
            for k, a in outs3.items():
                assert a.untouched(), "%s refused its workspace but wrote %s" % (name, k)
    for k, t in got.items():                                            # (d)
        bad = torch.isnan(t.float()) if t.dtype.is_floating_point else None
        assert bad is None or not bad.any(), "%s: %d NaN left in %s, first at flat index %d" % (
            name, int(bad.sum()), k, int(bad.flatten().nonzero()[0]))
    figures = []
    for chk in spec.checks:                                             # (e)
        if callable(chk):
            figures += chk(got)
            continue
        k, ref, kind, bound = chk
        g = got[k]
        assert tuple(g.shape) == tuple(ref.shape), (k, g.shape, ref.shape)
        if kind == "bits":
            figures.append((k + " exact", 0.0 if torch.equal(g, ref.to(g.dtype)) else 1.0, 0.5))
        elif kind == "max":
            figures.append((k, _max_err(g, ref), bound))
        elif kind == "elem":
            figures.append((k, _elem_err(g, ref), bound))
        elif kind == "abs":
            figures.append((k, float((g.double() - ref).abs().max()), bound))
        elif kind == "bf16":
            figures.append((k, _max_err(g, ref), TOL_BF16))
            figures.append((k + " ulp-scaled", _ulp_scaled(g, ref), 1.0))
        else:
            raise ValueError(kind)
    report("abi contract %-58s ws=%s %s%s" % (name, "-" if spec.ws is None else spec.ws,
                                               "  ".join("%s=%.2e(<%.1e)" % f for f in figures), "  " + spec.note if spec.note else ""))
    for label, err, bound in figures:
        assert err < bound, "%s: %s err %.3e, bound %.3e" % (name, label, err, bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers shared by the rows
# ---------------------------------------------------------------------------------------------------------------------------------
def _L():
    from upscaler import _lib
    return _lib


def _K():
    from oracle import keras_ops
    return keras_ops


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()) % (2 ** 31))


def _kk(k):
    return (int(k[0]), int(k[1])) if isinstance(k, (tuple, list)) else (int(k), int(k))


def conv_desc(cin, cout, k, stride, padding, n, h, w):
    from upscaler._engine import same_pads
    L = _L()
    kh, kw = _kk(k)
    if padding == "same":
        oh, pt, _ = same_pads(h, kh, stride)
        ow, pl, _ = same_pads(w, kw, stride)
    else:
        p = int(padding)
        oh, ow, pt, pl = (h + 2 * p - kh) // stride + 1, (w + 2 * p - kw) // stride + 1, p, p
    return L.ConvDesc(n, cin, h, w, cout, oh, ow, kh, kw, stride, pt, pl)


def bf(t):
    return t.to(BF16).double()


def nhwc_bf16(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous().to(BF16)


def nchw64(y_nhwc):
    return y_nhwc.double().permute(0, 3, 1, 2).contiguous()


def ref_nhwc(ref_nchw):
    return ref_nchw.permute(0, 2, 3, 1).contiguous()


def lrelu(z, a):
    return torch.where(z >= 0, z, a * z)


def prelu(z, alpha):
    return torch.clamp(z, min=0) + alpha.view(1, -1, 1, 1) * torch.clamp(z, max=0)


def _tag(*a):
    return "x".join(str(v).replace(" ", "") for v in a)


ROWS = []


def rows(fn):
    """fn() -> [(id, builder(rt) -> Spec)]"""
    ROWS.extend(fn())
    return fn


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 convolution
# ---------------------------------------------------------------------------------------------------------------------------------
FP32_CONV = [(64, 64, 3, 1, "same", 1, 13, 45), (3, 64, 9, 1, "same", 1, 16, 40), (256, 3, 9, 1, "same", 1, 20, 70),
             (256, 3, 9, 1, "same", 1, 20, 64), (64, 128, 3, 2, "same", 1, 15, 31), (19, 25, (1, 7), 1, "same", 2, 13, 45),
             (25, 300, (5, 1), 1, "same", 1, 16, 40), (512, 1, 4, 1, 1, 1, 10, 10), (3, 64, 4, 2, 1, 1, 32, 32)]


@functools.lru_cache(maxsize=None)
def _conv_data(case):
    cin, cout, k, stride, padding, n, h, w = case
    K = _K()
    kh, kw = _kk(k)
    g = _gen("conv", cin, cout, kh, kw, h, w)
    x = torch.randn(n, cin, h, w, generator=g)
    wk = torch.randn(kh, kw, cin, cout, generator=g) * (1.0 / math.sqrt(kh * kw * cin))
    b = torch.rand(cout, generator=g) - 0.5
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, wk, b))
    z = K.conv2d(xr, wr, br, stride, padding)
    dy = torch.randn(*z.shape, generator=g)
    res_y = torch.randn(*z.shape, generator=g)
    res_x = torch.randn(n, cin, h, w, generator=g)
    gx, gw, gb = torch.autograd.grad((z * dy.double()).sum(), [xr, wr, br])
    return dict(x=x, w=wk, b=b, dy=dy, res_y=res_y, res_x=res_x, z=z.detach(), gx=gx, gw=gw, gb=gb)


@rows
def _fp32_conv_rows():
    out = []
    for case in FP32_CONV:
        cin, cout, k, stride, padding, n, h, w = case
        tag = _tag(cin, cout, k, "s%d" % stride, padding, n, h, w)

        def fwd(rt, case=case):
            L, D = _L(), _conv_data(case)
            d = conv_desc(*case)

            def call(p, ws, wsn, s):
                ep = L.Epilogue(p["b"], L.ACT_LRELU, 0.2, None, p["res"])
                return rt.lib.vcg_conv2d_fwd(ctypes.byref(d), p["x"], p["w"], p["y"], ctypes.byref(ep), s)
            return Spec(dict(x=D["x"], w=D["w"], b=D["b"], res=D["res_y"]), dict(y=(D["z"].shape, F32)), call,
                        [("y", lrelu(D["z"], 0.2) + D["res_y"].double(), "max", 1e-3)])

        def dgrad(rt, case=case):
            L, D = _L(), _conv_data(case)
            d = conv_desc(*case)
            wt = D["w"].permute(0, 1, 3, 2).contiguous()

            def call(p, ws, wsn, s):
                return rt.lib.vcg_conv2d_dgrad(ctypes.byref(d), p["dy"], p["w"], p["wt"], p["dx"], p["res"], s)
            return Spec(dict(dy=D["dy"], w=D["w"], wt=wt, res=D["res_x"]), dict(dx=(D["x"].shape, F32)), call,
                        [("dx", D["gx"] + D["res_x"].double(), "max", 1e-3)])

        def wgrad(rt, case=case):
            L, D = _L(), _conv_data(case)
            d = conv_desc(*case)

            def call(p, ws, wsn, s):
                return rt.lib.vcg_conv2d_wgrad(ctypes.byref(d), p["x"], p["dy"], p["dw"], p["db"], ws, wsn, s)
            return Spec(dict(x=D["x"], dy=D["dy"]), dict(dw=(D["w"].shape, F32), db=(D["b"].shape, F32)), call,
                        [("dw", D["gw"], "max", 1e-3), ("db", D["gb"], "max", 1e-3)],
                        ws=rt.lib.vcg_conv2d_wgrad_workspace_bytes(ctypes.byref(d)))
        out += [("vcg_conv2d_fwd-" + tag, fwd), ("vcg_conv2d_dgrad-" + tag, dgrad), ("vcg_conv2d_wgrad-" + tag, wgrad)]
    return out


FP32_STATS = [(64, 64, 3, 1, "same", 3, 37, 45, False), (64, 96, 3, 2, "same", 2, 31, 33, True)]


@rows
def _fp32_conv_stats_rows():
    out = []
    for case in FP32_STATS:
        def build(rt, case=case):
            from upscaler import _engine as E
            L, K = _L(), _K()
            cin, cout, k, stride, padding, n, h, w, inst = case
            d = conv_desc(*case[:8])
            g = _gen("cstats", h, w)
            x = torch.randn(n, cin, h, w, generator=g)
            wk = torch.randn(k, k, cin, cout, generator=g) * (1.0 / math.sqrt(k * k * cin))
            b = torch.rand(cout, generator=g) * 6 - 3              # |mean| >> spread for some channels
            mode = L.STATS_INSTANCE if inst else L.STATS_BATCH
            nrec = rt.lib.vcg_conv2d_stats_records(ctypes.byref(d), mode)
            assert nrec > 0, "this shape must be served by the statistics epilogue"
            groups = n if inst else 1
            yref = K.conv2d(x.double(), wk.double(), b.double(), stride, padding)
            cnt = d.oh * d.ow if inst else n * d.oh * d.ow
            eps = E.IN_EPS if inst else E.BN_EPS

            def call(p, ws, wsn, s):
                rc = rt.lib.vcg_conv2d_fwd_stats(ctypes.byref(d), p["x"], p["w"], p["b"], p["y"], p["stats"], s)
                if rc:
                    return rc
                return rt.lib.vcg_norm_finalize_partials_shifted(p["stats"], nrec, groups, cout, float(cnt), p["b"], None, None, eps, p["mean"],
                                                                 p["scale"], p["shift"], p["invstd"], None, None, 0.99, 0, s)

            def stats_check(got):
                yd = got["y"].double()
                dims = (2, 3) if inst else (0, 2, 3)
                m64, v64 = yd.mean(dims).reshape(-1), yd.var(dims, unbiased=False).reshape(-1)
                is64 = 1.0 / torch.sqrt(v64 + eps)
                e_m = float(((got["mean"].double() - m64).abs() / (v64.sqrt() + 1e-6)).max())
                return [("mean(sigmas)", e_m, 1e-5), ("invstd", _max_err(got["invstd"], is64), 1e-5),
                        ("scale", _max_err(got["scale"], is64), 1e-5), ("shift", _max_err(got["shift"], -m64 * is64), 1e-5)]
            gc = groups * cout
            return Spec(dict(x=x, w=wk, b=b),
                        dict(y=(yref.shape, F32), stats=((groups * nrec * 2 * cout,), F32), mean=((gc,), F32), scale=((gc,), F32),
                             shift=((gc,), F32), invstd=((gc,), F32)), call, [("y", yref, "max", 1e-3), stats_check],
                        note="records per group %d" % nrec)
        out.append(("vcg_conv2d_fwd_stats+finalize_partials_shifted-" + _tag(*case), build))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 transposed convolution
# ---------------------------------------------------------------------------------------------------------------------------------
FP32_CONVT = [(64, 256, 3, 2, 7, 19), (64, 256, 5, 1, 9, 33)]


@functools.lru_cache(maxsize=None)
def _convt_data(case):
    cin, cout, k, n, h, w = case
    K = _K()
    g = _gen("convt", k, h, w)
    x = torch.randn(n, cin, h, w, generator=g)
    wk = torch.randn(k, k, cout, cin, generator=g) * (1.0 / (k * math.sqrt(cin)))           # Keras Conv2DTranspose (kh,kw,out,in)
    b = torch.rand(cout, generator=g) - 0.5
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, wk, b))
    z = K.conv2d_transpose_same(xr, wr, br, 2)
    dy = torch.randn(*z.shape, generator=g)
    res_x = torch.randn(n, cin, h, w, generator=g)
    gx, gw, gb = torch.autograd.grad((z * dy.double()).sum(), [xr, wr, br])
    return dict(x=x, w=wk, b=b, dy=dy, res_x=res_x, z=z.detach(), gx=gx, gw=gw, gb=gb)


def convt_desc(cin, cout, k, n, h, w):
    crop = max(k - 2, 0) // 2
    return _L().ConvDesc(n, cin, h, w, cout, 2 * h, 2 * w, k, k, 2, crop, crop)


@rows
def _fp32_convt_rows():
    out = []
    for case in FP32_CONVT:
        tag = _tag(*case)

        def fwd(rt, case=case):
            L, D = _L(), _convt_data(case)
            d = convt_desc(*case)
            wt = D["w"].permute(0, 1, 3, 2).contiguous()                 # per-tap transpose: (kh,kw,in,out)

            def call(p, ws, wsn, s):
                ep = L.Epilogue(p["b"], L.ACT_LRELU, 0.2, None, None)
                return rt.lib.vcg_conv_transpose2d_fwd(ctypes.byref(d), p["x"], p["wt"], p["y"], ctypes.byref(ep), s)
            return Spec(dict(x=D["x"], wt=wt, b=D["b"]), dict(y=(D["z"].shape, F32)), call, [("y", lrelu(D["z"], 0.2), "max", 1e-3)])

        def dgrad(rt, case=case):
            D = _convt_data(case)
            d = convt_desc(*case)

            def call(p, ws, wsn, s):
                return rt.lib.vcg_conv_transpose2d_dgrad(ctypes.byref(d), p["dy"], p["w"], p["dx"], p["res"], s)
            return Spec(dict(dy=D["dy"], w=D["w"], res=D["res_x"]), dict(dx=(D["x"].shape, F32)), call,
                        [("dx", D["gx"] + D["res_x"].double(), "max", 1e-3)])

        def wgrad(rt, case=case):
            D = _convt_data(case)
            d = convt_desc(*case)

            def call(p, ws, wsn, s):
                return rt.lib.vcg_conv_transpose2d_wgrad(ctypes.byref(d), p["x"], p["dy"], p["dw"], p["db"], ws, wsn, s)
            return Spec(dict(x=D["x"], dy=D["dy"]), dict(dw=(D["w"].shape, F32), db=(D["b"].shape, F32)), call,
                        [("dw", D["gw"], "max", 1e-3), ("db", D["gb"], "max", 1e-3)],
                        ws=rt.lib.vcg_conv_transpose2d_wgrad_workspace_bytes(ctypes.byref(d)))
        out += [("vcg_conv_transpose2d_fwd-" + tag, fwd), ("vcg_conv_transpose2d_dgrad-" + tag, dgrad),
                ("vcg_conv_transpose2d_wgrad-" + tag, wgrad)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 normalisation
# ---------------------------------------------------------------------------------------------------------------------------------
# the last two rows take split = 2 slices per group (norm.hip's pick_split): scalar path with the boundary inside a plane, float4 path with
# the slice length rounded up to a multiple of 4
FP32_NORM = [("batch", "prelu", 3, 64, 7, 9), ("instance", "prelu", 2, 256, 6, 10), ("batch", "lrelu", 72, 1024, 1, 1),
             ("batch", "prelu", 3, 5, 37, 45), ("instance", "lrelu", 2, 3, 50, 82)]


def _norm_grads(inst, act, eps, x, dy, gamma, beta, alpha):
    """dx (, dgamma, dbeta) (, dalpha) of sum(dy * act(norm(x))) by autograd, in the dtype of its arguments"""
    c = x.shape[1]
    dims = (2, 3) if inst else (0, 2, 3)
    xr = x.clone().requires_grad_(True)
    gr, br, ar = (t.clone().requires_grad_(True) for t in (gamma, beta, alpha))
    mu, var = xr.mean(dims, keepdim=True), xr.var(dims, unbiased=False, keepdim=True)
    xh = (xr - mu) / torch.sqrt(var + eps)
    u = xh if inst else xh * gr.view(1, c, 1, 1) + br.view(1, c, 1, 1)
    y = prelu(u, ar) if act == "prelu" else torch.where(u > 0, u, 0.1 * u)
    grads = torch.autograd.grad((y * dy).sum(), [xr] + ([] if inst else [gr, br]) + ([ar] if act == "prelu" else []))
    return [t.detach() for t in grads]


@functools.lru_cache(maxsize=None)
def _norm_data(case):
    from upscaler import _engine as E
    norm, act, n, c, h, w = case
    inst = norm == "instance"
    g = _gen("norm", n, c, h, w)
    x = torch.randn(n, c, h, w, generator=g) * 1.7 + 0.4
    res = torch.randn(n, c, h, w, generator=g)
    dy = torch.randn(n, c, h, w, generator=g)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.rand(c, generator=g) - 0.5
    alpha = torch.rand(c, generator=g) * 0.4 + 0.05
    eps = E.IN_EPS if inst else E.BN_EPS
    dims = (2, 3) if inst else (0, 2, 3)
    mu, var = x.double().mean(dims).reshape(-1), x.double().var(dims, unbiased=False).reshape(-1)
    return dict(x=x, res=res, dy=dy, gamma=gamma, beta=beta, alpha=alpha, eps=eps, inst=inst, mean=mu.float(), var=var.float(), var64=var)


@rows
def _fp32_norm_rows():
    out = []
    for case in FP32_NORM:
        norm, act, n, c, h, w = case
        tag = _tag(*case)
        hw = h * w

        def stats(rt, case=case):
            L, D = _L(), _norm_data(case)
            norm, act, n, c, h, w = case
            mode = L.NORM_INSTANCE if D["inst"] else L.NORM_BATCH
            rows_ = n if D["inst"] else 1

            def call(p, ws, wsn, s):
                return rt.lib.vcg_norm_stats(p["x"], n, c, h * w, mode, p["mean"], p["var"], ws, wsn, s)
            dims = (2, 3) if D["inst"] else (0, 2, 3)
            (m64, v64), (bm, bv) = first_test_bound(lambda t: (t.mean(dims).reshape(-1), t.var(dims, unbiased=False).reshape(-1)), [D["x"]], _max_err)
            return Spec(dict(x=D["x"]), dict(mean=((rows_ * c,), F32), var=((rows_ * c,), F32)), call,
                        [("mean", m64, "max", bm), ("var", v64, "max", bv)],
                        ws=rt.lib.vcg_norm_stats_workspace_bytes(n, c, h * w, mode))

        def finalize(rt, case=case):
            D = _norm_data(case)
            norm, act, n, c, h, w = case
            inst = D["inst"]
            rows_ = n if inst else 1
            ga = torch.ones(rows_ * c) if inst else D["gamma"]
            be = torch.zeros(rows_ * c) if inst else D["beta"]

            def expr(m, v, ga_, be_):
                is_ = 1.0 / torch.sqrt(v + D["eps"])
                return ga_ * is_, be_ - m * ga_ * is_, is_
            (sc64, sh64, is64), (bsc, bsh, bis) = first_test_bound(expr, [D["mean"], D["var"], ga, be], _max_err)

            def call(p, ws, wsn, s):
                return rt.lib.vcg_norm_finalize(p["mean"], p["var"], None if inst else p["gamma"], None if inst else p["beta"], c, rows_, D["eps"],
                                                p["scale"], p["shift"], p["invstd"], None, None, 0.0, 0, s)
            o = ((rows_ * c,), F32)
            return Spec(dict(mean=D["mean"], var=D["var"], gamma=D["gamma"], beta=D["beta"]), dict(scale=o, shift=o, invstd=o), call,
                        [("scale", sc64, "max", bsc), ("shift", sh64, "max", bsh), ("invstd", is64, "max", bis)])

        def fwd(rt, case=case):
            L, D = _L(), _norm_data(case)
            norm, act, n, c, h, w = case
            inst = D["inst"]
            rows_ = n if inst else 1
            g = _gen("normfwd", c)
            scale, shift = torch.rand(rows_ * c, generator=g) + 0.5, torch.rand(rows_ * c, generator=g) - 0.5
            code = L.ACT_PRELU if act == "prelu" else L.ACT_LRELU
            shp = (n, c, 1, 1) if inst else (1, c, 1, 1)

            def expr(x_, sc_, sh_, al_, res_):
                u = x_ * sc_.view(shp) + sh_.view(shp)
                return (prelu(u, al_) if act == "prelu" else lrelu(u, 0.1)) + res_
            (ref,), (by,) = first_test_bound(expr, [D["x"], scale, shift, D["alpha"], D["res"]], _max_err)

            def call(p, ws, wsn, s):
                return rt.lib.vcg_norm_act_fwd(p["x"], n, c, h * w, p["scale"], p["shift"], 1 if inst else 0, code, 0.1,
                                               p["alpha"] if act == "prelu" else None, p["res"], p["y"], s)
            return Spec(dict(x=D["x"], scale=scale, shift=shift, alpha=D["alpha"], res=D["res"]), dict(y=(D["x"].shape, F32)), call,
                        [("y", ref, "max", by)])

        def bwd(rt, case=case):
            L, D = _L(), _norm_data(case)
            norm, act, n, c, h, w = case
            inst = D["inst"]
            mode = L.NORM_INSTANCE if inst else L.NORM_BATCH
            code = L.ACT_PRELU if act == "prelu" else L.ACT_LRELU
            invstd = (1.0 / torch.sqrt(D["var64"] + D["eps"])).float()
            grads, bounds = first_test_bound(functools.partial(_norm_grads, inst, act, D["eps"]),
                                             [D["x"], D["dy"], D["gamma"], D["beta"], D["alpha"]], _max_err)
            grads, bounds = list(grads), list(bounds)
            outs, checks = dict(dx=(D["x"].shape, F32)), [("dx", grads.pop(0), "max", bounds.pop(0))]
            if not inst:
                outs.update(dgamma=((c,), F32), dbeta=((c,), F32))
                checks += [("dgamma", grads.pop(0), "max", bounds.pop(0)), ("dbeta", grads.pop(0), "max", bounds.pop(0))]
            if act == "prelu":
                outs.update(dalpha=((c,), F32))
                checks.append(("dalpha", grads.pop(0), "max", bounds.pop(0)))

            def call(p, ws, wsn, s):
                return rt.lib.vcg_norm_act_bwd(p["x"], p["dy"], n, c, h * w, mode, p["mean"], p["invstd"], None if inst else p["gamma"],
                                               None if inst else p["beta"], code, 0.1, p["alpha"] if act == "prelu" else None, 1, p["dx"],
                                               p.get("dgamma"), p.get("dbeta"), p.get("dalpha"), ws, wsn, s)
            return Spec(dict(x=D["x"], dy=D["dy"], mean=D["mean"], invstd=invstd, gamma=D["gamma"], beta=D["beta"], alpha=D["alpha"]), outs, call,
                        checks, ws=rt.lib.vcg_norm_act_bwd_workspace_bytes(n, c, h * w, mode))
        out += [("vcg_norm_stats-" + tag, stats), ("vcg_norm_finalize-" + tag, finalize), ("vcg_norm_act_fwd-" + tag, fwd),
                ("vcg_norm_act_bwd-" + tag, bwd)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the remaining fp32 kernels
# ---------------------------------------------------------------------------------------------------------------------------------
ACT_BWD = [("prelu", 2, 64, 9, 20), ("lrelu", 3, 5, 7, 9), ("tanh", 1, 3, 37, 128)]


@rows
def _act_bwd_rows():
    out = []
    for case in ACT_BWD:
        def build(rt, case=case):
            L = _L()
            act, n, c, h, w = case
            g = _gen("actbwd", c, h)
            x = torch.randn(n, c, h, w, generator=g)
            dy = torch.randn(n, c, h, w, generator=g)
            alpha = torch.rand(c, generator=g) * 0.4 + 0.05
            if act == "prelu":
                saved, code = x, L.ACT_PRELU

                def expr(sv, dy_, al):
                    dx = dy_ * torch.where(sv >= 0, torch.ones_like(sv), al.view(1, -1, 1, 1).expand_as(sv))
                    return dx, (dy_ * torch.clamp(sv, max=0)).sum((0, 2, 3)), dx.sum((0, 2, 3))
            elif act == "lrelu":
                saved, code = torch.where(x >= 0, x, 0.2 * x), L.ACT_LRELU          # the saved OUTPUT

                def expr(sv, dy_, al):
                    dx = dy_ * torch.where(sv > 0, torch.ones_like(sv), torch.full_like(sv, 0.2))
                    return dx, None, dx.sum((0, 2, 3))
            else:
                saved, code = torch.tanh(x), L.ACT_TANH

                def expr(sv, dy_, al):
                    dx = dy_ * (1 - sv * sv)
                    return dx, None, dx.sum((0, 2, 3))
            r64 = expr(saved.double(), dy.double(), alpha.double())
            r32 = expr(saved, dy, alpha)
            bounds = [None if a is None else (lambda d: 1e-5 if d <= 2.5e-6 else 4 * d)(m(a, b))
                      for a, b, m in zip(r32, r64, (_elem_err, _max_err, _max_err))]
            outs, checks = dict(dx=(x.shape, F32), dsum=((c,), F32)), [("dx", r64[0], "elem", bounds[0]), ("dsum", r64[2], "max", bounds[2])]
            if act == "prelu":
                outs["dalpha"] = ((c,), F32)
                checks.append(("dalpha", r64[1], "max", bounds[1]))

            def call(p, ws, wsn, s):
                return rt.lib.vcg_act_bwd(p["saved"], p["dy"], n, c, h * w, code, 0.2, p["alpha"] if act == "prelu" else None, p["dx"],
                                          p.get("dalpha"), p["dsum"], ws, wsn, s)
            return Spec(dict(saved=saved, dy=dy, alpha=alpha), outs, call, checks, ws=rt.lib.vcg_act_bwd_workspace_bytes(n, c, h * w))
        out.append(("vcg_act_bwd-" + _tag(*case), build))
    return out


@rows
def _reduction_rows():
    def channel_sum(rt):
        n, c, hw = 3, 5, 7 * 9 * 11                     # 693 per plane, 10395 in all: no multiple of 256
        x = torch.randn(n, c, hw, generator=_gen("chsum"))
        (ref,), (b,) = first_test_bound(lambda t: t.sum((0, 2)), [x], _max_err)

        def call(p, ws, wsn, s):
            return rt.lib.vcg_channel_sum(p["x"], n, c, hw, p["out"], ws, wsn, s)
        return Spec(dict(x=x), dict(out=((c,), F32)), call, [("out", ref, "max", b)], ws=rt.lib.vcg_channel_sum_workspace_bytes(n, c, hw))

    def sum_records(rt):
        nrec, c = 37, 70
        part = torch.randn(nrec, c, generator=_gen("sumrec"))
        (ref,), (b,) = first_test_bound(lambda t: 0.5 * t.sum(0), [part], _max_err)

        def call(p, ws, wsn, s):
            return rt.lib.vcg_sum_records(p["part"], nrec, c, 0.5, p["out"], s)
        return Spec(dict(part=part), dict(out=((c,), F32)), call, [("out", ref, "max", b)])

    def mean_reduce(rt):
        count = 10007
        x = torch.rand(count, generator=_gen("mean")) * 2 - 0.5

        def call(p, ws, wsn, s):
            return rt.lib.vcg_mean_reduce(p["x"], count, p["out"], ws, wsn, s)
        return Spec(dict(x=x), dict(out=((1,), F32)), call, [("out", x.double().mean().view(1), "abs", 1e-6)],
                    ws=rt.lib.vcg_mean_reduce_workspace_bytes(count))

    def pixel_loss(kind):
        def build(rt):
            L = _L()
            g = _gen("pixel", kind)
            a, b = torch.randn(2, 3, 17, 19, generator=g), torch.randn(2, 3, 17, 19, generator=g)
            count = a.numel()                          # 1938
            ar = a.double().requires_grad_(True)
            lv = ((ar - b.double()) ** 2).mean() if kind == "mse" else (ar - b.double()).abs().mean()
            (da,) = torch.autograd.grad(0.7 * lv, [ar])

            def call(p, ws, wsn, s):
                return rt.lib.vcg_pixel_loss(p["a"], p["b"], count, L.LOSS_MSE if kind == "mse" else L.LOSS_MAE, 0.7, p["out"], p["da"], ws, wsn, s)
            return Spec(dict(a=a, b=b), dict(out=((1,), F32), da=(a.shape, F32)), call,
                        [("out", lv.detach().view(1), "max", 1e-5), ("da", da, "max", 1e-5)], ws=rt.lib.vcg_mean_reduce_workspace_bytes(count))
        return build
    return [("vcg_channel_sum-3x5x693", channel_sum), ("vcg_sum_records-37x70", sum_records), ("vcg_mean_reduce-10007", mean_reduce),
            ("vcg_pixel_loss-mse-1938", pixel_loss("mse")), ("vcg_pixel_loss-mae-1938", pixel_loss("mae"))]


@rows
def _dense_rows():
    b, cin, cout = 2, 77, 130

    @functools.lru_cache(maxsize=None)
    def data():
        g = _gen("dense")
        x, wk, bias = torch.randn(b, cin, generator=g), torch.randn(cin, cout, generator=g) * 0.1, torch.rand(cout, generator=g) - 0.5
        xr, wr, br = (t.double().requires_grad_(True) for t in (x, wk, bias))
        y = _K().dense(xr, wr, br)
        dy = torch.randn(b, cout, generator=g)
        gx, gw, gb = torch.autograd.grad((y * dy.double()).sum(), [xr, wr, br])
        return dict(x=x, w=wk, b=bias, dy=dy, y=y.detach(), gx=gx, gw=gw, gb=gb)

    def fwd(rt):
        D = data()
        return Spec(dict(x=D["x"], w=D["w"], b=D["b"]), dict(y=((b, cout), F32)),
                    lambda p, ws, wsn, s: rt.lib.vcg_dense_fwd(p["x"], p["w"], p["b"], p["y"], b, cin, cout, s), [("y", D["y"], "max", 1e-3)])

    def dgrad(rt):
        D = data()
        return Spec(dict(dy=D["dy"], w=D["w"]), dict(dx=((b, cin), F32)),
                    lambda p, ws, wsn, s: rt.lib.vcg_dense_dgrad(p["dy"], p["w"], p["dx"], b, cin, cout, s), [("dx", D["gx"], "max", 1e-3)])

    def wgrad(rt):
        D = data()
        return Spec(dict(x=D["x"], dy=D["dy"]), dict(dw=((cin, cout), F32), db=((cout,), F32)),
                    lambda p, ws, wsn, s: rt.lib.vcg_dense_wgrad(p["x"], p["dy"], p["dw"], p["db"], b, cin, cout, s),
                    [("dw", D["gw"], "max", 1e-3), ("db", D["gb"], "max", 1e-3)])
    return [("vcg_dense_fwd-2x77x130", fwd), ("vcg_dense_dgrad-2x77x130", dgrad), ("vcg_dense_wgrad-2x77x130", wgrad)]


@rows
def _elementwise_rows():
    ODD = (3, 5, 11, 14)

    def kernel_transpose(rt):
        taps, a, b = 15, 11, 14
        w = torch.randn(taps, a, b, generator=_gen("ktr"))
        return Spec(dict(src=w), dict(dst=((taps, b, a), F32)),
                    lambda p, ws, wsn, s: rt.lib.vcg_kernel_transpose(p["src"], p["dst"], taps, a, b, s), [("dst", w.transpose(1, 2).contiguous(), "bits", 0)])

    def _fold_inputs(g, c):
        # values without cancellation in (bias - mean) * scale + beta, so that the element-wise relative error is that of the arithmetic
        return (torch.rand(c, generator=g) * 0.5 + 0.5, -torch.rand(c, generator=g) * 0.5, torch.rand(c, generator=g) * 1.5 + 0.5,
                torch.rand(c, generator=g) + 0.5, torch.rand(c, generator=g) + 1.0)

    def _fold(bias, mm, mv, ga, be):
        sc = ga / torch.sqrt(mv + 1e-3)
        return sc, (bias - mm) * sc + be

    def bn_fold(rt):
        c = 70
        ins = _fold_inputs(_gen("fold"), c)
        (sc, sh), (b0, b1) = first_test_bound(_fold, ins, _elem_err)

        def call(p, ws, wsn, s):
            return rt.lib.vcg_bn_fold(p["bias"], p["mm"], p["mv"], p["ga"], p["be"], c, 1e-3, p["scale"], p["shift"], s)
        return Spec(dict(zip(("bias", "mm", "mv", "ga", "be"), ins)), dict(scale=((c,), F32), shift=((c,), F32)), call,
                    [("scale", sc, "elem", b0), ("shift", sh, "elem", b1)])

    def bn_fold_batch(rt):
        count, c = 3, 64
        g = _gen("foldb")
        ins = [torch.stack(t) for t in zip(*[_fold_inputs(g, c) for _ in range(count)])]           # five [count][c] tensors
        (sc, sh), (b0, b1) = first_test_bound(_fold, ins, _elem_err)

        def call(p, ws, wsn, s):
            col = lambda k: (ctypes.c_void_p * count)(*[p[k] + 4 * c * i for i in range(count)])
            return rt.lib.vcg_bn_fold_batch(col("bias"), col("mm"), col("mv"), col("ga"), col("be"), count, c, 1e-3, p["scale"], p["shift"], s)
        return Spec(dict(zip(("bias", "mm", "mv", "ga", "be"), ins)), dict(scale=((count, c), F32), shift=((count, c), F32)), call,
                    [("scale", sc, "elem", b0), ("shift", sh, "elem", b1)])

    def gate_fwd(rt):
        g = _gen("gate")
        a, m = torch.randn(*ODD, generator=g) * 3, torch.randn(*ODD, generator=g)
        (ref,), (b,) = first_test_bound(lambda a_, m_: torch.sigmoid(a_) * m_, [a, m], _elem_err)
        return Spec(dict(a=a, m=m), dict(y=(ODD, F32)), lambda p, ws, wsn, s: rt.lib.vcg_sigmoid_gate_fwd(p["a"], p["m"], p["y"], a.numel(), s),
                    [("y", ref, "elem", b)])

    def gate_bwd(rt):
        g = _gen("gateb")
        a, m, dy = torch.randn(*ODD, generator=g) * 3, torch.randn(*ODD, generator=g), torch.randn(*ODD, generator=g)

        def expr(a_, m_, dy_):
            sg = torch.sigmoid(a_)
            return dy_ * m_ * sg * (1 - sg), dy_ * sg
        (da, dm), (b0, b1) = first_test_bound(expr, [a, m, dy], _elem_err)
        return Spec(dict(a=a, m=m, dy=dy), dict(da=(ODD, F32), dm=(ODD, F32)),
                    lambda p, ws, wsn, s: rt.lib.vcg_sigmoid_gate_bwd(p["a"], p["m"], p["dy"], p["da"], p["dm"], a.numel(), s),
                    [("da", da, "elem", b0), ("dm", dm, "elem", b1)])

    def atanh_scale(rt):
        g = _gen("atanh")
        x = torch.cat([torch.rand(2303, generator=g) * 2 - 1, torch.tensor([0.0, 1.0, -1.0, 1e-6, -1e-6, 0.999, -0.999])])
        scale = torch.tensor(0.99999, dtype=torch.float32)
        (ref,), (b,) = first_test_bound(lambda x_, s_: torch.atanh(s_ * x_), [x, scale], _elem_err)
        return Spec(dict(x=x), dict(y=(x.shape, F32)), lambda p, ws, wsn, s: rt.lib.vcg_atanh_scale(p["x"], p["y"], x.numel(), float(scale), s),
                    [("y", ref, "elem", b)], note="bound used %.2e" % b)

    def dilate(rt):
        n, c, h, w = ODD
        st = 3
        x = torch.randn(*ODD, generator=_gen("dil"))
        ref = torch.zeros(n, c, (h - 1) * st + 1, (w - 1) * st + 1)
        ref[:, :, ::st, ::st] = x
        return Spec(dict(src=x), dict(dst=(ref.shape, F32)), lambda p, ws, wsn, s: rt.lib.vcg_dilate2d(p["src"], p["dst"], n * c, h, w, st, s),
                    [("dst", ref, "bits", 0)])

    def maxpool_fwd(rt):
        n, c, h, w = 3, 5, 11, 13
        x = torch.randn(n, c, h, w, generator=_gen("mp"))
        ref = torch.nn.functional.max_pool2d(x, 2)
        return Spec(dict(x=x), dict(y=(ref.shape, F32)), lambda p, ws, wsn, s: rt.lib.vcg_maxpool2x2_fwd(p["x"], p["y"], n, c, h, w, s),
                    [("y", ref, "bits", 0)])

    def maxpool_bwd(rt):
        n, c, h, w = 3, 5, 11, 13
        g = _gen("mpb")
        x = torch.randn(n, c, h, w, generator=g)
        dy = torch.randn(n, c, h // 2, w // 2, generator=g)
        xr = x.clone().requires_grad_(True)
        (ref,) = torch.autograd.grad((torch.nn.functional.max_pool2d(xr, 2) * dy).sum(), [xr])        # zeros in the odd last row / column
        return Spec(dict(x=x, dy=dy), dict(dx=(x.shape, F32)), lambda p, ws, wsn, s: rt.lib.vcg_maxpool2x2_bwd(p["x"], p["dy"], p["dx"], n, c, h, w, s),
                    [("dx", ref, "bits", 0)])

    def resize(bilinear):
        def build(rt):
            from oracle import models as M
            f = 2
            x = torch.randn(2, 3, 13, 17, generator=_gen("rs"))
            ref = M.resize_images_tf1(x.double(), f, "bilinear" if bilinear else "nearest")
            return Spec(dict(src=x), dict(dst=(ref.shape, F32)), lambda p, ws, wsn, s: rt.lib.vcg_resize2d(p["src"], p["dst"], 6, 13, 17, f, bilinear, s),
                        [("dst", ref, "abs", 2e-6) if bilinear else ("dst", ref, "bits", 0)])
        return build

    def crop(rt):
        x = torch.randn(*ODD, generator=_gen("crop"))
        return Spec(dict(src=x), dict(dst=((3, 5, 8, 9), F32)), lambda p, ws, wsn, s: rt.lib.vcg_crop2d(p["src"], p["dst"], 15, 11, 14, 1, 3, 8, 9, s),
                    [("dst", x[:, :, 1:9, 3:12].contiguous(), "bits", 0)])

    def pad(rt):
        y = torch.randn(3, 5, 8, 9, generator=_gen("pad"))
        ref = torch.zeros(*ODD)
        ref[:, :, 1:9, 3:12] = y
        return Spec(dict(src=y), dict(dst=(ODD, F32)), lambda p, ws, wsn, s: rt.lib.vcg_pad2d(p["src"], p["dst"], 15, 8, 9, 1, 3, 11, 14, s),
                    [("dst", ref, "bits", 0)])

    def copy_channels(rt):
        src = torch.randn(2, 7, 6, 7, generator=_gen("cc"))

        def call(p, ws, wsn, s):        # channels 2..6 of src into channels 1..5 of a 6-channel dst, then channel 0 of src into channel 0
            rc = rt.lib.vcg_copy_channels(p["src"], p["dst"], 2, 7, 2, 6, 1, 5, 42, s)
            return rc or rt.lib.vcg_copy_channels(p["src"], p["dst"], 2, 7, 0, 6, 0, 1, 42, s)
        return Spec(dict(src=src), dict(dst=((2, 6, 6, 7), F32)), call, [("dst", torch.cat([src[:, 0:1], src[:, 2:7]], 1).contiguous(), "bits", 0)])

    def layout(which):
        def build(rt):
            n, h, w, c = 2, 9, 11, 3
            g = _gen("layout", which)
            lib = rt.lib
            if which == "nhwc_to_nchw":
                x = torch.randn(n, h, w, c, generator=g)
                return Spec(dict(x=x), dict(y=((n, c, h, w), F32)), lambda p, ws, wsn, s: lib.vcg_nhwc_to_nchw(p["x"], p["y"], n, h, w, c, s),
                            [("y", x.permute(0, 3, 1, 2).contiguous(), "bits", 0)])
            if which == "nchw_to_nhwc":
                x = torch.randn(n, c, h, w, generator=g)
                return Spec(dict(x=x), dict(y=((n, h, w, c), F32)), lambda p, ws, wsn, s: lib.vcg_nchw_to_nhwc(p["x"], p["y"], n, h, w, c, s),
                            [("y", x.permute(0, 2, 3, 1).contiguous(), "bits", 0)])
            if which == "f32_nchw_to_bf16_nhwc":
                c = 72
                x = torch.randn(n, c, h, w, generator=g)
                return Spec(dict(x=x), dict(y=((n, h, w, c), BF16)), lambda p, ws, wsn, s: lib.vcg_f32_nchw_to_bf16_nhwc(p["x"], p["y"], n, c, h, w, s),
                            [("y", nhwc_bf16(x), "bits", 0)])
            if which == "bf16_nhwc_to_f32_nchw":
                c = 72
                x = torch.randn(n, h, w, c, generator=g).to(BF16)
                return Spec(dict(x=x), dict(y=((n, c, h, w), F32)), lambda p, ws, wsn, s: lib.vcg_bf16_nhwc_to_f32_nchw(p["x"], p["y"], n, c, h, w, s),
                            [("y", x.float().permute(0, 3, 1, 2).contiguous(), "bits", 0)])
            if which == "frames_u8_to_nchw":
                from oracle import data as OD
                u8 = torch.randint(0, 256, (n, h, w, c), generator=g, dtype=U8)
                ref = torch.tensor(OD.convert_uint8_to_array(u8.numpy())).permute(0, 3, 1, 2).float().contiguous()
                return Spec(dict(x=u8), dict(y=((n, c, h, w), F32)), lambda p, ws, wsn, s: lib.vcg_frames_u8_to_nchw(p["x"], p["y"], n, h, w, c, s),
                            [("y", ref, "bits", 0)])
            if which == "nchw_to_frames_u8":
                from oracle import data as OD
                import numpy as np
                xs = torch.rand(n, h, w, c, generator=g) * 2 - 1
                ref = torch.from_numpy(OD.convert_array_to_uint8(xs.numpy().astype(np.float32)))
                return Spec(dict(x=xs.permute(0, 3, 1, 2).contiguous()), dict(y=((n, h, w, c), U8)),
                            lambda p, ws, wsn, s: lib.vcg_nchw_to_frames_u8(p["x"], p["y"], n, h, w, c, s), [("y", ref, "bits", 0)])
            count = 2311
            if which == "f32_to_bf16":
                x = torch.randn(count, generator=g)
                return Spec(dict(x=x), dict(y=((count,), BF16)), lambda p, ws, wsn, s: lib.vcg_f32_to_bf16(p["x"], p["y"], count, s),
                            [("y", x.to(BF16), "bits", 0)])
            x = torch.randn(count, generator=g).to(BF16)
            return Spec(dict(x=x), dict(y=((count,), F32)), lambda p, ws, wsn, s: lib.vcg_bf16_to_f32(p["x"], p["y"], count, s), [("y", x.float(), "bits", 0)])
        return build
    return [("vcg_kernel_transpose-15x11x14", kernel_transpose), ("vcg_bn_fold-c70", bn_fold), ("vcg_bn_fold_batch-3xc64", bn_fold_batch),
            ("vcg_sigmoid_gate_fwd-3x5x11x14", gate_fwd), ("vcg_sigmoid_gate_bwd-3x5x11x14", gate_bwd), ("vcg_atanh_scale-2310", atanh_scale),
            ("vcg_dilate2d-s3-3x5x11x14", dilate), ("vcg_maxpool2x2_fwd-3x5x11x13", maxpool_fwd), ("vcg_maxpool2x2_bwd-3x5x11x13", maxpool_bwd),
            ("vcg_resize2d-nearest-13x17", resize(0)), ("vcg_resize2d-bilinear-13x17", resize(1)), ("vcg_crop2d-11x14", crop), ("vcg_pad2d-8x9", pad),
            ("vcg_copy_channels-2x7x42", copy_channels)] + \
        [("vcg_" + k, layout(k)) for k in ("nhwc_to_nchw", "nchw_to_nhwc", "f32_nchw_to_bf16_nhwc", "bf16_nhwc_to_f32_nchw", "frames_u8_to_nchw",
                                           "nchw_to_frames_u8", "f32_to_bf16", "bf16_to_f32")]


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16: weight packing (bit-exact against torch's rounding)
# ---------------------------------------------------------------------------------------------------------------------------------
def _same_values(name, w, pad_to):
    """a fragment layout holds exactly the bf16 roundings of w (torch's round-to-nearest-even) plus zero padding, whatever the order:
    the order itself is pinned by the convolutions that multiply these fragments"""
    def chk(got):
        g = got[name].view(torch.int16).flatten().sort().values
        ref = torch.cat([w.to(BF16).view(torch.int16).flatten(), torch.zeros(pad_to - w.numel(), dtype=torch.int16)]).sort().values
        return [(name + " values exact", 0.0 if g.numel() == ref.numel() and torch.equal(g, ref) else 1.0, 0.5)]
    return chk


def _pack_frag_cpu(rt, w, taps, mdim, kdim, mode):
    L = _L()
    wd = w.to(rt.device)
    out = torch.empty(taps * mdim * kdim, dtype=BF16, device=rt.device)
    L.check(rt.lib.vcg_pack_conv_frag_bf16(wd.data_ptr(), taps, mdim, kdim, mode, out.data_ptr(), rt.stream), "vcg_pack_conv_frag_bf16")
    torch.cuda.current_stream().synchronize()
    return out.cpu()


@rows
def _pack_rows():
    def pack_kernel(transpose, flip):
        def build(rt):
            taps, a, b = 9, 64, 48
            w = torch.randn(taps, b, a, generator=_gen("pk")) if transpose else torch.randn(taps, a, b, generator=_gen("pk"))
            ref = w.transpose(1, 2) if transpose else w
            ref = (ref.flip(0) if flip else ref).contiguous().to(BF16)
            return Spec(dict(w=w), dict(out=((taps, a, b), BF16)),
                        lambda p, ws, wsn, s: rt.lib.vcg_pack_conv_kernel_bf16(p["w"], taps, a, b, transpose, flip, p["out"], s), [("out", ref, "bits", 0)])
        return build

    def pack_batch(rt):
        count = 3
        w = torch.randn(count, 9, 64, 64, generator=_gen("pkb"))             # Keras (3,3,in,out) each
        fwd = w.transpose(2, 3)                                                # [tap][out][in]
        dgr = w.flip(1)                                                        # [tap'][in][out]
        ref = torch.stack([fwd, dgr], 1).contiguous().to(BF16)

        def call(p, ws, wsn, s):
            arr = (ctypes.c_void_p * count)(*[p["w"] + 4 * 9 * 64 * 64 * i for i in range(count)])
            return rt.lib.vcg_pack_conv3x3_c64_bf16_batch(arr, count, p["out"], s)
        return Spec(dict(w=w), dict(out=((count, 2, 9, 64, 64), BF16)), call, [("out", ref, "bits", 0)])

    def pack_frag(mode):
        def build(rt):
            taps, cin, cout = 9, 96, 64
            w = torch.randn(taps, cin, cout, generator=_gen("pf"))
            mdim, kdim = (cout, cin) if mode == 0 else (cin, cout)
            nb = rt.lib.vcg_conv_frag_bf16_bytes(taps, mdim, kdim)
            assert nb == taps * cin * cout * 2
            return Spec(dict(w=w), dict(out=((nb // 2,), BF16)),
                        lambda p, ws, wsn, s: rt.lib.vcg_pack_conv_frag_bf16(p["w"], taps, mdim, kdim, mode, p["out"], s),
                        [_same_values("out", w, nb // 2)])
        return build

    def pack_pair(rt):
        taps, cin, cout = 16, 96, 64
        w = torch.randn(taps, cin, cout, generator=_gen("pp"))
        nb = rt.lib.vcg_conv_frag_bf16_bytes(taps, cout, cin)
        f0, f1 = _pack_frag_cpu(rt, w, taps, cout, cin, 0), _pack_frag_cpu(rt, w, taps, cin, cout, 1)       # the two single calls
        return Spec(dict(w=w), dict(fwd=((nb // 2,), BF16), dgrad=((nb // 2,), BF16)),
                    lambda p, ws, wsn, s: rt.lib.vcg_pack_conv_frag_bf16_pair(p["w"], taps, cin, cout, p["fwd"], p["dgrad"], s),
                    [("fwd", f0, "bits", 0), ("dgrad", f1, "bits", 0), _same_values("fwd", w, nb // 2)])

    def pack_final(rt):
        L = _L()
        w = torch.randn(9, 9, 256, 3, generator=_gen("pfin"))
        return Spec(dict(w=w), dict(out=((L.FINAL9X9_WFRAG_BYTES // 2,), BF16)), lambda p, ws, wsn, s: rt.lib.vcg_pack_final9x9_bf16(p["w"], p["out"], s),
                    [_same_values("out", w, L.FINAL9X9_WFRAG_BYTES // 2)])

    def pack_first(rt):
        L = _L()
        w = torch.randn(9, 9, 3, 64, generator=_gen("pfst"))
        return Spec(dict(w=w), dict(out=((L.FIRST9X9_WFRAG_BYTES // 2,), BF16)), lambda p, ws, wsn, s: rt.lib.vcg_pack_first9x9_bf16(p["w"], p["out"], s),
                    [_same_values("out", w, L.FIRST9X9_WFRAG_BYTES // 2)])

    def pack_9x9_3ch(dgrad):
        def build(rt):
            L = _L()
            cout = 256
            w = torch.randn(9, 9, cout, 3, generator=_gen("p93")) if dgrad else torch.randn(9, 9, 3, cout, generator=_gen("p93"))
            nb = 4 * L.FIRST9X9_WFRAG_BYTES
            return Spec(dict(w=w), dict(out=((nb // 2,), BF16)), lambda p, ws, wsn, s: rt.lib.vcg_pack_conv9x9_3ch_bf16(p["w"], cout, dgrad, p["out"], s),
                        [_same_values("out", w, nb // 2)])
        return build

    def pack_3ch(k):
        def build(rt):
            cout = 128
            w = torch.randn(k, k, 3, cout, generator=_gen("p3", k))
            nb = rt.lib.vcg_conv3ch_bf16_wfrag_bytes(k, k, cout)
            assert nb > 0
            return Spec(dict(w=w), dict(out=((nb // 2,), BF16)), lambda p, ws, wsn, s: rt.lib.vcg_pack_conv3ch_bf16(p["w"], k, k, cout, p["out"], s),
                        [_same_values("out", w, nb // 2)])
        return build
    return [("vcg_pack_conv_kernel_bf16-t%d-f%d" % tf, pack_kernel(*tf)) for tf in ((1, 0), (0, 1), (0, 0), (1, 1))] + \
        [("vcg_pack_conv3x3_c64_bf16_batch-3", pack_batch), ("vcg_pack_conv_frag_bf16-mode0", pack_frag(0)), ("vcg_pack_conv_frag_bf16-mode1", pack_frag(1)),
         ("vcg_pack_conv_frag_bf16_pair-16x96x64", pack_pair), ("vcg_pack_final9x9_bf16", pack_final), ("vcg_pack_first9x9_bf16", pack_first),
         ("vcg_pack_conv9x9_3ch_bf16-fwd", pack_9x9_3ch(0)), ("vcg_pack_conv9x9_3ch_bf16-dgrad", pack_9x9_3ch(1)),
         ("vcg_pack_conv3ch_bf16-k3", pack_3ch(3)), ("vcg_pack_conv3ch_bf16-k4", pack_3ch(4))]


def _packed(rt, fn, w, nbytes, *args):
    """bytes of a packed weight buffer made by pack function fn(w, *args, out, stream), as a CPU uint8 tensor of exactly nbytes"""
    L = _L()
    wd = w.to(rt.device)
    out = torch.empty(nbytes, dtype=U8, device=rt.device)
    L.check(fn(wd.data_ptr(), *args, out.data_ptr(), rt.stream), "pack")
    torch.cuda.current_stream().synchronize()
    return out.cpu()


def _partials_check(got, y_key, nrec, groups, c, inst, eps, tol=2e-5):
    """mean / invstd finalized from epilogue records against the fp64 statistics of the STORED bf16 NHWC tensor"""
    yd = got[y_key].double()
    dims = (1, 2) if inst else (0, 1, 2)
    m64, v64 = yd.mean(dims).reshape(-1), yd.var(dims, unbiased=False).reshape(-1)
    is64 = 1.0 / torch.sqrt(v64 + eps)
    e_m = float((got["mean"].double() - m64).abs().max()) / float(v64.sqrt().max())
    return [("mean(sigmas)", e_m, tol), ("invstd", _max_err(got["invstd"], is64), tol), ("scale", _max_err(got["scale"], is64), tol)]


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16: the generator's kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@rows
def _bf16_trunk_rows():
    out = []
    for n, h, w in ((1, 13, 45), (2, 5, 7)):
        def conv3(rt, n=n, h=h, w=w):
            from upscaler import _engine as E
            L, K = _L(), _K()
            g = _gen("c3", n, h, w)
            x = torch.randn(n, 64, h, w, generator=g) + 0.3
            wk = torch.randn(3, 3, 64, 64, generator=g) * 0.06
            bias = torch.randn(64, generator=g) * 0.7
            wp = _packed(rt, rt.lib.vcg_pack_conv_kernel_bf16, wk, 9 * 64 * 64 * 2, 9, 64, 64, 1, 0)
            d = L.ConvDesc(n, 64, h, w, 64, h, w, 3, 3, 1, 1, 1)
            nrec = rt.lib.vcg_conv2d_bf16_stats_records(ctypes.byref(d), L.STATS_BATCH)
            assert nrec > 0
            ref = K.conv2d(bf(x), bf(wk), bias.double(), 1, "same")

            def call(p, ws, wsn, s):
                ep = L.EpilogueBf16(None, p["bias"], L.ACT_NONE, 0.0, None, None, p["stats"], L.STATS_BATCH)
                rc = rt.lib.vcg_conv2d_bf16_fwd(ctypes.byref(d), p["x"], p["wp"], p["y"], ctypes.byref(ep), s)
                return rc or rt.lib.vcg_norm_finalize_partials(p["stats"], nrec, 1, 64, float(n * h * w), None, None, E.BN_EPS, p["mean"], p["scale"],
                                                               p["shift"], p["invstd"], None, None, 0.99, 0, s)
            o = ((64,), F32)
            return Spec(dict(x=nhwc_bf16(x), wp=wp, bias=bias), dict(y=((n, h, w, 64), BF16), stats=((nrec * 2 * 64,), F32), mean=o, scale=o, shift=o, invstd=o),
                        call, [("y", ref_nhwc(ref), "bf16", 0), lambda got: _partials_check(got, "y", nrec, 1, 64, False, E.BN_EPS)],
                        note="records %d" % nrec)

        def conv5(rt, n=n, h=h, w=w):
            L, K = _L(), _K()
            g = _gen("c5", n, h, w)
            x = torch.randn(n, 64, h, w, generator=g)
            wk = torch.randn(5, 5, 64, 64, generator=g) * 0.04
            scale, shift = torch.rand(64, generator=g) + 0.5, torch.rand(64, generator=g) - 0.5
            res = torch.randn(n, 64, h, w, generator=g)
            nb = rt.lib.vcg_conv_frag_bf16_bytes(25, 64, 64)
            wp = _packed(rt, rt.lib.vcg_pack_conv_frag_bf16, wk, nb, 25, 64, 64, 0)
            d = L.ConvDesc(n, 64, h, w, 64, h, w, 5, 5, 1, 2, 2)
            ref = K.conv2d(bf(x), bf(wk), None, 1, "same") * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1) + bf(res)

            def call(p, ws, wsn, s):
                ep = L.EpilogueBf16(p["scale"], p["shift"], L.ACT_NONE, 0.2, None, p["res"], None, L.STATS_NONE)
                return rt.lib.vcg_conv2d_bf16_fwd(ctypes.byref(d), p["x"], p["wp"], p["y"], ctypes.byref(ep), s)
            return Spec(dict(x=nhwc_bf16(x), wp=wp, scale=scale, shift=shift, res=nhwc_bf16(res)), dict(y=((n, h, w, 64), BF16)), call,
                        [("y", ref_nhwc(ref), "bf16", 0)])
        out += [("vcg_conv2d_bf16_fwd-3x3-batchstats-%dx%dx%d" % (n, h, w), conv3), ("vcg_conv2d_bf16_fwd-5x5-affine-res-%dx%dx%d" % (n, h, w), conv5)]

    def convt(rt):
        L, K = _L(), _K()
        n, h, w, cout = 1, 7, 9, 256
        g = _gen("ct")
        x = torch.randn(n, 64, h, w, generator=g)
        wk = torch.randn(3, 3, cout, 64, generator=g) * 0.06
        bias = torch.randn(cout, generator=g) * 0.3
        wp = _packed(rt, rt.lib.vcg_pack_conv_kernel_bf16, wk, 9 * cout * 64 * 2, 9, cout, 64, 0, 0)
        d = L.ConvDesc(n, 64, h, w, cout, 2 * h, 2 * w, 3, 3, 2, 0, 0)
        ref = lrelu(K.conv2d_transpose_same(bf(x), bf(wk), bias.double(), 2), 0.2)

        def call(p, ws, wsn, s):
            ep = L.EpilogueBf16(None, p["bias"], L.ACT_LRELU, 0.2, None, None, None, L.STATS_NONE)
            return rt.lib.vcg_conv_transpose2d_bf16_fwd(ctypes.byref(d), p["x"], p["wp"], p["y"], ctypes.byref(ep), s)
        return Spec(dict(x=nhwc_bf16(x), wp=wp, bias=bias), dict(y=((n, 2 * h, 2 * w, cout), BF16)), call, [("y", ref_nhwc(ref), "bf16", 0)])

    def wgrad3(rt):
        L, K = _L(), _K()
        n, h, w = 1, 13, 45
        g = _gen("wg3")
        x, dy = torch.randn(n, 64, h, w, generator=g), torch.randn(n, 64, h, w, generator=g)
        wk = torch.zeros(3, 3, 64, 64, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(64, dtype=torch.float64, requires_grad=True)
        gw, gb = torch.autograd.grad((K.conv2d(bf(x), wk, b, 1, "same") * bf(dy)).sum(), [wk, b])
        d = L.ConvDesc(n, 64, h, w, 64, h, w, 3, 3, 1, 1, 1)

        def call(p, ws, wsn, s):
            return rt.lib.vcg_conv2d_bf16_wgrad(ctypes.byref(d), p["x"], p["dy"], p["dw"], p["db"], ws, wsn, s)
        return Spec(dict(x=nhwc_bf16(x), dy=nhwc_bf16(dy)), dict(dw=((3, 3, 64, 64), F32), db=((64,), F32)), call,
                    [("dw", gw, "max", 1e-4), ("db", gb, "max", 1e-4)], ws=rt.lib.vcg_conv2d_bf16_wgrad_workspace_bytes(ctypes.byref(d)))
    out += [("vcg_conv_transpose2d_bf16_fwd-cout256-1x7x9", convt), ("vcg_conv2d_bf16_wgrad-1x13x45", wgrad3)]
    return out


@rows
def _bf16_final9x9_rows():
    N, H, W = 2, 37, 70

    @functools.lru_cache(maxsize=None)
    def data():
        K = _K()
        g = _gen("f9")
        x = torch.randn(N, 256, H, W, generator=g)
        wk = torch.randn(9, 9, 256, 3, generator=g) * 0.01
        b = torch.randn(3, generator=g) * 0.1
        dy = torch.randn(N, 3, H, W, generator=g)
        yprev = torch.randn(N, 256, H, W, generator=g)
        xr = bf(x).requires_grad_(True)
        wr = torch.zeros(9, 9, 256, 3, dtype=torch.float64, requires_grad=True)
        y = torch.tanh(K.conv2d(bf(x), bf(wk), b.double(), 1, "same"))
        (gx,) = torch.autograd.grad((K.conv2d(xr, bf(wk), None, 1, "same") * bf(dy)).sum(), [xr])
        (gw,) = torch.autograd.grad((K.conv2d(bf(x), wr, None, 1, "same") * bf(dy)).sum(), [wr])
        return dict(x=x, w=wk, b=b, dy=dy, yprev=yprev, y=y, gx=gx * torch.where(bf(yprev) > 0, 1.0, 0.2), gw=gw)

    def desc():
        return _L().ConvDesc(N, 256, H, W, 3, H, W, 9, 9, 1, 4, 4)

    def fwd(rt):
        L, D = _L(), data()
        d = desc()
        wf = _packed(rt, rt.lib.vcg_pack_final9x9_bf16, D["w"], L.FINAL9X9_WFRAG_BYTES)
        return Spec(dict(x=nhwc_bf16(D["x"]), wf=wf, b=D["b"]), dict(y=((N, 3, H, W), F32)),
                    lambda p, ws, wsn, s: rt.lib.vcg_conv9x9_to3_bf16_fwd(ctypes.byref(d), p["x"], p["wf"], p["b"], 1, p["y"], s), [("y", D["y"], "max", 1e-4)])

    def dgrad(chsum):
        def build(rt):
            L, D = _L(), data()
            d = desc()
            wd = _packed(rt, rt.lib.vcg_pack_conv9x9_3ch_bf16, D["w"], 4 * L.FIRST9X9_WFRAG_BYTES, 256, 1)
            ins = dict(dy=D["dy"], wd=wd, yprev=nhwc_bf16(D["yprev"]))
            outs = dict(dx=((N, H, W, 256), BF16))
            checks = [("dx", ref_nhwc(D["gx"]), "bf16", 0)]
            if not chsum:
                return Spec(ins, outs, lambda p, ws, wsn, s: rt.lib.vcg_conv9x9_to3_bf16_dgrad(ctypes.byref(d), p["dy"], p["wd"], p["yprev"], 0.2, p["dx"], s),
                            checks)
            nrec = rt.lib.vcg_conv9x9_to3_bf16_dgrad_chsum_records(ctypes.byref(d))
            assert nrec > 0
            outs.update(rec=((nrec, 256), F32), dsum=((256,), F32))

            def call(p, ws, wsn, s):
                rc = rt.lib.vcg_conv9x9_to3_bf16_dgrad_chsum(ctypes.byref(d), p["dy"], p["wd"], p["yprev"], 0.2, p["dx"], p["rec"], s)
                return rc or rt.lib.vcg_sum_records(p["rec"], nrec, 256, 1.0, p["dsum"], s)
            # per-channel sums of the STORED dx (include/vcg.h): the fp64 sum of the bf16 tensor the kernel wrote; dx itself is pinned above
            checks.append(lambda got: [("dsum vs stored dx", _max_err(got["dsum"], got["dx"].double().sum((0, 1, 2))), 1e-5)])
            return Spec(ins, outs, call, checks, note="records %d" % nrec)
        return build

    def wgrad(rt):
        D = data()
        d = desc()
        return Spec(dict(x=nhwc_bf16(D["x"]), dz=D["dy"]), dict(dw=((9, 9, 256, 3), F32)),
                    lambda p, ws, wsn, s: rt.lib.vcg_conv9x9_to3_bf16_wgrad(ctypes.byref(d), p["x"], p["dz"], p["dw"], ws, wsn, s),
                    [("dw", D["gw"], "max", 1e-5)], ws=rt.lib.vcg_conv9x9_to3_bf16_wgrad_workspace_bytes(ctypes.byref(d)))
    return [("vcg_conv9x9_to3_bf16_fwd-2x37x70", fwd), ("vcg_conv9x9_to3_bf16_dgrad-mask-2x37x70", dgrad(False)),
            ("vcg_conv9x9_to3_bf16_dgrad_chsum-2x37x70", dgrad(True)), ("vcg_conv9x9_to3_bf16_wgrad-2x37x70", wgrad)]


@rows
def _bf16_first9x9_rows():
    def build(train):
        def b(rt):
            L, K = _L(), _K()
            n, h, w = 1, 13, 45
            g = _gen("i9")
            x = torch.rand(n, 3, h, w, generator=g) * 2 - 1
            wk = torch.randn(9, 9, 3, 64, generator=g) * 0.1
            bias, al = torch.randn(64, generator=g) * 0.2, torch.rand(64, generator=g) * 0.5
            wf = _packed(rt, rt.lib.vcg_pack_first9x9_bf16, wk, L.FIRST9X9_WFRAG_BYTES)
            d = L.ConvDesc(n, 3, h, w, 64, h, w, 9, 9, 1, 4, 4)
            z = K.conv2d(bf(x), bf(wk), bias.double(), 1, "same")
            ins = dict(x=x, wf=wf, bias=bias, al=al)
            o = ((n, h, w, 64), BF16)
            if train:
                return Spec(ins, dict(y=o, z=o), lambda p, ws, wsn, s: rt.lib.vcg_conv9x9_from3_bf16_fwd_train(ctypes.byref(d), p["x"], p["wf"], p["bias"], p["al"],
                                                                                                               p["y"], p["z"], s),
                            [("y", ref_nhwc(prelu(z, al.double())), "bf16", 0), ("z", ref_nhwc(z), "bf16", 0)])
            return Spec(ins, dict(y=o), lambda p, ws, wsn, s: rt.lib.vcg_conv9x9_from3_bf16_fwd(ctypes.byref(d), p["x"], p["wf"], p["bias"], p["al"], p["y"], s),
                        [("y", ref_nhwc(prelu(z, al.double())), "bf16", 0)])
        return b

    def prelu_bwd(to_bf16, with_d2):
        def b(rt):
            n, c, hw = 2, 64, 13 * 45
            g = _gen("pb", with_d2)
            d1, d2, z = (torch.randn(n, hw, c, generator=g).to(BF16) for _ in range(3))
            alpha = torch.rand(c, generator=g) * 0.4 + 0.05
            nrec = rt.lib.vcg_prelu_bwd_nhwc_bf16_records(n, hw)
            assert nrec > 0
            dsum = d1.double() + (d2.double() if with_d2 else 0.0)
            dz = dsum * torch.where(z.double() >= 0, torch.ones(1, dtype=torch.float64), alpha.double().view(1, 1, c))
            dal = (dsum * torch.clamp(z.double(), max=0)).sum((0, 1))
            fn = rt.lib.vcg_prelu_bwd_nhwc_bf16_to_bf16 if to_bf16 else rt.lib.vcg_prelu_bwd_nhwc_bf16

            def call(p, ws, wsn, s):
                rc = fn(p["d1"], p["d2"] if with_d2 else None, p["z"], p["alpha"], n, c, hw, p["dz"], p["rec"], s)
                return rc or rt.lib.vcg_sum_records(p["rec"], nrec, c, 1.0, p["dalpha"], s)
            ins = dict(d1=d1, z=z, alpha=alpha)
            if with_d2:
                ins["d2"] = d2
            if to_bf16:
                o, chk = ((n, hw, c), BF16), ("dz", dz, "bf16", 0)
            else:           # fp32 NCHW: one fp32 rounding of (d1 + d2) and one of the product
                o, chk = ((n, c, hw), F32), ("dz", dz.permute(0, 2, 1).contiguous(), "elem", 1e-5)
            return Spec(ins, dict(dz=o, rec=((nrec, c), F32), dalpha=((c,), F32)), call, [chk, ("dalpha", dal, "max", 1e-5)], note="records %d" % nrec)
        return b
    out = [("vcg_conv9x9_from3_bf16_fwd-1x13x45", build(False)), ("vcg_conv9x9_from3_bf16_fwd_train-1x13x45", build(True))]
    for to_bf16 in (False, True):
        for with_d2 in (True, False):
            out.append(("vcg_prelu_bwd_nhwc_bf16%s-%s-2x64x585" % ("_to_bf16" if to_bf16 else "", "d2" if with_d2 else "nod2"), prelu_bwd(to_bf16, with_d2)))
    return out


@rows
def _bf16_norm_rows():
    n, c, h, w = 2, 64, 30, 33

    @functools.lru_cache(maxsize=None)
    def data():
        from upscaler import _engine as E
        g = _gen("nb")
        x = torch.randn(n, c, h, w, generator=g) * 1.5 + torch.randn(1, c, 1, 1, generator=g)
        dy, res = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g)
        xb = bf(x).requires_grad_(True)
        mu, var = xb.mean((2, 3), keepdim=True), xb.var((2, 3), unbiased=False, keepdim=True)
        xh = (xb - mu) / torch.sqrt(var + E.IN_EPS)
        (gx,) = torch.autograd.grad((xh * bf(dy)).sum(), [xb])
        return dict(x=x, dy=dy, res=res, mean=mu.detach().reshape(-1), var=var.detach().reshape(-1), xh=xh.detach(), gx=gx, eps=E.IN_EPS)

    def stats(rt):
        L, D = _L(), data()
        o = ((n * c,), F32)
        return Spec(dict(x=nhwc_bf16(D["x"])), dict(mean=o, var=o),
                    lambda p, ws, wsn, s: rt.lib.vcg_norm_stats_bf16(p["x"], n, c, h * w, L.NORM_INSTANCE, p["mean"], p["var"], ws, wsn, s),
                    [("mean", D["mean"], "max", 1e-5), ("var", D["var"], "max", 1e-4)],
                    ws=rt.lib.vcg_norm_stats_bf16_workspace_bytes(n, c, h * w, L.NORM_INSTANCE))

    def fwd(rt):
        L, D = _L(), data()
        is64 = 1.0 / torch.sqrt(D["var"] + D["eps"])
        scale, shift = is64.float(), (-D["mean"] * is64).float()
        ref = bf(D["x"]) * scale.double().view(n, c, 1, 1) + shift.double().view(n, c, 1, 1) + bf(D["res"])
        return Spec(dict(x=nhwc_bf16(D["x"]), scale=scale, shift=shift, res=nhwc_bf16(D["res"])), dict(y=((n, h, w, c), BF16)),
                    lambda p, ws, wsn, s: rt.lib.vcg_norm_act_fwd_bf16(p["x"], n, c, h * w, p["scale"], p["shift"], 1, L.ACT_NONE, 0.2, None, p["res"], p["y"], s),
                    [("y", ref_nhwc(ref), "bf16", 0)])

    def bwd(rt):
        L, D = _L(), data()
        invstd = (1.0 / torch.sqrt(D["var"] + D["eps"])).float()

        def call(p, ws, wsn, s):
            return rt.lib.vcg_norm_act_bwd_bf16(p["x"], p["dy"], n, c, h * w, L.NORM_INSTANCE, p["mean"], p["invstd"], None, None, L.ACT_NONE, 0.2, None, 1,
                                                p["dx"], None, None, None, ws, wsn, s)
        return Spec(dict(x=nhwc_bf16(D["x"]), dy=nhwc_bf16(D["dy"]), mean=D["mean"].float(), invstd=invstd), dict(dx=((n, h, w, c), BF16)), call,
                    [("dx", ref_nhwc(D["gx"]), "max", TOL_BF16)], ws=rt.lib.vcg_norm_act_bwd_bf16_workspace_bytes(n, c, h * w, L.NORM_INSTANCE))
    tag = "instance-2x64x30x33"
    return [("vcg_norm_stats_bf16-" + tag, stats), ("vcg_norm_act_fwd_bf16-" + tag, fwd), ("vcg_norm_act_bwd_bf16-" + tag, bwd)]


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16: the critics' kernels
# ---------------------------------------------------------------------------------------------------------------------------------
CONV3CH = [(64, 3, 1, "same", None, 2, 40, 72), (64, 4, 2, 1, 0.2, 1, 70, 54)]


@rows
def _bf16_conv3ch_rows():
    out = []

    @functools.lru_cache(maxsize=None)
    def data(case):
        K = _K()
        cout, k, stride, padding, slope, n, h, w = case
        g = _gen("c3ch", k, h)
        wk = torch.randn(k, k, 3, cout, generator=g) * (2.0 / (k * k * 3)) ** 0.5
        bk = torch.randn(cout, generator=g) * 0.1
        x = torch.randint(0, 256, (n, 3, h, w), generator=g).float() / 127.5 - 1
        z = K.conv2d(bf(x), bf(wk), bk.double(), stride, padding)
        y = lrelu(z, slope) if slope else z
        dz = torch.randn(*z.shape, generator=g).to(BF16).float()
        xg, wg, bg = bf(x).requires_grad_(True), wk.double().requires_grad_(True), bk.double().requires_grad_(True)
        gw, gb = torch.autograd.grad((K.conv2d(xg, wg, bg, stride, padding) * dz.double()).sum(), [wg, bg])
        xr = x.double().requires_grad_(True)
        (gx,) = torch.autograd.grad((K.conv2d(xr, bf(wk), bk.double(), stride, padding) * dz.double()).sum(), [xr])
        return dict(x=x, w=wk, b=bk, y=y, dz=dz, gw=gw, gb=gb, gx=gx)

    for case in CONV3CH:
        cout, k, stride, padding, slope, n, h, w = case
        tag = _tag("k%d" % k, "s%d" % stride, n, h, w)

        def fwd(rt, case=case):
            D = data(case)
            cout, k, stride, padding, slope, n, h, w = case
            d = conv_desc(3, cout, k, stride, padding, n, h, w)
            nb = rt.lib.vcg_conv3ch_bf16_wfrag_bytes(k, k, cout)
            wf = _packed(rt, rt.lib.vcg_pack_conv3ch_bf16, D["w"], nb, k, k, cout)
            return Spec(dict(x=D["x"], wf=wf, b=D["b"]), dict(y=((n, d.oh, d.ow, cout), BF16)),
                        lambda p, ws, wsn, s: rt.lib.vcg_conv3ch_bf16_fwd(ctypes.byref(d), p["x"], p["wf"], p["b"], float(slope) if slope else 1.0, p["y"], s),
                        [("y", ref_nhwc(D["y"]), "bf16", 0)])

        def dgrad(rt, case=case):
            D = data(case)
            cout, k, stride, padding, slope, n, h, w = case
            d = conv_desc(3, cout, k, stride, padding, n, h, w)
            return Spec(dict(dz=nhwc_bf16(D["dz"]), w=D["w"]), dict(dx=((n, 3, h, w), F32)),
                        lambda p, ws, wsn, s: rt.lib.vcg_conv3ch_bf16_dgrad(ctypes.byref(d), p["dz"], p["w"], p["dx"], ws, wsn, s),
                        [("dx", D["gx"], "max", TOL_BF16)], ws=rt.lib.vcg_conv3ch_bf16_dgrad_workspace_bytes(ctypes.byref(d)))

        def wgrad(rt, case=case):
            D = data(case)
            cout, k, stride, padding, slope, n, h, w = case
            d = conv_desc(3, cout, k, stride, padding, n, h, w)
            need = rt.lib.vcg_conv3ch_bf16_wgrad_workspace_bytes(ctypes.byref(d))
            assert need > 0, "even widths are served by the bf16 weight gradient"
            return Spec(dict(x=D["x"], dz=nhwc_bf16(D["dz"])), dict(dw=((k, k, 3, cout), F32), db=((cout,), F32)),
                        lambda p, ws, wsn, s: rt.lib.vcg_conv3ch_bf16_wgrad(ctypes.byref(d), p["x"], p["dz"], p["dw"], p["db"], ws, wsn, s),
                        [("dw", D["gw"], "max", 1e-5), ("db", D["gb"], "max", 1e-5)], ws=need)
        out += [("vcg_conv3ch_bf16_fwd-" + tag, fwd), ("vcg_conv3ch_bf16_dgrad-" + tag, dgrad), ("vcg_conv3ch_bf16_wgrad-" + tag, wgrad)]
    return out


GCONV = [(256, 512, 4, 1, 1, 1, 10, 10), (128, 128, 3, 2, "same", 1, 15, 17)]
GSTAT = (128, 128, 3, 1, "same", 5, 67, 45, False)


@functools.lru_cache(maxsize=None)
def _gconv_data(case):
    K = _K()
    cin, cout, k, stride, padding, n, h, w = case
    g = _gen("gconv", cin, cout, k, h)
    wk = torch.randn(k, k, cin, cout, generator=g) * (2.0 / (k * k * cin)) ** 0.5
    bk = torch.randn(cout, generator=g) * 0.1
    x = torch.randn(n, cin, h, w, generator=g)
    xr, wr, br = bf(x).requires_grad_(True), bf(wk).requires_grad_(True), bk.double().requires_grad_(True)
    y = K.conv2d(xr, wr, br, stride, padding)
    dy = torch.randn(*y.shape, generator=g)
    mask = torch.randn(n, cin, h, w, generator=g)
    gx, gw, gb = torch.autograd.grad((y * bf(dy)).sum(), [xr, wr, br])
    return dict(x=x, w=wk, b=bk, dy=dy, mask=mask, y=y.detach(), gx=gx * torch.where(bf(mask) > 0, 1.0, 0.2), gw=gw, gb=gb)


@rows
def _bf16_generic_rows():
    out = []
    for case in GCONV:
        cin, cout, k, stride, padding, n, h, w = case
        tag = _tag(*case)

        def fwd(rt, case=case):
            L, D = _L(), _gconv_data(case)
            cin, cout, k, stride, padding, n, h, w = case
            d = conv_desc(*case)
            nb = rt.lib.vcg_conv_frag_bf16_bytes(k * k, cout, cin)
            wf = _packed(rt, rt.lib.vcg_pack_conv_frag_bf16, D["w"], nb, k * k, cout, cin, 0)
            return Spec(dict(x=nhwc_bf16(D["x"]), wf=wf, b=D["b"]), dict(y=((n, d.oh, d.ow, cout), BF16)),
                        lambda p, ws, wsn, s: rt.lib.vcg_conv2d_nhwc_bf16_fwd(ctypes.byref(d), p["x"], p["wf"], p["b"], L.ACT_LRELU, 0.2, p["y"], s),
                        [("y", ref_nhwc(lrelu(D["y"], 0.2)), "bf16", 0)])

        def dgrad(rt, case=case):
            D = _gconv_data(case)
            cin, cout, k, stride, padding, n, h, w = case
            d = conv_desc(*case)
            nb = rt.lib.vcg_conv_frag_bf16_bytes(k * k, cin, cout)
            wd = _packed(rt, rt.lib.vcg_pack_conv_frag_bf16, D["w"], nb, k * k, cin, cout, 1)
            return Spec(dict(dy=nhwc_bf16(D["dy"]), wd=wd, mask=nhwc_bf16(D["mask"])), dict(dx=((n, h, w, cin), BF16)),
                        lambda p, ws, wsn, s: rt.lib.vcg_conv2d_nhwc_bf16_dgrad(ctypes.byref(d), p["dy"], p["wd"], p["mask"], 0.2, p["dx"], s),
                        [("dx", ref_nhwc(D["gx"]), "max", TOL_BF16)])

        def wgrad(rt, case=case):
            D = _gconv_data(case)
            cin, cout, k, stride, padding, n, h, w = case
            d = conv_desc(*case)
            return Spec(dict(x=nhwc_bf16(D["x"]), dy=nhwc_bf16(D["dy"])), dict(dw=((k, k, cin, cout), F32), db=((cout,), F32)),
                        lambda p, ws, wsn, s: rt.lib.vcg_conv2d_nhwc_bf16_wgrad(ctypes.byref(d), p["x"], p["dy"], p["dw"], p["db"], ws, wsn, s),
                        [("dw", D["gw"], "max", 1e-4), ("db", D["gb"], "max", 1e-4)], ws=rt.lib.vcg_conv2d_nhwc_bf16_wgrad_workspace_bytes(ctypes.byref(d)))
        out += [("vcg_conv2d_nhwc_bf16_fwd-" + tag, fwd), ("vcg_conv2d_nhwc_bf16_dgrad-mask-" + tag, dgrad), ("vcg_conv2d_nhwc_bf16_wgrad-" + tag, wgrad)]

    def fwd_stats(rt):
        from upscaler import _engine as E
        L, K = _L(), _K()
        cin, cout, k, stride, padding, n, h, w, inst = GSTAT
        g = _gen("gstat")
        wk = torch.randn(k, k, cin, cout, generator=g) * (2.0 / (k * k * cin)) ** 0.5
        bk = torch.randn(cout, generator=g) * 0.5
        x = torch.randn(n, cin, h, w, generator=g)
        d = conv_desc(*GSTAT[:8])
        per_image = rt.lib.vcg_conv2d_nhwc_bf16_stats_records(ctypes.byref(d), L.STATS_INSTANCE)
        nrec = rt.lib.vcg_conv2d_nhwc_bf16_stats_records(ctypes.byref(d), L.STATS_BATCH)
        assert per_image > 0 and nrec == n * per_image
        nb = rt.lib.vcg_conv_frag_bf16_bytes(k * k, cout, cin)
        wf = _packed(rt, rt.lib.vcg_pack_conv_frag_bf16, wk, nb, k * k, cout, cin, 0)
        ref = K.conv2d(bf(x), bf(wk), bk.double(), stride, padding)

        def call(p, ws, wsn, s):
            rc = rt.lib.vcg_conv2d_nhwc_bf16_fwd_stats(ctypes.byref(d), p["x"], p["wf"], p["b"], p["y"], p["stats"], s)
            return rc or rt.lib.vcg_norm_finalize_partials(p["stats"], nrec, 1, cout, float(n * d.oh * d.ow), None, None, E.BN_EPS, p["mean"], p["scale"],
                                                           p["shift"], p["invstd"], None, None, 0.99, 0, s)
        o = ((cout,), F32)
        return Spec(dict(x=nhwc_bf16(x), wf=wf, b=bk), dict(y=((n, d.oh, d.ow, cout), BF16), stats=((n * per_image * 2 * cout,), F32), mean=o, scale=o,
                                                             shift=o, invstd=o), call,
                    [("y", ref_nhwc(ref), "bf16", 0), lambda got: _partials_check(got, "y", nrec, 1, cout, False, E.BN_EPS)], note="records %d" % nrec)
    out.append(("vcg_conv2d_nhwc_bf16_fwd_stats-" + _tag(*GSTAT), fwd_stats))

    def _ct_case(rt):
        """(k, cin, cout, n, h, w): the listed (5, 256, 1, 5, 7) where the weight gradient serves it, else the 3x3 64 -> 256 layer of the k3 generator"""
        L = _L()
        for k, cin in ((5, 256), (3, 64)):
            crop = (k - 2) // 2
            d = L.ConvDesc(1, cin, 5, 7, 256, 10, 14, k, k, 2, crop, crop)
            if rt.lib.vcg_conv_transpose2d_nhwc_bf16_wgrad_workspace_bytes(ctypes.byref(d)) > 0:
                return k, cin, d
        raise AssertionError("vcg_conv_transpose2d_nhwc_bf16_wgrad serves neither shape")

    def ct_data(k, cin):
        K = _K()
        g = _gen("gct", k, cin)
        x = torch.randn(1, cin, 5, 7, generator=g)
        wk = torch.randn(k, k, 256, cin, generator=g) * (0.5 / (k * (cin ** 0.5)))
        bias = torch.randn(256, generator=g) * 0.3
        dz = torch.randn(1, 256, 10, 14, generator=g)
        wr = bf(wk).requires_grad_(True)
        z = K.conv2d_transpose_same(bf(x), wr, bias.double(), 2)
        (gw,) = torch.autograd.grad((z * bf(dz)).sum(), [wr])
        return x, wk, bias, dz, z.detach(), gw

    def ct_fwd(rt):
        L = _L()
        k, cin = 5, 256
        x, wk, bias, dz, z, gw = ct_data(k, cin)
        d = L.ConvDesc(1, cin, 5, 7, 256, 10, 14, k, k, 2, 1, 1)
        nb = rt.lib.vcg_conv_frag_bf16_bytes(k * k, 256, cin)
        wf = _packed(rt, rt.lib.vcg_pack_conv_frag_bf16, wk, nb, k * k, 256, cin, 1)
        return Spec(dict(x=nhwc_bf16(x), wf=wf, b=bias), dict(y=((1, 10, 14, 256), BF16)),
                    lambda p, ws, wsn, s: rt.lib.vcg_conv_transpose2d_nhwc_bf16_fwd(ctypes.byref(d), p["x"], p["wf"], p["b"], L.ACT_LRELU, 0.2, p["y"], s),
                    [("y", ref_nhwc(lrelu(z, 0.2)), "bf16", 0)])

    def ct_wgrad(rt):
        k, cin, d = _ct_case(rt)
        x, wk, bias, dz, z, gw = ct_data(k, cin)
        return Spec(dict(x=nhwc_bf16(x), dz=nhwc_bf16(dz)), dict(dw=((k, k, 256, cin), F32)),
                    lambda p, ws, wsn, s: rt.lib.vcg_conv_transpose2d_nhwc_bf16_wgrad(ctypes.byref(d), p["x"], p["dz"], p["dw"], ws, wsn, s),
                    [("dw", gw, "max", 1e-4)], ws=rt.lib.vcg_conv_transpose2d_nhwc_bf16_wgrad_workspace_bytes(ctypes.byref(d)),
                    note="k=%d cin=%d" % (k, cin))
    out += [("vcg_conv_transpose2d_nhwc_bf16_fwd-5x256x1x5x7", ct_fwd), ("vcg_conv_transpose2d_nhwc_bf16_wgrad-1x5x7", ct_wgrad)]
    return out


@rows
def _bf16_cout1_rows():
    case = (256, 4, 1, 2, 9, 11)

    @functools.lru_cache(maxsize=None)
    def data():
        K = _K()
        cin, k, padding, n, h, w = case
        g = _gen("cout1")
        wk = torch.randn(k, k, cin, 1, generator=g) * (2.0 / (k * k * cin)) ** 0.5
        bk = torch.randn(1, generator=g) * 0.1
        x = torch.randn(n, cin, h, w, generator=g)
        xr, wr, br = bf(x).requires_grad_(True), wk.double().requires_grad_(True), bk.double().requires_grad_(True)
        y = K.conv2d(xr, wr, br, 1, padding)
        dy = torch.randn(*y.shape, generator=g)
        gx, gw, gb = torch.autograd.grad((y * dy.double()).sum(), [xr, wr, br])
        return dict(x=x, w=wk, b=bk, dy=dy, y=y.detach(), gx=gx, gw=gw, gb=gb)
    cin, k, padding, n, h, w = case

    def desc():
        return conv_desc(cin, 1, k, 1, padding, n, h, w)

    def fwd(rt):
        D, d = data(), desc()
        return Spec(dict(x=nhwc_bf16(D["x"]), w=D["w"], b=D["b"]), dict(y=(D["y"].shape, F32)),
                    lambda p, ws, wsn, s: rt.lib.vcg_conv2d_cout1_nhwc_bf16_fwd(ctypes.byref(d), p["x"], p["w"], p["b"], p["y"], s), [("y", D["y"], "max", 1e-5)])

    def dgrad(rt):
        D, d = data(), desc()
        return Spec(dict(dy=D["dy"], w=D["w"]), dict(dx=((n, h, w, cin), BF16)),
                    lambda p, ws, wsn, s: rt.lib.vcg_conv2d_cout1_nhwc_bf16_dgrad(ctypes.byref(d), p["dy"], p["w"], p["dx"], s),
                    [("dx", ref_nhwc(D["gx"]), "max", TOL_BF16)])

    def wgrad(rt):
        D, d = data(), desc()
        return Spec(dict(x=nhwc_bf16(D["x"]), dy=D["dy"]), dict(dw=((k, k, cin, 1), F32), db=((1,), F32)),
                    lambda p, ws, wsn, s: rt.lib.vcg_conv2d_cout1_nhwc_bf16_wgrad(ctypes.byref(d), p["x"], p["dy"], p["dw"], p["db"], ws, wsn, s),
                    [("dw", D["gw"], "max", 1e-5), ("db", D["gb"], "max", 1e-5)], ws=rt.lib.vcg_conv2d_cout1_nhwc_bf16_wgrad_workspace_bytes(ctypes.byref(d)))
    tag = _tag(*case)
    return [("vcg_conv2d_cout1_nhwc_bf16_fwd-" + tag, fwd), ("vcg_conv2d_cout1_nhwc_bf16_dgrad-" + tag, dgrad), ("vcg_conv2d_cout1_nhwc_bf16_wgrad-" + tag, wgrad)]


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,build", ROWS, ids=[r[0] for r in ROWS])
def test_abi_memory_contract(rt, name, build):
    run_spec(rt, name, build(rt))


def test_harness_catches_a_write_one_element_past_the_payload(rt):
    """vcg_fill of numel + 1 elements into an output arena: the extra element lands in the arena's own back guard"""
    numel = 1001
    a = A.output_arena((numel,), F32, rt.device)
    assert rt.lib.vcg_fill(a.ptr, numel, 2.0, rt.stream) == OK
    a.check()
    assert bool((a.view(F32) == 2.0).all())
    assert rt.lib.vcg_fill(a.ptr, numel + 1, 3.0, rt.stream) == OK
    with pytest.raises(A.GuardError) as e:
        a.check()
    assert "back guard" in str(e.value) and "offsets %d .. %d" % (4 * numel, 4 * numel + 3) in str(e.value)

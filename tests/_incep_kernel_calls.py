"""One inception block of make_upscaler_incep_resnet on the device, launch by launch, for the kernel and memory-contract tests
(tests/test_incep_kernels_bf16_gpu.py, tests/test_abi_incep_contract_gpu.py): random block parameters that exercise both PReLU branches,
every operand inside a guarded arena (tests/_arena.py) of exactly its stated / queried size, outputs pre-filled with NaN bytes, and each
launch's fp64 reference from tests/_incep_bf16_emulation.py applied to the DEVICE'S OWN stored input."""
import ctypes

import torch

import _arena as A
import _incep_bf16_emulation as EM

OK = 0
EPS = 1e-3
TOL_BF16 = 2.0 ** -8


def pad32(c):
    return (c + 31) // 32 * 32


def block_spec(btype, k):
    """(name, minis = [(mini, cin, cout, kh, kw)], heads, mids, srcs) as the engine plans a block"""
    if btype == "3path":
        n = "inc_res_block/A/3p/0"
        minis = [("a/1", 64, 32, 1, 1), ("b/1", 64, 32, 1, 1), ("b/2", 32, 32, k, k), ("c/1", 64, 32, 1, 1), ("c/2", 32, 48, k, k), ("c/3", 48, 64, k, k)]
        heads = [("a/1", None), ("b/1", "b/2"), ("c/1", "c/2")]
        mids = [("b/2", None, "b/1"), ("c/2", "c/3", "c/1"), ("c/3", None, "c/2")]
        srcs = ["a/1", "b/2", "c/3"]
    else:
        n = "inc_res_block/B/2p/0"
        minis = [("a/1", 64, 32, 1, 1), ("b/1", 64, 19, 1, 1), ("b/2", 19, 25, 1, k), ("b/3", 25, 32, k, 1)]
        heads = [("a/1", None), ("b/1", "b/2")]
        mids = [("b/2", "b/3", "b/1"), ("b/3", None, "b/2")]
        srcs = ["a/1", "b/3"]
    return n, minis, heads, mids, srcs


def block_weights(btype, k, seed):
    """fp32 parameters of one block: BatchNormalization scales of both signs, negative shifts, slopes in 0.05 .. 0.4"""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g) * (hi - lo) + lo
    n, minis, _, _, srcs = block_spec(btype, k)
    w = {}
    for mini, cin, cout, kh, kw in minis:
        p = "%s/%s" % (n, mini)
        sign = torch.where(torch.rand(cin, generator=g) < 0.5, -1.0, 1.0)
        w[p + "/batch_norm/gamma"] = u(0.6, 1.4, cin) * sign
        w[p + "/batch_norm/beta"] = u(-0.6, 0.1, cin)
        w[p + "/batch_norm/moving_mean"] = u(-0.3, 0.3, cin)
        w[p + "/batch_norm/moving_variance"] = u(0.5, 1.5, cin)
        w[p + "/prelu/alpha"] = u(0.05, 0.4, cin)
        w["%s/%dx%d/kernel" % (p, kh, kw)] = torch.randn(kh, kw, cin, cout, generator=g) * (kh * kw * cin) ** -0.5
        w["%s/%dx%d/bias" % (p, kh, kw)] = u(-0.3, 0.3, cout)
    total = sum(c for m_, _, c, _, _ in minis if m_ in srcs)
    w[n + "/final/1x1/kernel"] = torch.randn(1, 1, total, 64, generator=g) * total ** -0.5
    w[n + "/final/1x1/bias"] = u(-0.3, 0.3, 64)
    return w


class Device:
    """the operands of the launches, each in its own arena; check() asserts every guard and that every input still holds its bytes"""
    def __init__(self, rt):
        self.rt, self.inputs, self.outputs = rt, [], []

    def put(self, t, name):
        a = A.input_arena(t, self.rt.device, name=name)
        self.inputs.append((a, t.contiguous().view(-1).view(torch.uint8).clone()))
        return a

    def out(self, shape, dtype, name):
        a = A.output_arena(shape, dtype, self.rt.device, name=name)
        self.outputs.append(a)
        return a

    def check(self):
        torch.cuda.current_stream().synchronize()
        for a in self.outputs:
            a.check()
        for a, raw in self.inputs:
            a.check()
            assert torch.equal(a.payload.cpu(), raw), a.name

    def fold(self, w, c, bias=None, norm=None, prelu=None):
        """vcg_incep_fold into arenas of exactly padded(c) floats -> (scale, shift, alpha or None) arenas"""
        lib, cp = self.rt.lib, pad32(c)
        assert lib.vcg_incep_padded_channels(c) == cp
        p = lambda name: self.put(w[name], name).ptr if name else None
        sc, sh = self.out((cp,), torch.float32, "scale"), self.out((cp,), torch.float32, "shift")
        al = self.out((cp,), torch.float32, "alpha") if prelu else None
        rc = lib.vcg_incep_fold(p(bias and bias + "/bias"), p(norm and norm + "/moving_mean"), p(norm and norm + "/moving_variance"),
                                p(norm and norm + "/gamma"), p(norm and norm + "/beta"), p(prelu and prelu + "/alpha"), c, EPS, sc.ptr, sh.ptr,
                                al.ptr if al else None, self.rt.stream)
        assert rc == OK, rc
        for a in (sc, sh) + ((al,) if al else ()):
            v = a.view(torch.float32).cpu()
            assert not torch.isnan(v).any() and bool((v[c:] == 0).all()), a.name          # zeros in the padding
        return sc, sh, al

    def pack(self, wk, k0=0, kcount=None):
        """vcg_pack_incep_frag_bf16 into an arena of exactly the queried bytes"""
        kh, kw, cin_total, cout = wk.shape
        kcount = cin_total if kcount is None else kcount
        nbytes = self.rt.lib.vcg_incep_frag_bf16_bytes(kh * kw, kcount, cout)
        assert nbytes == kh * kw * pad32(kcount) * pad32(cout) * 2
        pk = self.out((nbytes,), torch.uint8, "wfrag")
        assert self.rt.lib.vcg_pack_incep_frag_bf16(self.put(wk, "kernel").ptr, kh * kw, cin_total, cout, k0, kcount, pk.ptr, self.rt.stream) == OK
        vals = pk.view(torch.bfloat16).float().cpu()
        assert not torch.isnan(vals).any()
        # as many non-zero values as the kernel slice has (a random kernel has no zeros), every other one zero
        assert int((vals != 0).sum()) == int((wk[:, :, k0:k0 + kcount].to(torch.bfloat16) != 0).sum())
        return pk


def to_nhwc_bf16(x_nchw, cp=None):
    """host NCHW float -> bf16 NHWC, channels padded with zeros to cp"""
    n, c, h, w = x_nchw.shape
    y = torch.zeros(n, h, w, cp or c, dtype=torch.bfloat16)
    y[..., :c] = x_nchw.permute(0, 2, 3, 1).to(torch.bfloat16)
    return y


def stored(arena, n, h, w, c):
    """an output arena's bf16 NHWC [n][h][w][padded(c)] tensor as fp64 NCHW of its c channels; asserts exact zeros in the padding and no NaN"""
    t = arena.view(torch.bfloat16, (n, h, w, pad32(c))).float().cpu()
    assert not torch.isnan(t).any(), arena.name
    assert bool((t[..., c:] == 0).all()), "%s: padded channels are not zero" % arena.name
    return t[..., :c].permute(0, 3, 1, 2).double()


def ulp_scaled(got, ref):
    return float(((got - ref).abs() / (ref.abs() * 2.0 ** -8 + 1e-3 * ref.abs().max())).max())


def run_head(dev, w, btype, k, m_arena, n, h, wd):
    """-> {mini: output arena}"""
    from upscaler import _lib as L
    name, minis, heads, _, _ = block_spec(btype, k)
    cout = {m_: c for m_, _, c, _, _ in minis}
    hd = L.IncepHeadDesc(n, h, wd, 64, len(heads))
    paths = (L.IncepHeadPath * len(heads))()
    outs = {}
    for i, (mini, nxt) in enumerate(heads):
        p = "%s/%s" % (name, mini)
        isc, ish, ial = dev.fold(w, 64, norm=p + "/batch_norm", prelu=p + "/prelu")
        q = "%s/%s" % (name, nxt)
        osc, osh, oal = dev.fold(w, cout[mini], bias=p + "/1x1", norm=nxt and q + "/batch_norm", prelu=nxt and q + "/prelu")
        wf = dev.pack(w[p + "/1x1/kernel"])
        outs[mini] = dev.out((n, h, wd, 32), torch.bfloat16, "y " + mini)
        hd.cout[i] = cout[mini]
        paths[i] = L.IncepHeadPath(isc.ptr, ish.ptr, ial.ptr, wf.ptr, osc.ptr, osh.ptr, oal.ptr if oal else None, outs[mini].ptr)
    assert dev.rt.lib.vcg_incep_head_bf16_fwd(ctypes.byref(hd), m_arena.ptr, paths, dev.rt.stream) == OK
    return outs


def run_mid(dev, w, btype, k, mini, x_arena, n, h, wd):
    from upscaler import _lib as L
    name, minis, _, mids, _ = block_spec(btype, k)
    _, cin, cout, kh, kw = [m_ for m_ in minis if m_[0] == mini][0]
    nxt = [m_[1] for m_ in mids if m_[0] == mini][0]
    p, q = "%s/%s/%dx%d" % (name, mini, kh, kw), "%s/%s" % (name, nxt)
    sc, sh, al = dev.fold(w, cout, bias=p, norm=nxt and q + "/batch_norm", prelu=nxt and q + "/prelu")
    wf = dev.pack(w[p + "/kernel"])
    y = dev.out((n, h, wd, pad32(cout)), torch.bfloat16, "y " + mini)
    d = L.ConvDesc(n, cin, h, wd, cout, h, wd, kh, kw, 1, kh // 2, kw // 2)
    ep = L.EpilogueBf16(sc.ptr, sh.ptr, L.ACT_PRELU if al else L.ACT_NONE, 0.0, al.ptr if al else None, None)
    rc = dev.rt.lib.vcg_conv2d_nhwc_bf16_fwd_epilogue(ctypes.byref(d), x_arena.ptr, wf.ptr, y.ptr, ctypes.byref(ep), dev.rt.stream)
    assert rc == OK, rc
    return y, (cin, cout, kh, kw, nxt)


def run_join(dev, w, btype, k, src_arenas, m_arena, n, h, wd):
    from upscaler import _lib as L
    name, minis, _, _, srcs = block_spec(btype, k)
    cout = {m_: c for m_, _, c, _, _ in minis}
    jd = L.IncepJoinDesc(n, h, wd, 64, len(srcs))
    wk, k0, wfs = w[name + "/final/1x1/kernel"], 0, []
    for i, s in enumerate(srcs):
        jd.cin[i] = cout[s]
        wfs.append(dev.pack(wk, k0, cout[s]))
        k0 += cout[s]
    z = (ctypes.c_void_p * len(srcs))(*[a.ptr for a in src_arenas])
    wf = (ctypes.c_void_p * len(srcs))(*[a.ptr for a in wfs])
    y = dev.out((n, h, wd, 64), torch.bfloat16, "y join")
    bias = dev.put(w[name + "/final/1x1/bias"], "join bias")
    assert dev.rt.lib.vcg_incep_join_bf16_fwd(ctypes.byref(jd), z, wf, bias.ptr, m_arena.ptr, y.ptr, dev.rt.stream) == OK
    return y


def run_block(rt, btype, k, n, h, wd, seed=0):
    """one block, launch by launch: -> [(what, got fp64 NCHW, teacher-forced fp64 reference)] and the Device (for its arenas)"""
    w = block_weights(btype, k, 1000 * k + seed + (7 if btype == "3path" else 0))
    w64 = {kk: v.double() for kk, v in w.items()}
    name, minis, heads, mids, srcs = block_spec(btype, k)
    cout = {m_: c for m_, _, c, _, _ in minis}
    g = torch.Generator().manual_seed(n * 10000 + h * 100 + wd)
    m = torch.randn(n, 64, h, wd, generator=g)
    dev = Device(rt)
    mb = to_nhwc_bf16(m)
    m_arena = dev.put(mb, "m")
    m64 = mb.float().permute(0, 3, 1, 2).double()
    res, arena, val = [], {}, {}
    with torch.no_grad():
        arena.update(run_head(dev, w, btype, k, m_arena, n, h, wd))
        for mini, nxt in heads:
            val[mini] = stored(arena[mini], n, h, wd, cout[mini])
            res.append(("head " + mini, val[mini], EM.f_head(w64, name, mini, nxt, m64)))
        for mini, nxt, src in mids:
            arena[mini], (cin, co, kh, kw, _) = run_mid(dev, w, btype, k, mini, arena[src], n, h, wd)
            val[mini] = stored(arena[mini], n, h, wd, co)
            res.append(("mid %s %dx%d %d->%d" % (mini, kh, kw, cin, co), val[mini], EM.f_mid(w64, name, mini, kh, kw, nxt, val[src])))
        y = run_join(dev, w, btype, k, [arena[s] for s in srcs], m_arena, n, h, wd)
        res.append(("join", stored(y, n, h, wd, 64), EM.f_join(w64, name, [val[s] for s in srcs], m64)))
    dev.check()
    return res, dev

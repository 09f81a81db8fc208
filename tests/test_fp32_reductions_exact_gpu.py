"""Counting tests for the fp32 norm and reduction kernels of csrc/norm.hip and csrc/elementwise.hip, on the exact data of
tests/_exact_data.py: every term a kernel sums is a small dyadic number, every partial sum in any order is exactly representable in
fp32 (tests/test_exact_data_cpu.py proves it per case), so a sum that is not BIT-EQUAL to the fp64 value means an element was dropped,
duplicated or read from the wrong place -- whatever the slicing, the wave reduction or the order of a chain.

Each case is the smallest shape that reaches one slicing regime (the tables in _exact_data.py; test_exact_data_cpu.py asserts that they
reach them).  The calls go straight through the C ABI in the guarded arenas of test_abi_memory_contract_gpu.run_spec: exact-size
workspaces, prefilled with NaN bytes and then with junk, the outputs bit-identical between the two.

Bit-equality is asserted wherever the output is a pure sum or an element-wise dyadic expression.  Where the kernel rounds behind its exact
sums (mean and variance: 1/M, a product, dm*dm, a subtraction; dx of the norm backward when M is no power of two; the scalar outputs of
the mean and loss reductions; da of the pixel loss) the absolute error is bounded by 2^-21 (eight units of fp32 roundoff, for at most
four roundings) times the largest magnitude that enters that last expression; a group whose |x_first| exceeds its deviations is also
allowed the half unit in the last place of the stored mean, which at |x_first| ~ 1000 is ten times the deviations' bound and which no fp32
output can avoid (_exact_data.ulp_bound_mean)."""
import pytest
import torch

import _exact_data as X
from test_abi_memory_contract_gpu import F32, Spec, _L, run_spec

pytestmark = pytest.mark.gpu


def _bits(k, ref):
    return (k, ref, "bits", 0)


def _bounded(k, ref, bound):
    """|got - ref| <= bound element by element (bound a tensor or a number), reported as the largest error in units of its bound"""
    def chk(got):
        err = (got[k].double().reshape(ref.shape) - ref).abs()
        b = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
        worst = float((err / b.clamp_min(1e-300)).max())
        return [(k + " err/bound", worst, 1.0 + 2.0 ** -40)]
    return chk


def _f(t):
    """the fp32 tensor handed to the kernel: every value of the exact data is representable"""
    r = t.float()
    assert torch.equal(r.double(), t.double())
    return r.contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# vcg_norm_stats, vcg_norm_act_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
_NORM_CACHE = {}


def _norm_case(case):
    key = case[:7]
    if key not in _NORM_CACHE:
        _NORM_CACHE.clear()                                             # one case's tensors at a time
        label, mode, n, c, h, w, big, _ = case
        r = X.group_regime(mode, n, c, h * w)
        P = X.group_data("norm", mode, n, c, h * w, r["split"], r["vec"], big)
        _NORM_CACHE[key] = (P, X.norm_reference(P), r)
    return _NORM_CACHE[key]


def _norm_note(label, r, big):
    return "[%s; split %d, %s, M %d%s]" % (label, r["split"], "float4" if r["vec"] else "scalar", r["M"], ", offsets ~1000" if big else "")


# a case's two kernels run back to back, so that its data and references are computed once
NORM = [(c, k) for c in X.NORM_CASES for k in ("stats", "act_bwd")]


@pytest.mark.parametrize("case,kernel", NORM, ids=["%s-%s-%dx%dx%dx%d" % ((k,) + c[1:6]) for c, k in NORM])
def test_norm_exact(rt, case, kernel):
    (_norm_stats_exact if kernel == "stats" else _norm_act_bwd_exact)(rt, case)


def _norm_stats_exact(rt, case):
    L = _L()
    label, mode, n, c, h, w, big, _ = case
    P, R, r = _norm_case(case)
    hw, G = h * w, P["G"]
    code = L.NORM_INSTANCE if mode == "instance" else L.NORM_BATCH

    def call(p, ws, wsn, s):
        return rt.lib.vcg_norm_stats(p["x"], n, c, hw, code, p["mean"], p["var"], ws, wsn, s)
    checks = [_bounded("mean", R["mean"], X.ulp_bound_mean(R["first"], R["mean"], R["dev_max"])),
              _bounded("var", R["var"], X.U8 * R["dev_max"] ** 2)]
    run_spec(rt, "exact vcg_norm_stats-%s-%dx%dx%dx%d" % (mode, n, c, h, w),
             Spec(dict(x=_f(P["x"])), dict(mean=((G,), F32), var=((G,), F32)), call, checks,
                  ws=rt.lib.vcg_norm_stats_workspace_bytes(n, c, hw, code), note=_norm_note(label, r, big)))


def _norm_act_bwd_exact(rt, case):
    L = _L()
    label, mode, n, c, h, w, big, _ = case
    P, R, r = _norm_case(case)
    hw, inst = h * w, mode == "instance"
    code = L.NORM_INSTANCE if inst else L.NORM_BATCH
    ins = dict(x=_f(P["x"]), dy=_f(P["dy"]), mean=_f(P["mean"]), invstd=_f(P["invstd"]), alpha=_f(P["alpha"]))
    outs = dict(dx=((n, c, hw), F32), dalpha=((c,), F32))
    checks = [_bits("dalpha", R["dalpha"])]
    if not inst:
        ins.update(gamma=_f(P["gamma"]), beta=_f(P["beta"]))
        outs.update(dgamma=((c,), F32), dbeta=((c,), F32))
        checks += [_bits("dgamma", R["dgamma"]), _bits("dbeta", R["dbeta"])]
    if X.is_pow2(P["M"]):
        checks.append(_bits("dx", R["dx"]))
    else:
        # 1/M and its two products, xhat * (s1/M) and two subtractions round: at most 4 units of roundoff of the sum of the magnitudes
        checks.append(_bounded("dx", R["dx"], X.U8 * R["dx_mag"]))

    def call(p, ws, wsn, s):
        return rt.lib.vcg_norm_act_bwd(p["x"], p["dy"], n, c, hw, code, p["mean"], p["invstd"], p.get("gamma"), p.get("beta"), L.ACT_PRELU, 0.0,
                                       p["alpha"], 1, p["dx"], p.get("dgamma"), p.get("dbeta"), p["dalpha"], ws, wsn, s)
    run_spec(rt, "exact vcg_norm_act_bwd-%s-%dx%dx%dx%d" % (mode, n, c, h, w),
             Spec(ins, outs, call, checks, ws=rt.lib.vcg_norm_act_bwd_workspace_bytes(n, c, hw, code),
                  note=_norm_note(label, r, big) + (" dx bit-equal" if X.is_pow2(P["M"]) else " dx within 2^-21")))


# ---------------------------------------------------------------------------------------------------------------------------------
# vcg_norm_act_fwd
# ---------------------------------------------------------------------------------------------------------------------------------
FWD = [(c, ps, act) for c in X.FWD_CASES for ps in (0, 1) for act in ("prelu", "lrelu")]


@pytest.mark.parametrize("case,ps,act", FWD, ids=["%dx%dx%d-ps%d-%s" % (c[1], c[2], c[3], ps, act) for c, ps, act in FWD])
def test_norm_act_fwd_exact(rt, case, ps, act):
    L = _L()
    label, n, c, hw, path = case
    D = X.fwd_data(n, c, hw, ps, act)
    prelu = act == "prelu"

    def call(p, ws, wsn, s):
        return rt.lib.vcg_norm_act_fwd(p["x"], n, c, hw, p["scale"], p["shift"], ps, L.ACT_PRELU if prelu else L.ACT_LRELU, D["slope"],
                                       p["alpha"] if prelu else None, p["res"], p["y"], s)
    run_spec(rt, "exact vcg_norm_act_fwd-%dx%dx%d-ps%d-%s" % (n, c, hw, ps, act),
             Spec(dict(x=_f(D["x"]), scale=_f(D["scale"]), shift=_f(D["shift"]), alpha=_f(D["alpha"]), res=_f(D["res"])),
                  dict(y=((n, c, hw), F32)), call, [_bits("y", D["y"])], note="[%s; %s path]" % (label, path)))


# ---------------------------------------------------------------------------------------------------------------------------------
# vcg_act_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.ACT_BWD_CASES, ids=["%s-%dx%dx%d" % c[1:5] for c in X.ACT_BWD_CASES])
def test_act_bwd_exact(rt, case):
    L = _L()
    label, act, n, c, hw, _ = case
    D = X.act_bwd_data(act, n, c, hw)
    R = X.act_bwd_reference(D)
    r = X.act_bwd_regime(n, c, hw)
    prelu = act == "prelu"
    outs, checks = dict(dx=((n, c, hw), F32), dsum=((c,), F32)), [_bits("dx", R["dx"]), _bits("dsum", R["dsum"])]
    if prelu:
        outs["dalpha"] = ((c,), F32)
        checks.append(_bits("dalpha", R["dalpha"]))

    def call(p, ws, wsn, s):
        return rt.lib.vcg_act_bwd(p["saved"], p["dy"], n, c, hw, L.ACT_PRELU if prelu else L.ACT_LRELU, D["slope"], p["alpha"] if prelu else None,
                                  p["dx"], p.get("dalpha"), p["dsum"], ws, wsn, s)
    run_spec(rt, "exact vcg_act_bwd-%s-%dx%dx%d" % (act, n, c, hw),
             Spec(dict(saved=_f(D["saved"]), dy=_f(D["dy"]), alpha=_f(D["alpha"])), outs, call, checks, ws=rt.lib.vcg_act_bwd_workspace_bytes(n, c, hw),
                  note="[%s; gx %d, %s, %d pass(es), chains 32/8/1: %d/%d/%d]" % (label, r["gx"], "float4" if r["vec"] else "scalar", r["passes"],
                                                                                  r["chain32"], r["chain8"], r["chain1"])))


# ---------------------------------------------------------------------------------------------------------------------------------
# vcg_channel_sum
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.CHANNEL_SUM_CASES, ids=["%dx%dx%d" % c[1:4] for c in X.CHANNEL_SUM_CASES])
def test_channel_sum_exact(rt, case):
    label, n, c, hw, _ = case
    r = X.group_regime("batch", n, c, hw, vec_kernel=False, split_fn=X.pick_split_cs)
    P = X.group_data("chsum", "batch", n, c, hw, r["split"], False, offsets="none")

    def call(p, ws, wsn, s):
        return rt.lib.vcg_channel_sum(p["x"], n, c, hw, p["out"], ws, wsn, s)
    run_spec(rt, "exact vcg_channel_sum-%dx%dx%d" % (n, c, hw),
             Spec(dict(x=_f(P["x"])), dict(out=((c,), F32)), call, [_bits("out", P["x"].sum((0, 2)))],
                  ws=rt.lib.vcg_channel_sum_workspace_bytes(n, c, hw), note="[%s; split %d, M %d]" % (label, r["split"], r["M"])))


# ---------------------------------------------------------------------------------------------------------------------------------
# vcg_mean_reduce, vcg_pixel_loss
# ---------------------------------------------------------------------------------------------------------------------------------
def _flat_note(label, count):
    r = X.flat_regime(count)
    return "[%s; %d block(s), %d pass(es)]" % (label, r["blocks"], r["passes"])


@pytest.mark.parametrize("case", X.FLAT_CASES, ids=[str(c[1]) for c in X.FLAT_CASES])
def test_mean_reduce_exact(rt, case):
    label, count, _ = case
    D = X.flat_data(count)
    ref = X.flat_reference(D)["mean"].view(1)

    def call(p, ws, wsn, s):
        return rt.lib.vcg_mean_reduce(p["x"], count, p["out"], ws, wsn, s)
    run_spec(rt, "exact vcg_mean_reduce-%d" % count,
             Spec(dict(x=_f(D["x"])), dict(out=((1,), F32)), call, [_bounded("out", ref, X.U8 * ref.abs())],
                  ws=rt.lib.vcg_mean_reduce_workspace_bytes(count), note=_flat_note(label, count)))


@pytest.mark.parametrize("kind", ["mse", "mae"])
@pytest.mark.parametrize("case", X.FLAT_CASES, ids=[str(c[1]) for c in X.FLAT_CASES])
def test_pixel_loss_exact(rt, case, kind):
    L = _L()
    label, count, _ = case
    D = X.flat_data(count)
    R = X.flat_reference(D)
    ref, da = R[kind].view(1), R["da_" + kind]

    def call(p, ws, wsn, s):
        return rt.lib.vcg_pixel_loss(p["a"], p["b"], count, L.LOSS_MSE if kind == "mse" else L.LOSS_MAE, X.GRAD_SCALE, p["out"], p["da"], ws, wsn, s)
    run_spec(rt, "exact vcg_pixel_loss-%s-%d" % (kind, count),
             Spec(dict(a=_f(D["a"]), b=_f(D["b"])), dict(out=((1,), F32), da=((count,), F32)), call,
                  [_bounded("out", ref, X.U8 * ref.abs()), _bounded("da", da, X.U8 * da.abs())],
                  ws=rt.lib.vcg_mean_reduce_workspace_bytes(count), note=_flat_note(label, count)))

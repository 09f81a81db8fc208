"""Exact ("dyadic") data for the fp32 norm and reduction kernels, CPU only.

Every value is a small integer or a small integer times a power of two, chosen so that every term a kernel sums is a multiple of one
power of two (the granularity) and count * max|term| / granularity <= 2^24.  Then EVERY partial sum, in any order and any grouping, is
an integer below 2^24 in units of the granularity, i.e. exactly representable in fp32: the kernel's sum must equal the exact sum bit
for bit whatever its slicing, wave reduction or chain order.  A different value means an element was dropped, duplicated or read from
the wrong place.  exact_budget() is that condition (a condition on the data, not a measurement of the kernel).

What the method cannot see: how well a kernel rounds (nothing rounds here), and an element whose summed term is zero -- the group's
first element in the statistics (the kernels sum x - x_first), any element with zero deviation or zero gradient.  The generators
therefore force non-zero terms of one sign onto the elements at slice boundaries (first and last element of every slice, the element
that follows a group or plane in memory).

pick_split, pick_split_cs and slice_len are COPIES of the host functions in csrc/norm.hip and csrc/elementwise.hip.  They only label
which regime a case reaches and place the forced boundary elements; the GPU checks do not depend on them being right.
"""
import zlib

import torch

F64 = torch.float64
BUDGET = float(2 ** 24)
U8 = 2.0 ** -21            # eight units of fp32 roundoff (2^-24 each): the bound on an output formed by at most four roundings behind exact sums
MUTATIONS = ("skip_last", "dup_first", "overread")


def gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()) % (2 ** 31))


# ---------------------------------------------------------------------------------------------------------------------------------
# copies of the host-side slicing arithmetic (csrc/norm.hip: pick_split, slice_len, kMaxSplit; csrc/elementwise.hip: pick_split_cs)
# ---------------------------------------------------------------------------------------------------------------------------------
MAX_SPLIT = 64


def pick_split(groups, elems_per_group):
    """COPY of pick_split in csrc/norm.hip"""
    s = 1
    while s < MAX_SPLIT and groups * s < 1024 and elems_per_group // (s * 2) >= 2048:
        s *= 2
    return s


def pick_split_cs(c, per_channel):
    """COPY of pick_split_cs in csrc/elementwise.hip"""
    s = 1
    while s < MAX_SPLIT and c * s < 1024 and per_channel // (s * 2) >= 2048:
        s *= 2
    return s


def slice_len(M, split, vec):
    """COPY of slice_len in csrc/norm.hip"""
    per = (M + split - 1) // split
    if vec:
        per = (per + 3) & ~3
    return per


def slices(M, split, vec):
    per = slice_len(M, split, vec)
    out = []
    for s in range(split):
        beg, end = s * per, min(s * per + per, M)
        if beg < end:
            out.append((beg, end))
    return out


def group_regime(mode, n, c, hw, vec_kernel=True, split_fn=pick_split):
    """which slicing regime the sliced kernels (norm statistics / backward sums, channel sum) take for this shape"""
    inst = mode == "instance"
    groups, M = (n * c, hw) if inst else (c, n * hw)
    split = split_fn(groups, M)
    vec = vec_kernel and hw % 4 == 0
    sl = slices(M, split, vec)
    inner = [end for _, end in sl[:-1]]
    return dict(groups=groups, M=M, split=split, vec=vec, per=slice_len(M, split, vec),
                rounded_up=vec and ((M + split - 1) // split) % 4 != 0,
                crosses_planes=(not inst) and any((end - 1) // hw > beg // hw for beg, end in sl),
                boundary_inside_middle_plane=(not inst) and any(e % hw != 0 and 0 < e // hw < n - 1 for e in inner),
                capped_by_groups=split < split_fn(1, M) and split < MAX_SPLIT,
                at_max_split=split == MAX_SPLIT,
                apply_gx=min(64, -(-hw // (1024 if hw % 4 == 0 else 256))),
                apply_gx_capped=-(-hw // (1024 if hw % 4 == 0 else 256)) > 64)


def act_bwd_regime(n, c, hw):
    """vcg_act_bwd: gx = min(64, ceil(hw / 1024)) blocks per plane on both paths, float4 when hw % 4 == 0; plane_partial_final_kernel
    sums n * gx partials per channel in chains of 32, then 8, then 1"""
    gx_raw = max(1, -(-hw // 1024))
    gx = min(64, gx_raw)
    vec = hw % 4 == 0
    total = n * gx
    per_pass = gx * (1024 if vec else 256)
    return dict(gx=gx, gx_capped=gx_raw > 64, vec=vec, passes=-(-hw // per_pass), ragged_end=hw % per_pass != 0,
                chain32=total // 32, chain8=(total % 32) // 8, chain1=total % 8)


def flat_regime(count):
    """vcg_mean_reduce / vcg_pixel_loss: min(1024, ceil(count / 256)) blocks of 256, grid-stride"""
    nb_raw = -(-count // 256)
    nb = min(1024, nb_raw)
    return dict(blocks=nb, capped=nb_raw > 1024, passes=-(-count // (nb * 256)), ragged=count % 256 != 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the budget
# ---------------------------------------------------------------------------------------------------------------------------------
def granularity(terms):
    """largest power of two that divides every (fp64, dyadic) term"""
    t = terms.double().flatten()
    t = t[t != 0]
    if t.numel() == 0:
        return 1.0
    scaled = t.abs() * 2.0 ** 40
    assert bool((scaled == scaled.round()).all()) and float(scaled.max()) < 2.0 ** 62, "terms are not dyadic at 2^-40"
    k = scaled.to(torch.int64)
    low = k & -k
    return float(low.min()) * 2.0 ** -40


def exact_budget(terms, count):
    """count * max|term| / granularity: <= 2^24 makes every partial sum of up to `count` of these terms, in any order, exact in fp32"""
    t = terms.double()
    assert bool(torch.isfinite(t).all())
    return count * float(t.abs().max()) / granularity(t)


# ---------------------------------------------------------------------------------------------------------------------------------
# the case tables (regime label, shape, the regime properties the CPU test asserts)
# ---------------------------------------------------------------------------------------------------------------------------------
# (label, mode, n, c, h, w, big_offset, expected regime)
NORM_CASES = [
    ("split 1, scalar, hw < 256", "batch", 3, 5, 7, 9, True, dict(split=1, vec=False)),
    ("split 2, scalar, boundary inside a middle plane", "batch", 3, 5, 37, 45, True,
     dict(split=2, vec=False, M=4995, boundary_inside_middle_plane=True, crosses_planes=True)),
    ("split 2, float4, slice length rounded up", "instance", 2, 3, 50, 82, True, dict(split=2, vec=True, rounded_up=True, per=2052)),
    ("split 2, float4, slice crossing planes", "batch", 3, 4, 36, 38, False, dict(split=2, vec=True, M=4104, crosses_planes=True)),
    ("split 4, scalar", "batch", 2, 6, 65, 65, False, dict(split=4, vec=False, crosses_planes=True)),
    ("split 4, float4", "batch", 2, 6, 64, 64, False, dict(split=4, vec=True)),
    ("split 2, instance, scalar", "instance", 2, 3, 45, 111, False, dict(split=2, vec=False)),
    ("split capped by the group count", "batch", 2, 513, 64, 64, False, dict(split=2, vec=True, capped_by_groups=True)),
    ("split 64, scalar, apply gx capped", "batch", 1, 3, 362, 363, False, dict(split=64, vec=False, at_max_split=True, apply_gx_capped=True)),
    ("split 64, float4, apply gx capped", "batch", 1, 3, 256, 512, False, dict(split=64, vec=True, at_max_split=True, apply_gx_capped=True)),
]

# (label, n, c, hw, expected regime)
CHANNEL_SUM_CASES = [
    ("split 1", 2, 3, 100, dict(split=1)),
    ("split 4 crossing planes", 3, 5, 2773, dict(split=4, crosses_planes=True, boundary_inside_middle_plane=True)),
    ("split 64", 1, 3, 131406, dict(split=64, at_max_split=True)),
    ("split capped by the channel count", 2, 513, 4096, dict(split=2, capped_by_groups=True)),
]

# (label, act, n, c, hw, expected regime)
ACT_BWD_CASES = [
    ("gx 1, scalar", "prelu", 3, 5, 63, dict(gx=1, vec=False, passes=1)),
    ("gx 1, scalar, lrelu", "lrelu", 3, 5, 63, dict(gx=1, vec=False, passes=1)),
    ("1 < gx < 64, scalar", "prelu", 2, 3, 37 * 45, dict(gx=2, vec=False, gx_capped=False)),
    ("chains of 32, 8 and 1 all taken", "prelu", 9, 3, 4100, dict(gx=5, vec=True, chain32=1, chain8=1, chain1=5)),
    ("gx capped, second pass, ragged, float4", "prelu", 1, 2, 66000, dict(gx=64, gx_capped=True, vec=True, passes=2, ragged_end=True)),
    ("gx capped, further passes, ragged, scalar", "prelu", 1, 2, 66001, dict(gx=64, gx_capped=True, vec=False, ragged_end=True)),
]

# (label, n, c, hw, expected path): y = act(x * scale + shift) + residual; each runs with per_sample 0 / 1 and PReLU / LeakyReLU
FWD_CASES = [
    ("flat, hw 1", 70, 33, 1, "flat"),
    ("flat, hw 63", 3, 5, 63, "flat"),
    ("scalar, ragged last block", 2, 3, 37 * 45, "scalar"),
    ("float4, second block of one float4", 2, 3, 1028, "float4"),
    ("float4, hw 64: the flat path's boundary", 2, 3, 64, "float4"),
]

# (label, count, expected regime)
FLAT_CASES = [
    ("one ragged block", 100, dict(blocks=1, capped=False, passes=1, ragged=True)),
    ("40 blocks, ragged", 10007, dict(blocks=40, capped=False, passes=1, ragged=True)),
    ("1024-block cap, ragged second pass", 262144 + 300 + 1, dict(blocks=1024, capped=True, passes=2, ragged=True)),
]


def fwd_path(n, c, hw):
    """COPY of the dispatch in vcg_norm_act_fwd"""
    if hw < 64 or n * c > 65535:
        return "flat"
    return "float4" if hw % 4 == 0 else "scalar"


# ---------------------------------------------------------------------------------------------------------------------------------
# sliced kernels: norm statistics, norm backward, channel sum
# ---------------------------------------------------------------------------------------------------------------------------------
def group_index(mode, n, c, hw):
    """[G][M] flat offsets into x[n][c][hw] of the elements of each group, in the group's linear order (GroupMap::offset)"""
    if mode == "instance":
        return torch.arange(n * c * hw).view(n * c, hw)
    i = torch.arange(n * hw)
    return ((i // hw)[None, :] * c + torch.arange(c)[:, None]) * hw + (i % hw)[None, :]


def _pow2(g, lo, hi, shape):
    return 2.0 ** torch.randint(lo, hi + 1, shape, generator=g).double()


def group_data(tag, mode, n, c, hw, split, vec, big_offset=False, offsets=None):
    """x = offset[group] + d with d an integer in [-3, 3] and dy a non-zero integer in [-3, 3].  Forced: d = -3 on each group's first
    element, d = -2 and dy > 0 on the first and last element of every slice and on the element that follows the group in memory (with
    mean = offset, negative slope side: every summed term of those elements is non-zero and has the same sign in every slice).
    offsets are distinct integers (consecutive around 0, or of magnitude ~1000 for big_offset), so the groups' first elements differ."""
    inst = mode == "instance"
    G, M = (n * c, hw) if inst else (c, n * hw)
    total = n * c * hw
    g = gen("exact", tag, mode, n, c, hw)
    d = torch.randint(-3, 4, (total,), generator=g)
    dy = torch.randint(1, 4, (total,), generator=g) * (torch.randint(0, 2, (total,), generator=g) * 2 - 1)
    idx = group_index(mode, n, c, hw)
    bpos = sorted({p for beg, end in slices(M, split, vec) for p in (beg, end - 1)})
    forced = idx[:, bpos].flatten()
    after = idx[:, M - 1] + 1
    forced = torch.cat([forced, after[after < total]])
    d[forced] = -2
    dy[forced] = dy[forced].abs()
    d[idx[:, 0]] = -3
    dy[idx[:, 0]] = dy[idx[:, 0]].abs()
    k = torch.arange(G)
    offset = (1 - 2 * (k % 2)) * (1000 - k) if big_offset else k - G // 2
    if offsets == "none":                      # a plain sum (channel sum): no element may be zero at a boundary
        offset = torch.zeros_like(k)
    x = torch.empty(total, dtype=F64)
    x[idx] = (offset[:, None] + d[idx]).double()
    ch = (k % c) if inst else k
    P = dict(mode=mode, n=n, c=c, hw=hw, G=G, M=M, split=split, vec=vec, idx=idx, ch=ch, offset=offset.double(),
             x=x.view(n, c, hw), dy=dy.double().view(n, c, hw),
             mean=offset.double(), invstd=_pow2(g, 0, 1, (G,)),
             gamma=None if inst else _pow2(g, -1, 1, (c,)), beta=None if inst else torch.randint(-2, 1, (c,), generator=g).double(),
             alpha=_pow2(g, -2, -1, (c,)))
    return P


def after_slices(P, t):
    """for a flat [total] tensor t: [G][number of slices], the value that follows each slice's last element IN MEMORY (NaN past the end)"""
    pad = torch.cat([t.flatten().double(), torch.full((1,), float("nan"), dtype=F64)])
    ends = [end - 1 for _, end in slices(P["M"], P["split"], P["vec"])]
    return pad[P["idx"][:, ends] + 1]


def lin(P, t):
    return t.flatten().double()[P["idx"]]


def stats_terms(P, xv):
    """xv [G][K] values of x read for group g -> the two summed terms, as norm.hip's stats_partial_kernel forms them"""
    dev = xv - lin(P, P["x"])[:, :1]
    return dict(dev=dev, dev2=dev * dev)


def bwd_terms(P, xv, dyv):
    """xv, dyv [G][K] values read for group g -> xhat, dz and the three summed terms, as norm_bwd_partial_kernel forms them"""
    ch = P["ch"]
    ga = torch.ones(P["G"], dtype=F64) if P["gamma"] is None else P["gamma"][ch]
    be = torch.zeros(P["G"], dtype=F64) if P["beta"] is None else P["beta"][ch]
    al = P["alpha"][ch]
    xh = (xv - P["mean"][:, None]) * P["invstd"][:, None]
    z = ga[:, None] * xh + be[:, None]
    dz = dyv * torch.where(z > 0, torch.ones_like(z), al[:, None].expand_as(z))
    return dict(xh=xh, dz=dz, dz_xhat=dz * xh, dy_minz=dyv * torch.clamp(z, max=0), gi=(ga * P["invstd"])[:, None])


def norm_reference(P):
    """fp64 references of vcg_norm_stats and vcg_norm_act_bwd (use_batch_stats = 1) on this data; the sums are exact"""
    xl, dl = lin(P, P["x"]), lin(P, P["dy"])
    S, B = stats_terms(P, xl), bwd_terms(P, xl, dl)
    M, G, c, n = P["M"], P["G"], P["c"], P["n"]
    first = xl[:, 0]
    dm = S["dev"].sum(1) / M
    mean, var = first + dm, S["dev2"].sum(1) / M - dm * dm
    s0, s1, s2 = B["dz"].sum(1), B["dz_xhat"].sum(1), B["dy_minz"].sum(1)
    a, b = (s0 / M)[:, None], B["xh"] * (s1 / M)[:, None]
    dx = torch.empty(P["x"].numel(), dtype=F64)
    dx[P["idx"]] = B["gi"] * (B["dz"] - a - b)
    inst = P["mode"] == "instance"
    per_ch = (lambda s: s.view(n, c).sum(0)) if inst else (lambda s: s)
    mag = float(B["gi"].abs().max()) * (float(B["dz"].abs().max()) + float(a.abs().max()) + float(b.abs().max()))
    return dict(first=first, mean=mean, var=var, dev_max=S["dev"].abs().amax(1), dbeta=per_ch(s0), dgamma=per_ch(s1), dalpha=per_ch(s2),
                dx=dx.view(n, c, P["hw"]), dx_mag=mag, dx_parts=torch.cat([B["dz"].flatten(), a.flatten(), b.flatten(), (B["dz"] - a).flatten(),
                                                                          (B["dz"] - a - b).flatten()]),
                terms=dict(S, dz=B["dz"], dz_xhat=B["dz_xhat"], dy_minz=B["dy_minz"]))


def slicewise_sum(P, term_lin, term_after, mutation=None):
    """sum term_lin [G][M] slice by slice with the kernels' slice arithmetic; mutation: None, or one deliberately wrong boundary in every
    slice -- 'skip_last' (the slice's last element left out), 'dup_first' (its first counted twice), 'overread' (a float4 tail that takes
    the element behind the slice's last one in memory: term_after [G][slices])"""
    tot = torch.zeros(term_lin.shape[0], dtype=F64)
    for k, (beg, end) in enumerate(slices(P["M"], P["split"], P["vec"])):
        if mutation == "skip_last":
            s = term_lin[:, beg:end - 1].sum(1)
        else:
            s = term_lin[:, beg:end].sum(1)
            if mutation == "dup_first":
                s = s + term_lin[:, beg]
            elif mutation == "overread":
                s = s + term_after[:, k]
        tot = tot + s
    return tot


# ---------------------------------------------------------------------------------------------------------------------------------
# vcg_norm_act_fwd
# ---------------------------------------------------------------------------------------------------------------------------------
def fwd_data(n, c, hw, per_sample, act):
    g = gen("exactfwd", n, c, hw, per_sample, act)
    rows = n * c if per_sample else c
    x = torch.randint(-12, 13, (n, c, hw), generator=g).double()
    res = torch.randint(-5, 6, (n, c, hw), generator=g).double()
    scale = _pow2(g, -1, 1, (rows,))
    shift = torch.randint(-9, 10, (rows,), generator=g).double() * 0.25
    alpha = _pow2(g, -2, -1, (c,))
    slope = 0.25
    sv = (lambda t: t.view(n, c, 1)) if per_sample else (lambda t: t.view(1, c, 1))
    u = x * sv(scale) + sv(shift)
    y = torch.where(u >= 0, u, (alpha.view(1, c, 1) if act == "prelu" else slope) * u) + res
    return dict(x=x, res=res, scale=scale, shift=shift, alpha=alpha, slope=slope, y=y)


# ---------------------------------------------------------------------------------------------------------------------------------
# vcg_act_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
def act_bwd_data(act, n, c, hw):
    """saved (PReLU: the input; LeakyReLU: the output) and dy; each plane's first and last element on the negative side with dy > 0"""
    g = gen("exactact", act, n, c, hw)
    x = torch.randint(-3, 4, (n, c, hw), generator=g).double()
    dy = (torch.randint(1, 4, (n, c, hw), generator=g) * (torch.randint(0, 2, (n, c, hw), generator=g) * 2 - 1)).double()
    for e in (0, hw - 1):
        x[:, :, e] = -2
        dy[:, :, e] = dy[:, :, e].abs()
    alpha, slope = _pow2(g, -2, -1, (c,)), 0.25
    saved = x if act == "prelu" else torch.where(x >= 0, x, slope * x)
    return dict(act=act, n=n, c=c, hw=hw, saved=saved, dy=dy, alpha=alpha, slope=slope)


def act_bwd_terms(D, sv, dyv):
    """sv, dyv [n][c][K] -> dx and dy * min(saved, 0) as act_bwd_one forms them"""
    al = D["alpha"].view(1, -1, 1) if D["act"] == "prelu" else torch.full((1, D["c"], 1), D["slope"], dtype=F64)
    dx = dyv * torch.where(sv > 0, torch.ones_like(sv), al.expand_as(sv))
    return dict(dx=dx, dy_mins=dyv * torch.clamp(sv, max=0))


def act_bwd_reference(D):
    T = act_bwd_terms(D, D["saved"], D["dy"])
    return dict(dx=T["dx"], dsum=T["dx"].sum((0, 2)), dalpha=T["dy_mins"].sum((0, 2)), terms=T)


def planewise_sum(term, mutation=None):
    """per-channel sum of term [n][c][hw], plane by plane (the slice of act_bwd_kernel and of a flat reduction is the whole plane / array);
    'overread' takes the element behind the plane in memory (NaN behind the tensor)"""
    n, c, hw = term.shape
    s = term.sum(2)
    if mutation == "skip_last":
        s = term[:, :, :hw - 1].sum(2)
    elif mutation == "dup_first":
        s = s + term[:, :, 0]
    elif mutation == "overread":
        pad = torch.cat([term.flatten(), torch.full((1,), float("nan"), dtype=F64)])
        s = s + pad[(torch.arange(n * c) + 1) * hw].view(n, c)
    return s.sum(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# flat reductions
# ---------------------------------------------------------------------------------------------------------------------------------
GRAD_SCALE = 0.75


def flat_data(count):
    """x for vcg_mean_reduce, (a, b) for vcg_pixel_loss: integers, non-zero x and a - b at both ends"""
    g = gen("exactflat", count)
    x = torch.randint(-2, 5, (count,), generator=g).double()
    a = torch.randint(-2, 3, (count,), generator=g).double()
    b = torch.randint(-1, 2, (count,), generator=g).double()
    for e in (0, count - 1):
        x[e], a[e], b[e] = 3, 2, -1
    return dict(count=count, x=x, a=a, b=b)


def flat_reference(D):
    d, count = D["a"] - D["b"], D["count"]
    return dict(mean=D["x"].sum() / count, mse=(d * d).sum() / count, mae=d.abs().sum() / count,
                da_mse=2.0 * d * (GRAD_SCALE / count), da_mae=torch.sign(d) * (GRAD_SCALE / count),
                terms=dict(x=D["x"], sq=d * d, ab=d.abs()))


def ulp_bound_mean(first, mean, dev_max):
    """|mean error| allowed per group: 2^-21 * max|x - x_first| (the roundings of 1/M, of the product and of the last addition).  Where
    |x_first| exceeds max|x - x_first| the stored mean's own half unit in the last place (<= 2^-24 |mean|) can exceed that by itself --
    at |x_first| ~ 1000 it is 3e-5 against 3e-6 -- and no fp32 output avoids it: those groups, and only those, are allowed it on top"""
    return U8 * dev_max + torch.where(first.abs() > dev_max, 2.0 ** -24 * mean.abs(), torch.zeros_like(mean))


def is_pow2(m):
    return m & (m - 1) == 0

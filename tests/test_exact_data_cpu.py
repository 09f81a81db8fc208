"""The exact-data method of tests/_exact_data.py, proved on the CPU for every case of tests/test_fp32_reductions_exact_gpu.py:
(1) every summed quantity of every case is within the 2^24 budget, (2) the case tables reach every slicing regime they name (by the
copied split functions), (3) the method detects miscounting: a slice-wise sum with the kernels' slice arithmetic and one deliberately
wrong boundary per slice differs from the exact value, for each of three wrong boundaries."""
import functools

import pytest
import torch

import _exact_data as X


@functools.lru_cache(maxsize=None)
def _norm(i):
    label, mode, n, c, h, w, big, _ = X.NORM_CASES[i]
    r = X.group_regime(mode, n, c, h * w)
    P = X.group_data("norm", mode, n, c, h * w, r["split"], r["vec"], big)
    return P, X.norm_reference(P)


@functools.lru_cache(maxsize=None)
def _chsum(i):
    label, n, c, hw, _ = X.CHANNEL_SUM_CASES[i]
    r = X.group_regime("batch", n, c, hw, vec_kernel=False, split_fn=X.pick_split_cs)
    return X.group_data("chsum", "batch", n, c, hw, r["split"], False, offsets="none")


NORM_IDS = ["%s-%dx%dx%dx%d" % c[1:6] for c in X.NORM_CASES]
CS_IDS = ["%dx%dx%d" % c[1:4] for c in X.CHANNEL_SUM_CASES]
ACT_IDS = ["%s-%dx%dx%d" % c[1:5] for c in X.ACT_BWD_CASES]
FLAT_IDS = [str(c[1]) for c in X.FLAT_CASES]


def _expect(regime, want, what):
    for k, v in want.items():
        assert regime[k] == v, "%s: %s is %r, the table wants %r (%r)" % (what, k, regime[k], v, regime)


# ---------------------------------------------------------------------------------------------------------------------------------
# the helper itself
# ---------------------------------------------------------------------------------------------------------------------------------
def _tree_sum_f32(t):
    """a sum whose every addition is an fp32 addition (torch's own fp32 sums accumulate wider on the CPU)"""
    v = torch.zeros(1 << (t.numel() - 1).bit_length(), dtype=torch.float32)
    v[:t.numel()] = t.float()
    while v.numel() > 1:
        h = v.numel() // 2
        v = v[:h] + v[h:]
    return float(v)


def test_granularity_and_budget():
    assert X.granularity(torch.tensor([3.0, -0.75, 0.0, 40.0])) == 0.25
    assert X.granularity(torch.tensor([8.0, 24.0])) == 8.0
    assert X.exact_budget(torch.tensor([3.0, -0.75]), 100) == 100 * 3.0 / 0.25
    with pytest.raises(AssertionError):
        X.granularity(torch.tensor([1.0 / 3.0], dtype=torch.float64))


def test_budget_is_what_makes_fp32_sums_exact():
    """within the budget an fp32 sum in a scrambled order equals the fp64 sum bit for bit; the same terms on top of a large offset
    (x and x^2 summed unshifted at |offset| ~ 1000) leave it and an fp32 running sum misses"""
    g = X.gen("budget")
    t = torch.randint(-6, 7, (131406,), generator=g).double() ** 2 * 0.25
    assert X.exact_budget(t, t.numel()) <= X.BUDGET
    for _ in range(3):
        assert _tree_sum_f32(t[torch.randperm(t.numel(), generator=g)]) == float(t.sum())
    big = (1000.0 + torch.randint(-3, 4, (131406,), generator=g).double()) ** 2
    assert X.exact_budget(big, big.numel()) > X.BUDGET
    assert _tree_sum_f32(big) != float(big.sum())


def test_split_copies_known_values():
    assert X.pick_split(5, 189) == 1 and X.pick_split(5, 4995) == 2 and X.pick_split(6, 8192) == 4 and X.pick_split(3, 131072) == 64
    assert X.pick_split(513, 8192) == 2 and X.pick_split(1024, 1 << 20) == 1 and X.pick_split(1, 1 << 30) == 64
    assert X.pick_split_cs(5, 2079) == 1 and X.pick_split_cs(5, 8319) == 4
    assert X.slice_len(4100, 2, True) == 2052 and X.slice_len(4100, 2, False) == 2050 and X.slice_len(4995, 2, False) == 2498
    assert X.slices(4100, 2, True) == [(0, 2052), (2052, 4100)]


# ---------------------------------------------------------------------------------------------------------------------------------
# (2) the regimes
# ---------------------------------------------------------------------------------------------------------------------------------
def test_case_tables_reach_every_regime():
    seen = []
    for label, mode, n, c, h, w, big, want in X.NORM_CASES:
        r = X.group_regime(mode, n, c, h * w)
        _expect(r, want, "norm %s %dx%dx%dx%d" % (mode, n, c, h, w))
        seen.append((mode, r["split"], r["vec"]))
    assert sum(1 for c in X.NORM_CASES if c[6]) >= 3, "three cases carry the large offsets"
    assert {s for _, s, _ in seen} >= {1, 2, 4, 64}
    assert ("instance", 2, True) in seen and ("instance", 2, False) in seen
    assert {(64, True), (64, False), (4, True), (4, False)} <= {(s, v) for _, s, v in seen}
    for label, n, c, hw, want in X.CHANNEL_SUM_CASES:
        _expect(X.group_regime("batch", n, c, hw, vec_kernel=False, split_fn=X.pick_split_cs), want, "channel sum %dx%dx%d" % (n, c, hw))
    for label, act, n, c, hw, want in X.ACT_BWD_CASES:
        _expect(X.act_bwd_regime(n, c, hw), want, "act bwd %dx%dx%d" % (n, c, hw))
    assert any(c[1] == "lrelu" for c in X.ACT_BWD_CASES)
    for label, n, c, hw, want in X.FWD_CASES:
        assert X.fwd_path(n, c, hw) == want and n * c <= 65535
    assert X.fwd_path(2, 3, 63) == "flat" and X.fwd_path(2, 3, 64) == "float4"
    assert 1028 // 4 == 257 and (37 * 45) % 256 != 0
    for label, count, want in X.FLAT_CASES:
        _expect(X.flat_regime(count), want, "flat %d" % count)


# ---------------------------------------------------------------------------------------------------------------------------------
# (1) the budgets, (3) the three miscounts
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(X.NORM_CASES)), ids=NORM_IDS)
def test_norm_case_budget_and_miscounts(i):
    P, R = _norm(i)
    M, n, inst = P["M"], P["n"], P["mode"] == "instance"
    T = R["terms"]
    for k in ("dev", "dev2", "dz", "dz_xhat", "dy_minz"):
        count = M * n if (inst and k == "dy_minz") else M              # instance mode sums dalpha over the n groups of a channel as well
        assert X.exact_budget(T[k], count) <= X.BUDGET, (k, X.exact_budget(T[k], count))
    if X.is_pow2(M):                                                   # dx = gi * (dz - s0/M - xhat * s1/M) is then exact in any evaluation order
        assert X.exact_budget(R["dx_parts"], 1) <= X.BUDGET, X.exact_budget(R["dx_parts"], 1)
    # summing x and x^2 unshifted would leave the budget where the offsets are large
    if X.NORM_CASES[i][6]:
        assert X.exact_budget(P["x"] * P["x"], M) > X.BUDGET
    # the groups' first elements differ, every forced boundary element has non-zero terms
    first = R["first"]
    assert first.unique().numel() == first.numel()
    # one dropped element moves the mean by >= 1/M: more than the bound on the mean allows
    assert float((1.0 / M - X.ulp_bound_mean(R["first"], R["mean"], R["dev_max"])).min()) > 0
    xa, da = X.after_slices(P, P["x"]), X.after_slices(P, P["dy"])
    A = dict(X.stats_terms(P, xa), **X.bwd_terms(P, xa, da))
    for k in ("dev", "dev2", "dz", "dz_xhat", "dy_minz"):
        exact = X.slicewise_sum(P, T[k], None)
        assert torch.equal(exact, T[k].sum(1))
        for m in X.MUTATIONS:
            wrong = X.slicewise_sum(P, T[k], A[k], m)
            if m == "dup_first" and k in ("dev", "dev2") and P["split"] == 1:
                # the blind spot: the statistics sum x - x_first, and the only slice's first element is x_first itself
                assert torch.equal(wrong, exact)
                continue
            if m == "overread" and k == "dy_minz":
                # behind a group's LAST slice lies another group's element: with this group's mean it may sit on the positive side, where
                # this term is zero (dz and dz*xhat above do see it); behind every other slice lies a forced element of this group
                assert bool((A[k][:, :-1] != 0).all())
                continue
            assert bool((wrong != exact).all()), "%s: %s goes unseen in group(s) %s" % (k, m, (wrong == exact).nonzero().flatten().tolist())


@pytest.mark.parametrize("i", range(len(X.CHANNEL_SUM_CASES)), ids=CS_IDS)
def test_channel_sum_case_budget_and_miscounts(i):
    P = _chsum(i)
    xl = X.lin(P, P["x"])
    assert X.exact_budget(xl, P["M"]) <= X.BUDGET
    assert bool((xl[:, [p for s in X.slices(P["M"], P["split"], False) for p in (s[0], s[1] - 1)]] != 0).all())
    xa = X.after_slices(P, P["x"])
    exact = X.slicewise_sum(P, xl, None)
    assert torch.equal(exact, P["x"].sum((0, 2)))
    for m in X.MUTATIONS:
        assert bool((X.slicewise_sum(P, xl, xa, m) != exact).all()), m


@pytest.mark.parametrize("i", range(len(X.ACT_BWD_CASES)), ids=ACT_IDS)
def test_act_bwd_case_budget_and_miscounts(i):
    label, act, n, c, hw, _ = X.ACT_BWD_CASES[i]
    D = X.act_bwd_data(act, n, c, hw)
    R = X.act_bwd_reference(D)
    keys = ("dx", "dy_mins") if act == "prelu" else ("dx",)
    for k in keys:
        assert X.exact_budget(R["terms"][k], n * hw) <= X.BUDGET
        exact = X.planewise_sum(R["terms"][k])
        assert torch.equal(exact, R["dsum" if k == "dx" else "dalpha"])
        for m in X.MUTATIONS:
            assert bool((X.planewise_sum(R["terms"][k], m) != exact).all()), (k, m)


@pytest.mark.parametrize("i", range(len(X.FLAT_CASES)), ids=FLAT_IDS)
def test_flat_case_budget_and_miscounts(i):
    label, count, _ = X.FLAT_CASES[i]
    D = X.flat_data(count)
    R = X.flat_reference(D)
    for k, t in R["terms"].items():
        assert X.exact_budget(t, count) <= X.BUDGET
        exact = X.planewise_sum(t.view(1, 1, -1))
        assert float(exact) == float(t.sum())
        for m in X.MUTATIONS:
            assert bool((X.planewise_sum(t.view(1, 1, -1), m) != exact).all()), (k, m)
        # one element more or less moves the mean by >= 1/count: more than 2^-21 of the result
        assert 1.0 / count > X.U8 * float(t.sum() / count)


def test_fwd_data_is_exact_in_fp32():
    for label, n, c, hw, _ in X.FWD_CASES:
        for ps in (0, 1):
            for act in ("prelu", "lrelu"):
                D = X.fwd_data(n, c, hw, ps, act)
                assert torch.equal(D["y"].float().double(), D["y"]) and X.exact_budget(D["y"], 1) <= X.BUDGET
                assert bool((D["y"] - D["res"] < 0).any()) and bool((D["y"] - D["res"] > 0).any())

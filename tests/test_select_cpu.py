"""CPU: the host side of greedy batch selection (fitsnap_amd/solvers/select.py) -- the downdate factor and the numpy
statement of the loop against per-step refits (tests/select_cases.py), its properties, the tie rule and argument errors.
No GPU compute is called here."""
import numpy as np
import pytest

from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import select, solver_factory, uq

import select_cases as sc

EPS = sc.EPS
GAP_MIN = 1e-9          # precondition on the inputs: the reference's best and second-best live scores differ by more


def replay(p, picks):
    """The variances and covariance after every pick of ``picks`` by select.py's factor and fold."""
    A, cat, w = p["A"], p["cat"], p["w"]
    C = p["C0"]
    var = uq.fold(A, uq.QUAD, C)
    out = [(var, C, None)]
    for u in picks:
        V = select.downdate_factor(C, w[cat == u, None] * A[cat == u], p["tau"])
        C = select.downdate_cov(C, V)
        var = var - select.fold(A, V)
        out.append((var, C, V))
    return out


def check_against_refits(p, batch, objective):
    ref = sc.refit_reference(p["A"], p["cat"], p["ncat"], p["P0"], p["tau"], p["w"], batch, p["s"], objective)
    assert len(ref["picks"]) == batch and min(ref["gaps"]) > GAP_MIN, ("bad input: choose another seed", ref["gaps"])
    got = select.greedy_host(p["A"], p["cat"], p["ncat"], p["C0"], p["w"], p["tau"], batch, p["s"], objective)
    assert got["picks"] == ref["picks"], (got["picks"], ref["picks"])
    assert np.allclose(got["scores"], ref["scores"], rtol=16 * max(ref["kappa"]) * EPS, atol=0)
    steps = replay(p, ref["picks"])
    worst = 0.0
    for t, (var, C, _) in enumerate(steps):
        r, kappa = ref["var"][t], ref["kappa"][t]
        err = np.abs(var - r)
        worst = max(worst, float(np.max(err[r != 0] / np.abs(r[r != 0]))) / (kappa * EPS))
        assert np.all(err <= 16 * kappa * EPS * np.abs(r)), (t, objective)
        assert np.linalg.norm(C - ref["cov"][t]) <= 16 * kappa * EPS * np.linalg.norm(ref["cov"][t])
    print(f"K={p['A'].shape[1]} {objective}: worst variance error {worst:.2f} kappa eps (bar 16), "
          f"min gap {min(ref['gaps']):.1e}, kappa <= {max(ref['kappa']):.0f}")
    assert np.array_equal(got["var"], steps[-1][0]) and np.array_equal(got["cov"], steps[-1][1])
    return [int((p["cat"] == u).sum()) for u in ref["picks"]]


@pytest.mark.parametrize("K,seed,n_pool,batch", [(1, 11, 60, 8), (7, 12, 120, 16), (31, 13, 200, 16), (128, 14, 200, 16)])
def test_downdate_against_refits(K, seed, n_pool, batch):
    d = []
    for objective in select.OBJECTIVES:
        d += check_against_refits(sc.clustered(seed, K, n_pool=n_pool), batch, objective)
    # small configurations: picks with d <= K
    small = sc.clustered(seed + 100, K, n_pool=n_pool, size_lo=1, size_hi=max(1, K // 2))
    for objective in select.OBJECTIVES:
        d += check_against_refits(small, batch, objective)
    assert any(x <= K for x in d) and any(x > K for x in d)


def test_pinv_covariance_with_a_zero_column():
    p = sc.clustered(13, 31, zero_col=3)
    tiny = 1e-15 * np.abs(p["C0"]).max()              # pinv leaves rounding dust, not exact zeros
    assert np.all(np.abs(p["C0"][3]) <= tiny) and np.all(p["A"][:, 3] == 0.0)
    check_against_refits(p, 16, "sum")
    steps = replay(p, sc.refit_reference(p["A"], p["cat"], p["ncat"], p["P0"], p["tau"], p["w"], 4, p["s"])["picks"])
    for _, C, V in steps[1:]:
        assert np.all(np.abs(C[3]) <= tiny) and np.all(np.abs(C[:, 3]) <= tiny) and np.all(np.abs(V[3]) <= np.sqrt(tiny))


@pytest.mark.parametrize("K", [7, 31])
def test_properties(K):
    p = sc.clustered(20 + K, K, n_pool=80)
    got = select.greedy_host(p["A"], p["cat"], p["ncat"], p["C0"], p["w"], p["tau"], 12, p["s"], "sum")
    C = p["C0"]
    var = uq.fold(p["A"], uq.QUAD, C)
    prev, _, _ = select.aggregate(var, p["s"], p["cat"], p["ncat"])
    alive = np.ones(p["ncat"], dtype=bool)
    for u, V, J in zip(got["picks"], got["factors"], got["ranks"]):
        d = int((p["cat"] == u).sum())
        assert V.shape == (K, min(d, K)) and J == min(d, K)
        # the factor of the d > K picks is the QR form of Z L^-T: the same V V^T
        X = p["w"][p["cat"] == u, None] * p["A"][p["cat"] == u]
        Z = C @ X.T
        direct = Z @ np.linalg.solve(p["tau"] * np.eye(d) + X @ Z, Z.T)
        assert np.allclose(V @ V.T, direct, rtol=0, atol=1e-12 * np.abs(direct).max())
        C = select.downdate_cov(C, V)
        assert np.array_equal(C, C.T)
        assert np.linalg.eigvalsh(C).min() >= -16 * K * EPS * np.linalg.norm(C, 2)
        var = var - select.fold(p["A"], V)
        alive[u] = False
        now, _, _ = select.aggregate(var, p["s"], p["cat"], p["ncat"])
        assert np.all(now[alive] <= prev[alive] * (1 + 8 * EPS))       # a live category's score never increases
        prev = now
    assert np.all(np.diff(got["scores"]) <= 0)


def test_tie_rule():
    assert select.best_live(np.array([1.0, 3.0, 3.0, 2.0]), np.ones(4, dtype=bool)) == 1
    assert select.best_live(np.array([1.0, 3.0, 3.0, 2.0]), np.array([True, False, True, True])) == 2
    assert select.best_live(np.array([np.nan, -np.inf]), np.ones(2, dtype=bool)) == 0
    assert select.best_live(np.array([np.nan, -1.0]), np.ones(2, dtype=bool)) == 1
    assert select.best_live(np.array([1.0]), np.zeros(1, dtype=bool)) == -1
    assert select.best_of_ranks([(2.0, 4), (2.0, 0)]) == (0, 4)
    assert select.best_of_ranks([(1.0, -1), (0.5, 3), (0.75, 1)]) == (2, 1)
    assert select.best_of_ranks([(0.0, -1), (0.0, -1)]) == (-1, -1)
    # two categories with the same rows score the same: the first in key order goes first, then the other's score has dropped
    rng = np.random.default_rng(0)
    K = 5
    blk = rng.standard_normal((4, K))
    A = np.vstack([rng.standard_normal((3, K)) * 0.01, blk, blk])
    cat = np.array([0] * 3 + [1] * 4 + [2] * 4, dtype=np.int32)
    got = select.greedy_host(A, cat, 3, np.eye(K), None, 0.5, 3)
    assert got["picks"] == [1, 2, 0] and got["scores"][1] < got["scores"][0]
    # negative ids take no part, empty categories are never picked
    cat2 = np.array([-1] * 3 + [3] * 4 + [1] * 4, dtype=np.int32)
    got = select.greedy_host(A, cat2, 5, np.eye(K), None, 0.5, 5)
    assert got["picks"] == [1, 3] and len(got["scores"]) == 2


def make_solver():
    pt = ParallelTools()
    return pt, solver_factory.solver("ANL", pt, Config(pt, {"SOLVER": {"solver": "ANL"}}))


def test_argument_errors():
    p = sc.clustered(3, 7, n_pool=10, size_hi=5)
    A, cat = p["A"], p["cat"]
    with pytest.raises(ValueError, match="objective"):
        select.greedy_host(A, cat, 10, p["C0"], None, 0.1, 2, objective="median")
    for bad in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="noise"):
            select.greedy_host(A, cat, 10, p["C0"], None, bad, 2)
    assert select.check_objective("average") == "mean"
    # batch_size larger than the number of categories: every category once, in score order
    got = select.greedy_host(A, cat, 10, p["C0"], p["w"], p["tau"], 25)
    assert sorted(got["picks"]) == list(range(10)) and not got["alive"].any()
    with pytest.raises(ValueError):
        select.greedy_host(A, cat, 10, p["C0"], None, 0.1, -1)
    # the solver surface refuses before it touches a GPU
    pt, s = make_solver()
    assert s.sigmahat is None
    with pytest.raises(ValueError, match="covariance"):
        s.select_batch(2, a=A, categories=cat, noise=0.1)
    with pytest.raises(ValueError, match="noise"):
        s.select_batch(2, a=A, categories=cat, cov=p["C0"])
    with pytest.raises(ValueError, match="noise"):
        s.select_batch(2, a=A, categories=cat, cov=p["C0"], noise=0.0)
    with pytest.raises(ValueError, match="objective"):
        s.select_batch(2, a=A, categories=cat, cov=p["C0"], noise=0.1, objective="best")
    with pytest.raises(ValueError, match="length"):
        s.select_batch(2, a=A, categories=(["g"] * len(cat), ["c"] * (len(cat) - 1)), cov=p["C0"], noise=0.1)
    with pytest.raises(ValueError, match="categories"):
        s.select_batch(2, a=A, cov=p["C0"], noise=0.1)
    with pytest.raises(ValueError, match="weights"):
        s.select_batch(2, a=A, w=np.ones(3), categories=cat, cov=p["C0"], noise=0.1)
    pt.free()


def test_category_layout_and_scores():
    cat, keys = select.category_layout((["a", "a", "b", "a"], [1, 2, 1, 1]))
    assert keys == [("a", 1), ("a", 2), ("b", 1)] and cat.tolist() == [0, 1, 2, 0]
    cat, keys = select.category_layout(np.array([2, -1, 0]))
    assert keys == [0, 1, 2] and cat.dtype == np.int32
    s, mx, n = select.aggregate(np.array([1.0, 2.0, 4.0, 8.0]), np.array([1.0, 1.0, 0.5, 1.0]), np.array([0, 2, 2, -1]), 3)
    assert s.tolist() == [1.0, 0.0, 4.0] and mx.tolist() == [1.0, -np.inf, 2.0] and n.tolist() == [1, 0, 2]
    assert select.scores_of(s, mx, n, "mean")[2] == 2.0 and select.scores_of(s, mx, n, "max")[2] == 2.0

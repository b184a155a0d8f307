"""CPU: the host side of the grouped K-fold LASSO alpha path (fitsnap_amd/solvers/lasso_path.py) -- the host route on given
statistics against scikit-learn refits without each fold, the statistics form of the held-out error against the row-wise
long-double sum, fold dealing, the cross-validation curve and its two picks on hand-made tables, and the refusals."""
import os
import sys
import types

import numpy as np
import pytest

from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import lasso_path as lp
from fitsnap_amd.solvers import solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lasso_path_cases as cs  # noqa: E402


def make(name, sections):
    pt = ParallelTools()
    return pt, solver_factory.solver(name, pt, Config(pt, sections))


@pytest.mark.parametrize("m,K,F", [(600, 24, 4), (900, 70, 3)])
def test_host_route_matches_sklearn_refits_without_each_fold(m, K, F):
    """600 x 24 with 4 folds and 900 x 70 with 3 folds, columns scaled over two decades, 8 alphas from 0.5 down to 1e-5 of
    max |c| / n, tol = 1e-10: every problem passes the gap check (acceptance 1) and is within the strong-convexity bound
    (acceptance 2) of scikit-learn's Lasso on the weighted rows without the fold; the held-out sums are within HELDOUT_REL of
    the row-wise long-double sums."""
    sizes = [m // F + (1 if f < m % F else 0) for f in range(F)]
    A, b, w, fold, _ = cs.fold_rows(77 + K, K, sizes)
    blocks = cs.blocks_numpy(A, b, w, fold, F)
    alphas = cs.alpha_grid(blocks, K, cs.GRID8)
    tol = 1e-10           # tol y2 stays 1e4 x above the 64 K eps y2 rounding of a float64 duality gap
    coef, info, held = lp.lasso_path_host(blocks, K, alphas, cs.MAX_ITER, tol)
    folds, total = lp.sum_blocks(blocks)
    worst = 0.0
    for f in range(F + 1):
        Qm, qv, y2, n, dead = lp.downdated(folds, total, f, K)
        assert not dead.any() and n == m - (sizes[f] if f < F else 0)
        for q, alpha in enumerate(alphas):
            assert info[f, q, 2] == alpha * n and info[f, q, 3] == n
            gap = cs.check_gap(Qm, qv, y2, alpha * n, coef[f, q], info[f, q, 0], info[f, q, 1], cs.MAX_ITER, tol, (f, q))
            ref = cs.sklearn_refit(A, b, w, fold != f, alpha)
            gap_ref = float(cs.gap_ld(Qm, qv, y2, alpha * n, ref))
            diff = float(np.linalg.norm(coef[f, q] - ref))
            assert diff <= cs.bound2(Qm, dead, gap, gap_ref, coef[f, q]), (f, q, diff)
            worst = max(worst, diff / np.linalg.norm(ref))
            if f < F:
                rows = np.flatnonzero(fold == f)
                true = cs.heldout_ld(A, b, w, rows, coef[f, q])
                assert held[f, q, 0] == len(rows) and abs(held[f, q, 1] - true) <= cs.HELDOUT_REL * true
    print(f"{m} x {K}, {F} folds: worst relative difference to scikit-learn {worst:.2e}")
    assert np.count_nonzero(coef[F, 0]) < np.count_nonzero(coef[F, -1])


def test_host_route_dead_columns_empty_folds_and_sub_blocks():
    """A column no row touches and a column fold 1 alone touches are dead where they should be (coefficient exactly 0) and
    live elsewhere; a fold without rows refits to the full fit bit for bit; nsub = 3 sub-blocks give the bits of the folds
    summed beforehand."""
    K, F = 9, 4
    A, b, w, fold, cls = cs.fold_rows(5, K, [40, 45, 0, 50])
    A[:, 2] = 0.0
    A[fold != 1, 6] = 0.0
    b = b + 0.5 * A[:, 6]
    blocks = cs.blocks_numpy(A, b, w, fold, F)
    alphas = cs.alpha_grid(blocks, K, [1e-2, 1e-4])
    coef, info, held = lp.lasso_path_host(blocks, K, alphas, 5000, 1e-10)
    assert np.all(coef[:, :, 2] == 0.0)
    assert np.all(coef[1, :, 6] == 0.0) and np.all(coef[[0, 2, 3, 4], :, 6] != 0.0)
    assert np.array_equal(coef[2], coef[4]) and np.array_equal(info[2], info[4]) and np.all(held[2, :, 0] == 0)
    blocks3 = cs.blocks_numpy(A, b, w, fold * 3 + cls, 3 * F)
    pre, _ = lp.sum_blocks(blocks3, 3)
    c3, i3, h3 = lp.lasso_path_host(blocks3, K, alphas, 5000, 1e-10, nsub=3)
    c1, i1, h1 = lp.lasso_path_host(pre, K, alphas, 5000, 1e-10)
    assert np.array_equal(c3, c1) and np.array_equal(i3, i1) and np.array_equal(h3, h1)
    # threads do not change a bit
    c0, i0, h0 = lp.lasso_path_host(pre, K, alphas, 5000, 1e-10, threads=1)
    assert np.array_equal(c0, c1) and np.array_equal(i0, i1) and np.array_equal(h0, h1)


def test_fold_dealing_is_deterministic_and_balanced():
    keys = [f"cfg{i}" for i in range(23)]
    fold, F = lp.deal_folds(keys, 5, seed=0)
    again, _ = lp.deal_folds(list(reversed(keys)) + keys[:3], 5, seed=0)       # order and repeats do not matter
    assert F == 5 and fold == again and set(fold) == set(keys)
    sizes = np.bincount(list(fold.values()), minlength=5)
    assert sizes.max() - sizes.min() <= 1 and sizes.sum() == 23
    other, _ = lp.deal_folds(keys, 5, seed=1)
    assert other != fold
    assert fold == {k: i % 5 for i, k in enumerate(np.array(sorted(keys))[np.random.default_rng(0).permutation(23)])}


def test_fold_dealing_none_mapping_and_errors():
    keys = ["b", "a", "c", "a"]
    fold, F = lp.deal_folds(keys, None)
    assert F == 3 and fold == {"a": 0, "b": 1, "c": 2}
    fold, F = lp.deal_folds(keys, {"a": "x", "b": "y", "c": "x", "unused": "z"})
    assert F == 2 and fold == {"a": 0, "b": 1, "c": 0}
    fold, F = lp.deal_folds([3, 1, 2], {1: 10, 2: 10, 3: 7})
    assert F == 2 and fold == {1: 1, 2: 1, 3: 0}
    with pytest.raises(ValueError, match="no entry"):
        lp.deal_folds(keys, {"a": 0, "b": 1})
    for bad in (1, 0, 4, 2.5, True):
        with pytest.raises(ValueError):
            lp.deal_folds(keys, bad)


def test_testing_rows_take_no_part_in_the_categories():
    units = ["a", "b", "a", "c", "b", np.str_("c")]
    train = np.array([True, True, False, True, False, True])
    fold = {"a": 1, "b": 0, "c": 2}
    cls = np.array([0, 1, 2, 2, 0, 1], dtype=np.uint8)
    cat = lp.row_categories(units, train, fold, cls, 3)
    assert cat.dtype == np.int32 and cat.tolist() == [3, 1, -1, 8, -1, 7]
    assert lp.row_categories(units, train, fold, cls, 1).tolist() == [1, 0, -1, 2, -1, 2]
    # a unit that only testing rows carry needs no fold
    assert lp.row_categories(["a", "z"], [True, False], {"a": 0}, [0, 0], 1).tolist() == [0, -1]
    # and the statistics of the categories then hold the training rows only
    A, b, w, _, _ = cs.fold_rows(3, 4, [6])
    blocks = cs.blocks_numpy(A, b, w, cat, 9)
    assert blocks[:, -1].sum() == train.sum() and blocks[3, -1] == 1 and blocks[2, -1] == 0


def test_cv_curve_best_and_sparsest_on_a_hand_made_table():
    alphas = np.array([1e-3, 1e-1, 1e-2, 1.0])
    # three folds of 10, 20, 10 rows; sse per (fold, alpha)
    sse = np.array([[10.0, 12.0, 8.0, 40.0],
                    [20.0, 26.0, 22.0, 90.0],
                    [14.0, 10.0, 10.0, 50.0]])
    n = np.array([10.0, 20.0, 10.0])
    held = np.stack([np.repeat(n[:, None], 4, axis=1), sse, 2 * sse], axis=2)
    err, se, best, sparsest = lp.cv_curve(alphas, held)
    np.testing.assert_allclose(err, sse.sum(axis=0) / 40.0, rtol=1e-15)
    np.testing.assert_allclose(se, np.std(sse / n[:, None], axis=0, ddof=1) / np.sqrt(3), rtol=1e-15)
    assert best == 2                                  # 40 / 40 = 1.0 at alpha = 1e-2
    # pooled errors 1.1, 1.2, 1.0, 4.5; fold errors at the minimum 0.8, 1.1, 1.0: se = 0.088, nothing else within it
    assert se[2] == pytest.approx(np.std([0.8, 1.1, 1.0], ddof=1) / np.sqrt(3)) and sparsest == 2
    # a wider spread of the folds at the minimum admits the larger alpha
    held2 = held.copy()
    held2[:, 2, 1] = [4.0, 30.0, 6.0]                 # same pooled error, se = 0.34: 1.1 and 1.2 are within it
    _, se2, best2, sparsest2 = lp.cv_curve(alphas, held2)
    assert best2 == 2 and se2[2] > 0.2 and sparsest2 == 1


def test_cv_curve_ties_go_to_the_larger_alpha_and_empty_folds_do_not_count():
    alphas = np.array([1e-2, 1.0, 1e-1])
    held = np.zeros((3, 3, 3))
    held[0, :, 0], held[0, :, 1] = 10, [5.0, 7.0, 5.0]
    held[1, :, 0], held[1, :, 1] = 10, [5.0, 9.0, 5.0]        # fold 2 holds no rows
    err, se, best, sparsest = lp.cv_curve(alphas, held)
    assert err.tolist() == [0.5, 0.8, 0.5] and se.tolist() == [0.0, pytest.approx(0.1), 0.0]
    assert best == 2 and sparsest == 2
    err, se, best, sparsest = lp.cv_curve(alphas, np.zeros((2, 3, 3)))
    assert best is None and sparsest is None and np.all(np.isnan(err))
    table = lp.stats_table(alphas, held)
    assert table.loc[(1.0, "*ALL"), "ncount"] == 20 and table.loc[(1.0, "*ALL"), "w_rmse"] == pytest.approx(np.sqrt(0.8))


def test_pooling_of_the_row_pass_keeps_each_vector_on_its_own_fold():
    F, Q, nclass = 2, 3, 2
    rng = np.random.default_rng(0)
    sums4 = rng.random((F * Q, F * nclass, 4))
    counts = np.array([3, 4, 5, 6])
    pooled = lp.pool_rows(sums4, counts, F, Q, nclass)
    for q in range(Q):
        for k in range(nclass):
            own = [sums4[f * Q + q, f * nclass + k] for f in range(F)]
            assert pooled[q, k, 0] == counts[k] + counts[nclass + k]
            np.testing.assert_allclose(pooled[q, k, 1:], [own[0][0] + own[1][0], own[0][1] + own[1][1], own[0][3] + own[1][3]])


@pytest.mark.parametrize("name", ["SVD", "RIDGE", "ARD"])
def test_other_solvers_are_refused(name):
    _, s = make(name, {"SOLVER": {"solver": name}})
    with pytest.raises(ValueError, match="has no LASSO path"):
        s.lasso_path([1e-3, 1e-2])


def test_apply_transpose_bad_grids_methods_and_unfitted_solvers_are_refused():
    _, s = make("LASSO", {"SOLVER": {"solver": "LASSO"}, "EXTRAS": {"apply_transpose": 1}})
    with pytest.raises(ValueError, match="apply_transpose"):
        s.lasso_path([1e-3])
    _, s = make("LASSO", {"SOLVER": {"solver": "LASSO"}})
    for bad in ([], [-1.0], [np.nan], [1.0, np.inf]):
        with pytest.raises(ValueError, match="alpha"):
            s.lasso_path(bad)
    with pytest.raises(ValueError, match="method"):
        s.lasso_path([1.0], method="woodbury")
    with pytest.raises(ValueError, match="table"):
        s.lasso_path([1.0], table="units")
    with pytest.raises(RuntimeError, match="perform_fit"):
        s.lasso_path([1.0])
    with pytest.raises(ValueError, match="K <= 144"):
        lp.choose_method("device", 145)
    assert lp.choose_method("auto", 144) == "device" and lp.choose_method("auto", 145) == "host"


def test_rows_that_are_not_those_of_the_fit_are_refused():
    _, s = make("LASSO", {"SOLVER": {"solver": "LASSO"}})
    s.last_statistics = (np.eye(3), np.ones(3), np.zeros(3))
    s.pt.hip = lambda: types.SimpleNamespace(m=7, K=3)
    fs = {"Configs": ["a", "a", "b", "b"], "Groups": ["g"] * 4, "Testing": [False] * 4, "Row_Type": ["Energy"] * 4}
    with pytest.raises(ValueError, match="not those of the fit"):
        s.lasso_path([1.0], folds=2, fs_dict=fs, b=np.zeros(4), w=np.ones(4))
    with pytest.raises(ValueError, match="pass the truths"):
        s.lasso_path([1.0], folds=2, fs_dict=fs)

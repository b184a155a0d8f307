"""CPU: the host side of the leave-one-configuration-out errors (fitsnap_amd/solvers/loco.py) -- both closed forms (J space
and n space) against brute-force refits without each unit, the factors M of C = (G + alpha I)^-1, the unit index, the
table assembly, and the refusal paths."""
import numpy as np
import pytest

from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import loco, solver_factory


def problem(seed, K, sizes, zero_w=0, testing=0):
    """Random rows in units of the given sizes; ``zero_w`` training rows get weight 0, ``testing`` rows are testing."""
    rng = np.random.default_rng(seed)
    m = int(sum(sizes))
    A = rng.standard_normal((m, K)) * rng.uniform(0.5, 2.0, K)
    b = A @ rng.standard_normal(K) + 0.1 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    labels = np.repeat([f"c{i}" for i in range(len(sizes))], sizes)
    test = np.zeros(m, dtype=bool)
    test[rng.choice(m, testing, replace=False)] = True
    w[rng.choice(np.flatnonzero(~test), zero_w, replace=False)] = 0.0
    return A, b, w, labels, test


def brute_force(A, b, w_eff, labels, alpha, rcond=None):
    """Refit without each unit's training rows (RIDGE: (G_-c + alpha I)^-1 c_-c; SVD: lstsq), predict that unit's rows."""
    pred = np.full(len(b), np.nan)
    for u in dict.fromkeys(labels):
        out = labels == u
        keep = ~out & (w_eff != 0)
        Aw, bw = A[keep] * w_eff[keep, None], b[keep] * w_eff[keep]
        if alpha is None:
            beta = np.linalg.lstsq(Aw, bw, rcond=rcond)[0]
        else:
            beta = np.linalg.solve(Aw.T @ Aw + alpha * np.eye(A.shape[1]), Aw.T @ bw)
        pred[out] = A[out] @ beta
    return pred


def fit(A, b, w_eff, alpha):
    Aw, bw = A * w_eff[:, None], b * w_eff
    G = Aw.T @ Aw
    if alpha is None:
        return G, np.linalg.lstsq(Aw, bw, rcond=None)[0]
    return G, np.linalg.solve(G + alpha * np.eye(A.shape[1]), Aw.T @ bw)


CASES = [
    # (K, unit sizes, zero-weight rows, testing rows)
    (5, [3, 4, 9, 12, 6, 20], 0, 0),
    (8, [7, 8, 9, 30, 2, 15, 11], 3, 0),
    (12, [10, 25, 13, 40, 12, 31], 4, 6),
    (31, [20, 45, 33, 60, 50, 28, 44], 5, 10),
]


@pytest.mark.parametrize("alpha", [None, 1e-8, 1e-4, 0.5])
@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("space", ["J", "n", "auto"])
def test_closed_forms_match_brute_force_refits(case, alpha, space):
    K, sizes, nz, nt = CASES[case]
    A, b, w, labels, test = problem(case, K, sizes, nz, nt)
    w_eff = np.where(test, 0.0, w)
    G, beta = fit(A, b, w_eff, alpha)
    M = loco.factor_cholesky(G, alpha or 0.0)
    np.testing.assert_allclose(M @ M.T, np.linalg.inv(G + (alpha or 0.0) * np.eye(K)), rtol=1e-9, atol=1e-12)
    rows, off, units = loco.unit_index(labels, ~test)
    pred, info = loco.loco_host(A, b, w_eff, M, beta, rows, off, space=space)
    ref = brute_force(A, b, w_eff, labels, alpha)
    assert np.all(info[:, 2] == 1.0)
    train = ~test
    assert np.all(np.isnan(pred[test]))
    assert np.max(np.abs(pred[train] - ref[train])) <= 1e-10 * np.max(np.abs(b))
    assert np.array_equal(info[:, 0], np.minimum(np.diff(off), M.shape[1]))


def test_zero_weight_rows_are_predicted_by_the_fit_without_their_unit():
    A, b, w, labels, test = problem(7, 6, [5, 8, 9, 7, 10])
    w_eff = w.copy()
    w_eff[labels == "c2"] = 0.0               # a unit whose rows all have weight 0: its LOO fit is the fit itself
    G, beta = fit(A, b, w_eff, 1e-3)
    rows, off, _ = loco.unit_index(labels, np.ones(len(b), dtype=bool))
    pred, info = loco.loco_host(A, b, w_eff, loco.factor_cholesky(G, 1e-3), beta, rows, off)
    zero = labels == "c2"
    np.testing.assert_allclose(pred[zero], A[zero] @ beta, rtol=0, atol=1e-12 * np.max(np.abs(b)))
    assert info[2, 1] == 1.0                   # H = I: every pivot is 1


def test_truncated_factor_spans_the_kept_directions():
    # rank-deficient rows: the eigen factor of the kept directions is the pseudo-inverse
    rng = np.random.default_rng(3)
    A = rng.standard_normal((60, 4)) @ rng.standard_normal((4, 7))
    G = A.T @ A
    M = loco.factor_eigen(G, rank=4, scaled=False, rcond=0.0)
    assert M.shape == (7, 4)
    np.testing.assert_allclose(M @ M.T, np.linalg.pinv(G, rcond=1e-12), rtol=1e-7, atol=1e-9)
    Ms = loco.factor_eigen(G, rank=4)           # Jacobi-scaled: a different generalised inverse on the same range
    np.testing.assert_allclose(G @ (Ms @ Ms.T) @ G, G, rtol=1e-8, atol=1e-8 * np.abs(G).max())


def test_a_unit_that_alone_touches_a_column_is_flagged_without_ridge():
    A, b, w, labels, test = problem(11, 6, [10, 12, 9, 14], 0, 0)
    A[:, 5] = 0.0
    A[labels == "c1", 5] = 1.0 + np.arange(12) * 0.1          # column 5 lives in unit c1 only
    for alpha, ident in ((None, 0.0), (1e-4, 1.0)):
        G, beta = fit(A, b, w, alpha)
        rows, off, _ = loco.unit_index(labels, np.ones(len(b), dtype=bool))
        pred, info = loco.loco_host(A, b, w, loco.factor_cholesky(G, alpha or 0.0), beta, rows, off)
        assert info[1, 2] == ident
        assert np.all(info[[0, 2, 3], 2] == 1.0)
        assert np.all(np.isnan(pred[labels == "c1"])) == (ident == 0.0)
        assert np.all(np.isfinite(pred[labels != "c1"]))


def test_unit_index_is_stable_and_skips_testing_rows():
    labels = ["b", "a", "b", "c", "a", "b", "c"]
    train = np.array([1, 1, 1, 0, 1, 1, 1], dtype=bool)
    rows, off, units = loco.unit_index(labels, train)
    assert units == ["b", "a", "c"]
    assert rows.tolist() == [0, 2, 5, 1, 4, 6]
    assert off.tolist() == [0, 3, 5, 6]
    assert rows.dtype == np.int32 and off.dtype == np.int64


def make(name, sections):
    pt = ParallelTools()
    return pt, solver_factory.solver(name, pt, Config(pt, sections))


def test_tables_with_a_trivial_hat_matrix_equal_error_analysis():
    # M = 0: every LOO prediction is the in-sample one, so the LOCO tables are error_analysis's training rows
    from pandas import DataFrame

    A, b, w, labels, test = problem(5, 6, [30, 40, 25, 35, 30, 40], 3, 20)
    w_eff = np.where(test, 0.0, w)
    _, beta = fit(A, b, w_eff, 1e-6)
    rows, off, _ = loco.unit_index(labels, ~test)
    pred, _ = loco.loco_host(A, b, w_eff, np.zeros((6, 1)), beta, rows, off)
    train = ~test
    np.testing.assert_array_equal(pred[train], (A @ beta)[train])
    rng = np.random.default_rng(0)
    groups = np.where(np.arange(len(b)) < 90, "g0", "g1")
    rtypes = rng.choice(["Energy", "Force", "Stress"], len(b))
    _, s = make("RIDGE", {"SOLVER": {"solver": "RIDGE"}})
    ok = np.flatnonzero(train)
    keys, st = loco.error_sums(s, b[ok], pred[ok], w[ok], groups[ok].tolist(), rtypes[ok].tolist())
    g, a = s._tables_from_sums(keys, st)
    mine = s._assemble_errors(g, a, None)
    df = DataFrame({"truths": b[ok], "preds": (A @ beta)[ok], "weights": w[ok], "Groups": groups[ok], "Testing": False,
                    "Row_Type": rtypes[ok]})
    g2, a2 = s._host_error_tables(df)
    ref = s._assemble_errors(g2, a2, None)
    assert list(mine.index) == list(ref.index)
    np.testing.assert_allclose(mine.to_numpy(dtype=float), ref.to_numpy(dtype=float), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", ["ARD", "LASSO", "MERR", "MCMC"])
def test_solvers_that_are_not_linear_smoothers_are_refused(name):
    _, s = make(name, {"SOLVER": {"solver": name}})
    with pytest.raises(ValueError, match="not a linear smoother"):
        s.loco_errors()


@pytest.mark.parametrize("name", ["SVD", "RIDGE", "ANL"])
def test_apply_transpose_is_refused(name):
    _, s = make(name, {"SOLVER": {"solver": name}, "EXTRAS": {"apply_transpose": 1}})
    with pytest.raises(ValueError, match="apply_transpose"):
        s.loco_errors()


def test_a_unit_split_across_ranks_is_refused():
    loco.check_units_disjoint([["c0", "c2"], ["c1", "c3"]])
    with pytest.raises(ValueError, match="'c2' has rows on ranks 0 and 1"):
        loco.check_units_disjoint([["c0", "c2"], ["c1", "c2"]])

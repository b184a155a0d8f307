"""CPU: the host side of the leave-one-configuration-out errors (fitsnap_amd/solvers/loco.py) -- both closed forms (J space
and n space) against brute-force refits without each unit, the factors M of C = (G + alpha I)^-1, the unit index, the
table assembly, and the refusal paths; the long-double reference and the bars of the kernel tests (tests/loco_cases.py)
on loco_host, and on three subtly wrong variants of it that the bars must catch."""
import os
import sys

import numpy as np
import pytest

from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import loco, solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loco_cases as lc  # noqa: E402


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


# ---- the reference and the bars of tests/test_gpu_loco.py ----------------------------------------------------------------

def test_long_double_cholesky_solve_and_refit():
    lc.need_long_double()
    rng = np.random.default_rng(1)
    X = rng.standard_normal((40, 12))
    H = X.T @ X
    L, piv, ok = lc.cholesky_ld(H)
    assert ok and L.dtype == np.longdouble and np.all(np.triu(L, 1) == 0)
    assert float(np.max(np.abs(L @ L.T - H))) <= 1e-17 * np.max(np.abs(H))
    np.testing.assert_allclose(piv.astype(float), loco._cholesky_pivots(H), rtol=1e-12)
    r = rng.standard_normal(12)
    x = lc.solve_ld(H, r)
    assert float(np.max(np.abs(H.astype(np.longdouble) @ x - r))) <= 1e-17 * np.max(np.abs(r)) * np.linalg.cond(H)
    _, piv, ok = lc.cholesky_ld(np.diag([1.0, 0.0, 2.0]))
    assert not ok and piv.tolist() == [1.0, 0.0, 0.0]
    with pytest.raises(np.linalg.LinAlgError):
        lc.solve_ld(np.diag([1.0, -1.0]), np.ones(2))
    # the refit: J = K against the float64 downdated solve, J < K against lstsq in the projected features
    A, b, w, _ = lc.config_rows(4, 9, [30, 7, 12, 25])
    rows = np.arange(30, 37)
    np.testing.assert_allclose(lc.brute_force_ld(A, b, w, rows, 1e-4), lc.downdated(A, b, w, rows, 1e-4), rtol=0, atol=1e-12)
    Aw = A * w[:, None]
    M = loco.factor_eigen(Aw.T @ Aw, 0.0, rank=5)
    keep = np.setdiff1d(np.arange(len(b)), rows)
    gamma = np.linalg.lstsq(Aw[keep] @ M, (b * w)[keep], rcond=None)[0]
    np.testing.assert_allclose(lc.brute_force_ld(A, b, w, rows, 0.0, M), A[rows] @ M @ gamma, rtol=0, atol=1e-12)
    np.testing.assert_allclose(lc.Refit(A, b, w, 0.0, M, project_rows=True).predict(rows), A[rows] @ M @ gamma, rtol=0,
                               atol=1e-12)


def wrong_closed_form(A, b, w, M, beta, rows, off, defect):
    """loco_host's closed form with one defect: "zeta32" (zeta rounded through float32), "column" (the last column of M
    dropped) or "row" (the last row of each unit left out of the Gram matrix and the right-hand side, but predicted);
    None: no defect."""
    if defect == "column":
        M = M[:, :-1]
    J = M.shape[1]
    pred = np.full(len(b), np.nan)
    for c in range(len(off) - 1):
        r = rows[off[c]:off[c + 1]]
        zeta = A[r] @ M
        if defect == "zeta32":
            zeta = zeta.astype(np.float32).astype(np.float64)
        pb = A[r] @ beta
        Z = w[r, None] * zeta
        e = w[r] * b[r] - w[r] * pb
        if defect == "row":
            Z, e = Z[:-1], e[:-1]
        n = Z.shape[0]
        if n <= J:
            v = Z.T @ np.linalg.solve(np.eye(n) - Z @ Z.T, e)
        else:
            v = np.linalg.solve(np.eye(J) - Z.T @ Z, Z.T @ e)
        pred[r] = pb - zeta @ v
    return pred


@pytest.mark.parametrize("K", [31, 142, 150])
@pytest.mark.parametrize("alpha", lc.SWEEP_ALPHA)
def test_the_bars_of_the_kernel_tests_pass_loco_host_and_catch_three_defects(K, alpha):
    """The reduced sweep (the sizes and the J of tests/test_gpu_loco.py's sweep): loco_host passes the a-priori bar, the RMS
    condition and the pivot bound in every cell; a closed form with zeta through float32, without the last column of M, or
    without each unit's last row in the Gram matrix breaks the a-priori bar in every cell."""
    A, b, w, G, c, stats = lc.sweep_rows(K)
    m = len(b)
    rows = np.arange(m, dtype=np.int32)
    for J in lc.sweep_js(K):
        off, _ = lc.sweep_units(K, J, m)
        M, beta = lc.sweep_factor(G, c, alpha, J, stats)
        host, hinfo = loco.loco_host(A, b, w, M, beta, rows, off)
        res = lc.measure_cell(A, b, w, alpha, M, beta, rows, off, host, stats, host=host)
        print(lc.cell_line(f"host K={K} alpha={alpha:g} J={J}", res))
        assert np.min(res["lam_min"]) >= lc.LAM_MIN
        assert np.max(res["ratio"]) <= 1.0 and res["rms_pred"] <= lc.RMS_FACTOR * res["rms_host"]
        assert np.all(np.abs(hinfo[:, 1] - res["piv"]) <= 4 * (J + res["d"]) * lc.EPS)
        assert np.max(res["abs"]) <= 1e-9 * np.max(np.abs(b))
        same = wrong_closed_form(A, b, w, M, beta, rows, off, None)
        assert np.max(np.abs(same - host) / res["bar"]) <= 0.1          # the stand-in is the closed form
        for defect in ("zeta32", "column", "row"):
            wrong = wrong_closed_form(A, b, w, M, beta, rows, off, defect)
            excess = np.abs(wrong - res["truth"]) / res["bar"]
            assert np.max(excess) > 1.0, (defect, J, np.max(excess))
            # not one lucky row: the defect shows in most units
            bad = [np.max(excess[off[u]:off[u + 1]]) > 1.0 for u in range(len(off) - 1)]
            assert np.mean(bad) >= 0.5, (defect, J, np.mean(bad))


def test_factor_from_the_rows_triangle_where_the_statistics_are_too_ill_conditioned():
    # kappa(A_w) = 1e8: M^T G M = I holds for the factor from the rows, not for the eigenpairs of G (kappa^2 eps ~ 1)
    rng = np.random.default_rng(2)
    m, K = 1500, 12
    U, _ = np.linalg.qr(rng.standard_normal((m, K)))
    V, _ = np.linalg.qr(rng.standard_normal((K, K)))
    sv = np.ones(K)
    sv[-1] = 1e-8
    A = (U * sv) @ V.T
    w = rng.uniform(0.5, 2.0, m)
    b = A @ rng.standard_normal(K) + 1e-3 * rng.standard_normal(m)
    R = loco.rows_triangle(A, w)
    parts = [loco.rows_triangle(A[:400], w[:400]), loco.rows_triangle(A[400:], w[400:]), np.zeros((0, K))]
    Xl = (A * w[:, None]).astype(np.longdouble)
    for tri in (R, loco.rows_triangle(None, None, parts)):
        M = loco.factor_triangle(tri)
        T = Xl @ M.astype(np.longdouble)
        assert M.shape == (K, K) and float(np.max(np.abs(T.T @ T - np.eye(K)))) <= 1e-6
    assert loco.factor_triangle(R, rank=K - 1).shape == (K, K - 1)
    assert np.all(loco.factor_triangle(np.zeros((0, K))) == 0.0)
    # LOO predictions with it against the long-double refit in the projected features
    sizes = [1, 5, 12, 13, 40, 100] * 8 + [132]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = np.arange(m, dtype=np.int32)
    beta = np.linalg.lstsq(A * w[:, None], b * w, rcond=1e-13)[0]
    pred, info = loco.loco_host(A, b, w, M, beta, rows, off)
    refit = lc.Refit(A, b, w, 0.0, M, projected=True, project_rows=True)
    truth = np.concatenate([refit.predict(rows[off[u]:off[u + 1]]) for u in range(len(sizes))])
    assert np.all(info[:, 2] == 1.0)
    assert np.max(np.abs(pred - truth)) <= 1e-6 * np.max(np.abs(truth))

"""CPU: the host side of the influence vectors and cluster-robust covariances (fitsnap_amd/solvers/influence.py) -- the closed
forms of ``influence_host`` against long double under the a-priori bars of tests/influence_cases.py, the algebraic identities
(the exact refit, the jackknife from brute-force refits, the sandwich, White's HC0 / HC3), the statistical sanity case on the
reference, the tables and the covariance assembly on hand-made arrays, and the refusal paths."""
import os
import sys

import numpy as np
import pytest

from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import influence as infl
from fitsnap_amd.solvers import loco, loco_uq, solver_factory, uq

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import influence_cases as ic  # noqa: E402
import loco_cases as lc  # noqa: E402

LD = lc.LD


def make(name, d):
    pt = ParallelTools()
    return pt, solver_factory.solver(name, pt, Config(pt, d))


@pytest.mark.parametrize("alpha", [0.0, 1e-4])
@pytest.mark.parametrize("K", [1, 2, 17, 33, 64])
def test_host_closed_forms_sit_inside_every_bar_against_long_double(K, alpha):
    """float64 numpy against the long-double s_c, v_c, their norms, W_s and W_v over loco_cases' sweep of unit sizes: inside
    every a-priori bar, so the reference alone passes what the kernel is held to."""
    A, b, w, G, c, stats = lc.sweep_rows(K)
    m = len(b)
    rows = np.arange(m, dtype=np.int32)
    for J in ic.sweep_js(K):
        off, _ = lc.sweep_units(K, J, m)
        M, beta = lc.sweep_factor(G, c, alpha, J, stats)
        host = infl.influence_host(A, b, w, M, beta, rows, off)
        pred, info = loco.loco_host(A, b, w, M, beta, rows, off)
        assert np.array_equal(host["info"], info) and np.allclose(host["pred"], pred, rtol=0, atol=1e-12, equal_nan=True)
        assert np.all(host["info"][:, 2] == 1.0)
        scores = infl.influence_host(A, b, w, M, beta, rows, off, mode=infl.SCORES)
        assert np.array_equal(scores["S"], host["S"]) and np.array_equal(scores["Ws"], host["Ws"])
        assert scores["V"] is None and scores["Wv"] is None and scores["pred"] is None
        assert np.all(np.isnan(scores["unit"][:, [0, 2]])) and np.array_equal(scores["unit"][:, 1], host["unit"][:, 1])
        assert np.all(np.isinf(scores["info"][:, 1])) and np.array_equal(scores["info"][:, [0, 2, 3]], info[:, [0, 2, 3]])
        res = ic.measure_cell(A, b, w, M, beta, rows, off, host, host=host)
        ic.check_cell(f"host K={K} alpha={alpha:g} J={J}", res, factor=1.0)


def small_problem(seed, K, sizes, alpha):
    A, b, w, _ = lc.config_rows(seed, K, sizes)
    Aw, bw = A * w[:, None], b * w
    G, c = Aw.T @ Aw, Aw.T @ bw
    M = loco.factor_cholesky(G, alpha)
    beta = np.linalg.solve(G + alpha * np.eye(K), c)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return A, b, w, G, c, M, beta, off


def refit_betas(A, b, w, alpha, beta, off):
    """beta_{-c} - beta per unit from long-double refits without the unit (loco_cases.Refit's statistics; a solve per unit,
    not the Woodbury algebra); beta itself refitted in long double too."""
    rf = lc.Refit(A, b, w, alpha)
    full = lc.solve_ld(rf.Ga, rf.c)
    out = []
    for u in range(len(off) - 1):
        r = np.arange(off[u], off[u + 1])
        Xc = A[r].astype(LD) * rf.w[r, None]
        out.append(lc.solve_ld(rf.Ga - Xc.T @ Xc, rf.c - Xc.T @ rf.y[r]) - full)
    return np.array(out), full


@pytest.mark.parametrize("alpha", [0.0, 1e-3])
def test_influence_vectors_are_the_exact_refits_and_the_jackknife_is_theirs(alpha):
    K, sizes = 17, [30, 9, 17, 18, 25, 40, 12, 16, 33, 21, 50, 28]
    A, b, w, G, c, M, beta, off = small_problem(3, K, sizes, alpha)
    rows = np.arange(len(b), dtype=np.int32)
    host = infl.influence_host(A, b, w, M, beta, rows, off)
    assert np.all(host["info"][:, 2] == 1.0)
    delta, full = refit_betas(A, b, w, alpha, beta, off)
    scale = np.max(np.abs(full))
    np.testing.assert_allclose(-(host["V"] @ M.T), delta.astype(np.float64), rtol=0, atol=1e-10 * scale)
    # cov_jack assembled by the host layer against (U' - 1) / U' sum (beta_-c - beta)(...)^T from the brute-force refits
    U = len(sizes)
    cov = infl.covariances(M, host["Ws"], host["Wv"], 1.0, U, U, len(b), float(K), ("cr0", "cr1", "jack"))
    brute = ((U - 1) / U * (delta.T @ delta)).astype(np.float64)
    assert np.max(np.abs(cov["jack"] - brute)) <= 1e-10 * np.max(np.abs(brute))
    # cov_cr0 = C (sum_c X_c^T e_c e_c^T X_c) C, e the weighted residuals of the full fit
    C = np.linalg.inv(G + alpha * np.eye(K))
    X, e = A * w[:, None], w * (b - A @ beta)
    meat = sum(np.outer(X[off[u]:off[u + 1]].T @ e[off[u]:off[u + 1]], X[off[u]:off[u + 1]].T @ e[off[u]:off[u + 1]])
               for u in range(U))
    sand = C @ meat @ C
    assert np.max(np.abs(cov["cr0"] - sand)) <= 1e-10 * np.max(np.abs(sand))
    p = loco_uq.smoother_trace(G, M)
    np.testing.assert_allclose(cov["cr1"], U / (U - 1) * (len(b) - 1) / (len(b) - K) * cov["cr0"], rtol=1e-14)
    assert abs(p - K) < 1e-8 if alpha == 0.0 else p < K
    # Cook's distance through the unit records: |v_c|^2 / (p sigma^2) = dbeta^T (G + alpha I) dbeta / (p sigma^2)
    live, Uc, Uid, n = infl.unit_counts(w, rows, off, host["info"])
    assert (Uc, Uid, n) == (U, U, len(b)) and live.tolist() == sizes
    recs = infl.unit_records([f"u{u}" for u in range(U)], ["g"] * len(b), live, rows, off, host["info"], host["unit"], 0.3, p)
    d64 = delta.astype(np.float64)
    cook = np.einsum("ck,kl,cl->c", d64, G + alpha * np.eye(K), d64) / (p * 0.3)
    np.testing.assert_allclose([r[7] for r in recs], cook, rtol=1e-8)
    np.testing.assert_allclose([r[8] for r in recs], host["unit"][:, 0], rtol=0)


def test_one_row_per_unit_gives_whites_hc0_and_hc3():
    K, n = 6, 60
    A, b, w, G, c, M, beta, off = small_problem(11, K, [1] * n, 0.0)
    host = infl.influence_host(A, b, w, M, beta, np.arange(n, dtype=np.int32), off)
    assert np.all(host["info"][:, 3] == 1.0)                       # one row <= J: n space
    cov = infl.covariances(M, host["Ws"], host["Wv"], 1.0, n, n, n, float(K), ("cr0", "jack"))
    X, e = A * w[:, None], w * (b - A @ beta)
    C = np.linalg.inv(G)
    h = np.einsum("ik,kl,il->i", X, C, X)
    hc0 = C @ (X.T * e ** 2) @ X @ C
    hc3 = C @ (X.T * (e / (1 - h)) ** 2) @ X @ C
    np.testing.assert_allclose(cov["cr0"], hc0, rtol=1e-10, atol=1e-14 * np.max(np.abs(hc0)))
    np.testing.assert_allclose(cov["jack"], (n - 1) / n * hc3, rtol=1e-10, atol=1e-14 * np.max(np.abs(hc3)))


def test_edge_units_empty_zero_weight_and_not_identifiable():
    A, b, w, G, c, off = ic.edge_problem(0.0)
    M, beta = ic.edge_factor(G, c, 0.0, 33)
    rows = np.arange(off[-2], dtype=np.int32)
    host = infl.influence_host(A, b, w, M, beta, rows, off[:-1])
    assert host["info"][1].tolist() == [0, np.inf, 1, 1] and not host["unit"][1].any() and not host["S"][1].any()
    assert host["info"][2, 2] == 0.0 and not host["V"][2].any() and np.all(np.isfinite(host["S"][2])) and host["S"][2].any()
    assert np.isnan(host["unit"][2, 0]) and np.isnan(host["unit"][2, 2]) and host["unit"][2, 1] > 0
    np.testing.assert_allclose(host["Ws"], sum(np.outer(s, s) for s in host["S"]), rtol=1e-12, atol=1e-18)
    good = [0, 3, 4, 5]
    np.testing.assert_allclose(host["Wv"], sum(np.outer(host["V"][u], host["V"][u]) for u in good), rtol=1e-12, atol=1e-18)
    live, U, Uid, n = infl.unit_counts(w, rows, off[:-1], host["info"])
    assert live.tolist() == [18, 0, 40, 33, 34, 70] and (U, Uid, n) == (5, 4, 195)


def test_the_clustered_sanity_case_holds_on_the_reference():
    """Seed influence_cases.CLUSTER_SEED: with a per-unit random effect the cluster-robust standard errors exceed the classical
    ones on every coefficient, and cov_jack >= cov_cr0 in the Loewner order."""
    A, b, w, labels = ic.clustered_problem()
    G, c = A.T @ A, A.T @ b
    M = loco.factor_cholesky(G, 0.0)
    beta = np.linalg.solve(G, c)
    rows, off, units = loco.unit_index(labels["Configs"], np.ones(len(b), dtype=bool))
    host = infl.influence_host(A, b, w, M, beta, rows, off)
    res = b - A @ beta
    cov = infl.covariances(M, host["Ws"], host["Wv"], (res @ res) / (len(b) - 17), 400, 400, len(b), 17.0, ("cr0", "cr1", "jack"))
    frame = infl.stderr_frame(beta, cov)
    assert np.all(frame["ratio_cr1"].to_numpy() > 1.0)
    gap = np.linalg.eigvalsh(cov["jack"] - cov["cr0"])
    assert gap[0] >= -1e-12 * np.max(np.abs(np.linalg.eigvalsh(cov["jack"])))


def test_covariance_kinds_tables_and_b0_handling():
    rng = np.random.default_rng(5)
    M = rng.standard_normal((4, 3))
    Ws, Wv = np.diag([1.0, 2.0, 3.0]), np.diag([2.0, 2.0, 5.0])
    cov = infl.covariances(M, Ws, Wv, 0.5, 10, 8, 100, 3.0, ())
    assert list(cov) == ["classical"] and np.allclose(cov["classical"], 0.5 * M @ M.T)
    cov = infl.covariances(M, Ws, Wv, 0.5, 10, 8, 100, 3.0, ("jack", "cr0"))
    assert sorted(cov) == ["classical", "cr0", "jack"]
    np.testing.assert_allclose(cov["cr0"], M @ Ws @ M.T, rtol=1e-14)
    np.testing.assert_allclose(cov["jack"], 7 / 8 * M @ Wv @ M.T, rtol=1e-14)
    cr1 = infl.covariances(M, Ws, Wv, 0.5, 10, 8, 100, 3.0, ("cr1",))
    assert sorted(cr1) == ["classical", "cr1"]
    np.testing.assert_allclose(cr1["cr1"], 10 / 9 * 99 / 97 * M @ Ws @ M.T, rtol=1e-14)
    assert np.all(np.isnan(infl.covariances(M, Ws, Wv, 0.5, 1, 1, 100, 3.0, ("cr1",))["cr1"]))
    assert np.all(np.isnan(infl.covariances(M, Ws, Wv, 0.5, 3, 0, 100, 3.0, ("jack",))["jack"]))
    with pytest.raises(ValueError, match="kind"):
        infl.covariances(M, Ws, Wv, 0.5, 10, 8, 100, 3.0, ("cr2",))
    # the table takes the fit as the rows see it: the B0 zeros of _offset are taken out as uq.strip_b0 does, so that beta and
    # the K x K covariances have the same columns
    fit = np.array([0.0, 1.0, 2.0, 0.0, 3.0, 4.0])                 # two types, B0 in front of each
    beta = uq.strip_b0(fit, 2, 2)
    frame = infl.stderr_frame(beta, cov)
    assert list(frame.columns) == ["beta", "se_classical", "se_cr0", "se_jack", "ratio_cr0", "ratio_jack"]
    assert frame["beta"].tolist() == [1.0, 2.0, 3.0, 4.0] and len(frame) == 4
    np.testing.assert_allclose(frame["ratio_jack"], np.sqrt(np.diag(cov["jack"]) / np.diag(cov["classical"])), rtol=1e-14)
    with pytest.raises(ValueError, match="mode"):
        infl.influence_host(np.zeros((2, 4)), np.zeros(2), np.ones(2), M, np.zeros(4), [0, 1], [0, 2], mode=2)


@pytest.mark.parametrize("name", ["ARD", "LASSO"])
def test_solvers_that_are_not_linear_smoothers_are_refused(name):
    _, s = make(name, {"SOLVER": {"solver": name}})
    with pytest.raises(ValueError, match="influence: .* is not a linear smoother"):
        s.influence()


@pytest.mark.parametrize("name", ["SVD", "RIDGE", "ANL"])
def test_apply_transpose_unknown_kinds_and_methods_are_refused(name):
    _, s = make(name, {"SOLVER": {"solver": name}, "EXTRAS": {"apply_transpose": 1}})
    with pytest.raises(ValueError, match="apply_transpose"):
        s.influence()
    _, s = make(name, {"SOLVER": {"solver": name}})
    with pytest.raises(ValueError, match="method"):
        s.influence(method="refit")
    with pytest.raises(ValueError, match="kind"):
        s.influence(kinds=("cr2",))
    cov = np.eye(3) * 2.0
    s.use_covariance(cov)
    assert np.array_equal(s.cov, cov) and s.cov.flags.c_contiguous

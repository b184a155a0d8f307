"""CPU: the host side of the leave-one-configuration-out predictive variances (fitsnap_amd/solvers/loco_uq.py) -- the closed
forms of ``loco_uq_host`` (leverages, joint distances, log-determinants, predictions; n space and J space) against explicit
long-double refits without each unit (tests/loco_uq_cases.py), the calibration of a correctly specified model on a fixed
seed, the tables and the summary on hand-made arrays, the noise resolution and the refusal paths."""
import os
import sys

import numpy as np
import pytest

from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import loco, loco_uq, solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loco_cases as lc  # noqa: E402
import loco_uq_cases as uc  # noqa: E402


def cell_js(K):
    return [J for J in lc.sweep_js(K) if J in (K, 1, 15, K - 1)]


@pytest.mark.parametrize("alpha", lc.SWEEP_ALPHA)
@pytest.mark.parametrize("K", [1, 2, 17, 33, 64])
def test_closed_forms_match_long_double_refits(K, alpha):
    """q_i, D_c, l_c and the predictions of loco_uq_host on the sweep of loco_cases (every boundary unit size, J = K and
    J < K) against refits without the unit in long double, each under its a-priori bar; then both spaces forced on the
    units where the other one is the kernel's choice: the same numbers from the other formula."""
    A, b, w, G, c, stats = lc.sweep_rows(K)
    m = len(b)
    rows = np.arange(m, dtype=np.int32)
    for J in cell_js(K):
        off, _ = lc.sweep_units(K, J, m)
        M, beta = lc.sweep_factor(G, c, alpha, J, stats)
        host = loco_uq.loco_uq_host(A, b, w, M, beta, rows, off)
        pred, lev, info = host
        tag = f"host K={K} alpha={alpha:g} J={J}"
        res = uc.measure_cell(A, b, w, alpha, M, beta, rows, off, lev, info, stats, None, host)
        print(uc.cell_line(tag, res))
        n = np.diff(off)
        assert np.all(info[:, 2] == 1.0) and np.array_equal(info[:, 0], np.minimum(n, J))
        assert np.array_equal(info[:, 3], (n <= J).astype(float))
        assert np.min(res["lam_min"]) >= lc.LAM_MIN
        for k in ("q", "d", "l"):
            assert np.max(res["ratio_" + k]) <= 1.0, (tag, k, np.max(res["ratio_" + k]))
        assert np.max(np.abs(pred - res["truth_pred"])) <= 1e-9 * np.max(np.abs(b)), tag
        assert np.array_equal(pred, loco.loco_host(A, b, w, M, beta, rows, off)[0])
        # the other space on the same units: every unit of at most 129 rows (an n x n matrix per unit in n space)
        small = np.flatnonzero(n <= 129)
        soff = np.concatenate([[0], np.cumsum(n[small])]).astype(np.int64)
        srows = np.concatenate([rows[off[u]:off[u + 1]] for u in small]).astype(np.int32)
        pn, qn, infn = loco_uq.loco_uq_host(A, b, w, M, beta, srows, soff, space="n")
        pj, qj, infj = loco_uq.loco_uq_host(A, b, w, M, beta, srows, soff, space="J")
        assert np.all(infn[:, 3] == 1.0) and np.all(infj[:, 3] == 0.0)
        for i, u in enumerate(small):
            r = srows[soff[i]:soff[i + 1]]
            mid = lc.unit_reference(A, b, w, r, M, beta, precise=False)
            bq, bd, bl = uc.uq_bars(A[r], b[r], w[r], M, beta, mid["lam_min"], max(len(r), J), w[r] * (b[r] - pn[r]),
                                    infn[i, 4])
            assert np.all(np.abs(qn[r] - qj[r]) <= 2 * bq), (tag, u)
            assert abs(infn[i, 5] - infj[i, 5]) <= 2 * bd, (tag, u)
            assert abs(infn[i, 4] - infj[i, 4]) <= 2 * bl, (tag, u)          # Sylvester: one log-determinant, two matrices
            assert np.all(np.abs(pn[r] - pj[r]) <= 1e-9 * np.max(np.abs(b)))


def test_the_diagonal_identity_and_the_unidentifiable_and_empty_units():
    A, b, w, labels = lc.config_rows(11, 6, [10, 12, 0, 9, 14])
    cfg = np.asarray(labels["Configs"])
    Aw, bw = A * w[:, None], b * w
    G = Aw.T @ Aw
    beta = np.linalg.solve(G + 1e-4 * np.eye(6), Aw.T @ bw)
    off = np.array([0, 10, 22, 22, 31, 45])
    rows = np.arange(45, dtype=np.int32)
    M = loco.factor_cholesky(G, 1e-4)
    pred, lev, info = loco_uq.loco_uq_host(A, b, w, M, beta, rows, off, space="n")
    assert info[2].tolist() == [0, np.inf, 1, 1, 0, 0]
    for u in (0, 1, 3, 4):
        r = rows[off[u]:off[u + 1]]
        Z = w[r, None] * (A[r] @ M)
        Hinv = np.linalg.inv(np.eye(len(r)) - Z @ Z.T)
        np.testing.assert_allclose(w[r] ** 2 * lev[r], np.diag(Hinv) - 1.0, rtol=0, atol=1e-12)   # the form that cancels
        np.testing.assert_allclose(info[u, 4], np.linalg.slogdet(np.eye(len(r)) - Z @ Z.T)[1], rtol=0, atol=1e-12)
    # a column that unit 1 alone touches: without a ridge the fit without it cannot see the column
    A[:, 5] = 0.0
    A[cfg == "cfg1", 5] = 1.0 + 0.1 * np.arange(12)
    Aw = A * w[:, None]
    G = Aw.T @ Aw
    beta = np.linalg.solve(G, Aw.T @ bw)
    pred, lev, info = loco_uq.loco_uq_host(A, b, w, loco.factor_cholesky(G), beta, rows, off)
    assert info[1, 2] == 0.0 and np.all(np.isnan(info[1, 4:])) and np.all(np.isnan(lev[10:22])) and np.all(np.isnan(pred[10:22]))
    assert np.all(np.isfinite(lev[:10])) and np.all(np.isfinite(info[[0, 3, 4], 4:]))


def calibration_problem():
    """K = 12, 200 units of 1 ... 29 rows, weights in [0.5, 2], noise sigma / w_i with sigma = 0.3, ridge alpha = 1e-6."""
    rng = np.random.default_rng(0)
    K, sigma, alpha = 12, 0.3, 1e-6
    sizes = rng.integers(1, 30, 200)
    m = int(sizes.sum())
    A = rng.standard_normal((m, K))
    w = rng.uniform(0.5, 2.0, m)
    b = A @ rng.standard_normal(K) + sigma * rng.standard_normal(m) / w
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    Aw, bw = A * w[:, None], b * w
    G, c = Aw.T @ Aw, Aw.T @ bw
    beta = np.linalg.solve(G + alpha * np.eye(K), c)
    return A, b, w, off, G, c, np.array([bw @ bw, bw.sum(), m]), beta, loco.factor_cholesky(G, alpha), sigma


def test_a_correctly_specified_model_is_calibrated():
    """Fixed seed, 3 187 rows: mean z^2 and sum D_c / (n sigma^2) within 4 standard deviations sqrt(2 / 3187) = 0.025 of 1
    ([0.9, 1.1]), the coverages within 0.03 (more than 3 standard deviations sqrt(p (1 - p) / 3187) <= 0.0083) of nominal."""
    A, b, w, off, G, c, s, beta, M, sigma = calibration_problem()
    m = len(b)
    assert m == 3187
    rows = np.arange(m, dtype=np.int32)
    noise = loco_uq.resolve_noise("RIDGE", None, None, (G, c, s), beta, M)
    assert abs(noise / sigma ** 2 - 1.0) < 0.1
    pred, lev, info = loco_uq.loco_uq_host(A, b, w, M, beta, rows, off)
    var, z, nlpd = loco_uq.row_stats(b, w, pred, lev, noise)
    print(f"mean z^2 {np.mean(z * z):.4f}  coverage {np.mean(np.abs(z) <= 1):.4f} / {np.mean(np.abs(z) <= 2):.4f}  "
          f"D ratio {info[:, 5].sum() / (m * noise):.4f}")
    assert 0.9 <= np.mean(z * z) <= 1.1
    assert 0.9 <= info[:, 5].sum() / (m * noise) <= 1.1
    assert abs(np.mean(np.abs(z) <= 1.0) - loco_uq.NOMINAL_1) <= 0.03
    assert abs(np.mean(np.abs(z) <= 2.0) - loco_uq.NOMINAL_2) <= 0.03
    np.testing.assert_allclose(var, noise * (1.0 / w ** 2 + lev), rtol=1e-14)
    # the joint density of a unit of one row is its marginal density
    units = [f"u{i}" for i in range(len(off) - 1)]
    recs = loco_uq.unit_records(units, ["g"] * m, w, rows, off, info, noise)
    for u in np.flatnonzero(np.diff(off) == 1)[:5]:
        np.testing.assert_allclose(recs[u][8], -nlpd[off[u]], rtol=1e-12)
    keys, st = loco_uq.table_sums(z, nlpd, ["g"] * m, ["Energy"] * m)
    out = loco_uq.summary(recs, st)
    np.testing.assert_allclose(out["calibrated_noise"] * noise, info[:, 5].sum() / m, rtol=1e-14)
    np.testing.assert_allclose(out["logdens"], sum(r[8] for r in recs), rtol=1e-14)


def test_tables_and_summary_on_hand_made_arrays():
    b = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])
    pred = np.array([0.5, 2.0, 2.0, 4.5, np.nan, np.nan, 7.0, 5.0])       # rows 4, 5: a unit that is not identifiable
    lev = np.array([0.0, 3.0, 0.0, 3.0, np.nan, np.nan, 1.0, 0.0])
    w = np.array([1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 0.0, 1.0])               # row 6: weight 0
    noise = 0.25
    var, z, nlpd = loco_uq.row_stats(b, w, pred, lev, noise)
    np.testing.assert_allclose(var[[0, 1, 2, 3, 7]], [0.25, 1.0, 0.0625, 1.0, 0.25])
    np.testing.assert_allclose(z[[0, 1, 2, 3, 7]], [1.0, 0.0, 4.0, -0.5, 6.0])
    assert np.all(np.isnan(var[[4, 5, 6]])) and np.all(np.isnan(z[[4, 5, 6]]))
    np.testing.assert_allclose(nlpd[0], 0.5 * (np.log(2 * np.pi * 0.25) + 1.0))
    groups = ["g0", "g0", "g1", "g1", "g1", "g1", "g0", "g0"]
    rtypes = ["Energy", "Force", "Energy", "Force", "Force", "Force", "Force", "Force"]
    keys, st = loco_uq.table_sums(z, nlpd, groups, rtypes)
    assert keys == [("g0", "Energy"), ("g0", "Force"), ("g1", "Energy"), ("g1", "Force")]
    assert st[:, 0].tolist() == [1, 2, 1, 1]                  # the zero-weight row and the NaN rows are not counted
    t = loco_uq.tables_frame(keys, st)
    assert list(t.columns) == loco_uq.TABLE_COLUMNS
    assert list(t.index) == [("*ALL", "Energy"), ("*ALL", "Force"), ("*ALL", "*ALL")] + keys
    assert t.loc[("*ALL", "*ALL"), "n"] == 5
    np.testing.assert_allclose(t.loc[("*ALL", "*ALL"), "mean_z2"], (1 + 0 + 16 + 0.25 + 36) / 5)
    np.testing.assert_allclose(t.loc[("*ALL", "Force"), ["within_1", "within_2"]].to_numpy(dtype=float), [2 / 3, 2 / 3])
    np.testing.assert_allclose(t.loc[("g0", "Force"), "mean_z2"], 18.0)
    assert t.loc[("g1", "Energy"), "nominal_1"] == loco_uq.NOMINAL_1 and t.loc[("g1", "Energy"), "nominal_2"] == loco_uq.NOMINAL_2
    np.testing.assert_allclose(t.loc[("*ALL", "*ALL"), "nlpd"], np.nansum(nlpd) / 5)
    # units: rows (0, 1, 6), (2, 3), (4, 5) not identifiable, (7), and an empty one
    rows = np.array([0, 1, 6, 2, 3, 4, 5, 7], dtype=np.int32)
    off = np.array([0, 3, 5, 7, 8, 8])
    info = np.array([[3, 0.5, 1, 1, -0.7, 2.0], [2, 0.4, 1, 1, -0.3, 1.0], [2, 1e-12, 0, 1, np.nan, np.nan],
                     [1, 1.0, 1, 1, 0.0, 9.0], [0, np.inf, 1, 1, 0.0, 0.0]])
    recs = loco_uq.unit_records(["a", "b", "c", "d", "e"], groups, w, rows, off, info, noise)
    assert [r[2] for r in recs] == [3, 2, 2, 1, 0] and [r[3] for r in recs] == [2, 2, 2, 1, 0]
    assert [r[5] for r in recs] == [True, True, False, True, True]
    np.testing.assert_allclose(recs[0][6:], [8.0, -0.7, -0.5 * (2 * np.log(2 * np.pi * 0.25) + 0.7 + 8.0)])
    np.testing.assert_allclose(recs[1][8], -0.5 * (2 * np.log(2 * np.pi * 0.25) + 0.3 + 4.0) + np.log(2.0))
    assert np.all(np.isnan(recs[2][6:])) and recs[4][6:] == (0.0, 0.0, 0.0) and recs[4][1] is None
    out = loco_uq.summary(recs, st)
    assert out["units"] == 5 and out["unidentifiable"] == 1
    np.testing.assert_allclose(out["calibrated_noise"], (8.0 + 4.0 + 36.0) / 5)
    np.testing.assert_allclose(out["logdens"], recs[0][8] + recs[1][8] + recs[3][8])
    np.testing.assert_allclose(out["mean_z2"], 53.25 / 5)


def make(name, sections):
    pt = ParallelTools()
    return pt, solver_factory.solver(name, pt, Config(pt, sections))


def test_noise_resolution():
    A, b, w, off, G, c, s, beta, M, sigma = calibration_problem()
    assert loco_uq.resolve_noise("ANL", None, 0.125, None, beta, M) == 0.125
    assert loco_uq.resolve_noise("ANL", 0.5, 0.125, None, beta, M) == 0.5             # an explicit value wins
    res = w * (b - A @ beta)
    trace = np.trace(G @ np.linalg.inv(G + 1e-6 * np.eye(12)))
    np.testing.assert_allclose(loco_uq.smoother_trace(G, M), trace, rtol=1e-10)
    np.testing.assert_allclose(loco_uq.resolve_noise("RIDGE", None, None, (G, c, s), beta, M),
                               (res @ res) / (len(b) - trace), rtol=1e-9)
    np.testing.assert_allclose(loco_uq.resolve_noise("SVD", None, 7.0, (G, c, s), beta, M), (res @ res) / (len(b) - trace),
                               rtol=1e-9)
    few = np.array([s[0], s[1], 11.0])                     # fewer training rows than the fit spends: nothing left for the noise
    with pytest.raises(ValueError, match="degrees of freedom"):
        loco_uq.resolve_noise("RIDGE", None, None, (G, c, few), beta, M)
    for bad in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="not positive"):
            loco_uq.resolve_noise("RIDGE", bad, None, (G, c, s), beta, M)
    with pytest.raises(RuntimeError, match="perform_fit"):
        loco_uq.resolve_noise("ANL", None, None, None, beta, M)


@pytest.mark.parametrize("name", ["ARD", "LASSO", "MERR", "MCMC"])
def test_solvers_that_are_not_linear_smoothers_are_refused(name):
    _, s = make(name, {"SOLVER": {"solver": name}})
    with pytest.raises(ValueError, match="loco_predictive: .* is not a linear smoother"):
        s.loco_predictive()


@pytest.mark.parametrize("name", ["SVD", "RIDGE", "ANL"])
def test_apply_transpose_and_an_unknown_method_are_refused(name):
    _, s = make(name, {"SOLVER": {"solver": name}, "EXTRAS": {"apply_transpose": 1}})
    with pytest.raises(ValueError, match="apply_transpose"):
        s.loco_predictive()
    _, s = make(name, {"SOLVER": {"solver": name}})
    with pytest.raises(ValueError, match="method"):
        s.loco_predictive(method="refit")

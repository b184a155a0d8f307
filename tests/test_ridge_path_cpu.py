"""CPU: the host side of the leave-one-unit-out ridge alpha path (fitsnap_amd/solvers/ridge_path.py) -- ridge_path_host
against the long-double refit of tests/loco_cases.py on the boundary units, the table assembly, the rule for ``best``, the
refusals and the interior-minimum case."""
import os
import sys
import types

import numpy as np
import pytest

from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import ridge_path as rp
from fitsnap_amd.solvers import solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loco_cases as lc  # noqa: E402
import ridge_path_cases as rc  # noqa: E402


def make(name, sections):
    pt = ParallelTools()
    return pt, solver_factory.solver(name, pt, Config(pt, sections))


@pytest.mark.parametrize("K", [1, 2, 17, 64])
def test_host_form_matches_the_long_double_refit_on_the_boundary_units(K):
    """ridge_path_host against loco_cases.Refit(A, b, w, alpha).predict on the boundary-size units of the sweep, alpha in
    {0, 1e-8, 1e-4, 1, 1e2}: relative error <= 1e-13 (measured: 5e-15 at worst), no unit flagged, smallest scaled pivot
    >= 0.8 (measured: 0.83)."""
    lc.need_long_double()
    A, b, w, G, c, stats = lc.sweep_rows(K)
    m = len(b)
    off, boundary = lc.sweep_units(K, K, m)
    rows = np.arange(m, dtype=np.int32)
    sums, info, preds = rp.ridge_path_host(A, b, w, G, c, rc.ALPHAS, rows, off, rc.row_classes(m), rc.NCLASS)
    assert np.all(info[:, :, 1] == 1.0)
    assert np.min(info[:, :, 0]) >= 0.8
    worst = 0.0
    for q, alpha in enumerate(rc.ALPHAS):
        refit = lc.Refit(A, b, w, alpha, stats=stats)
        for u in np.flatnonzero(boundary):
            r = rows[off[u]:off[u + 1]]
            truth = refit.predict(r)
            worst = max(worst, float(np.max(np.abs(preds[q, r] - truth)) / np.max(np.abs(b))))
            own = rc.own_sums(b, w, preds[q], r, rc.row_classes(m), rc.NCLASS)
            assert np.all(np.abs(sums[q, u] - own) <= 4 * len(r) * lc.EPS * np.abs(own) + 1e-300)
    print(f"K={K}: worst relative error of ridge_path_host {worst:.3g}; smallest pivot {np.min(info[:, :, 0]):.3g}")
    assert worst <= 1e-13


def test_bar_passes_the_host_form_and_catches_a_wrong_downdate():
    """The a-priori bar of the kernel tests on ridge_path_host itself (K = 17 cell): every row within it; a variant that
    leaves each unit's last row out of G_u is far outside it."""
    lc.need_long_double()
    K = 17
    A, b, w, G, c, stats = lc.sweep_rows(K)
    m = len(b)
    off, boundary = lc.sweep_units(K, K, m)
    rows = np.arange(m, dtype=np.int32)
    _, _, preds = rp.ridge_path_host(A, b, w, G, c, rc.ALPHAS, rows, off)
    res = rc.measure(A, b, w, stats, rows, off, rc.ALPHAS, preds, preds)
    assert np.max(res["ratio"]) <= 1.0, np.max(res["ratio"])
    wrong = np.full_like(preds, np.nan)
    for u in range(len(off) - 1):
        r = rows[off[u]:off[u + 1]]
        if len(r) < 2:
            wrong[:, r] = preds[:, r]
            continue
        sub = np.array([0, len(r) - 1])
        _, _, p = rp.ridge_path_host(A, b, w, G, c, rc.ALPHAS, r[:-1], sub)
        wrong[:, r[:-1]] = p[:, r[:-1]]
        wrong[:, r[-1]] = preds[:, r[-1]]
    bad = rc.measure(A, b, w, stats, rows, off, rc.ALPHAS, wrong, preds)
    assert np.max(bad["ratio"]) > 1e3


def test_table_assembly_from_hand_made_sums():
    alphas = np.array([0.0, 0.5])
    # two units, two classes: (n, sum |r|, sum r^2, sum (w r)^2)
    sums = np.zeros((2, 2, 2, 4))
    sums[0, 0, 0] = (2, 3.0, 5.0, 20.0)
    sums[0, 0, 1] = (1, 1.0, 1.0, 4.0)
    sums[0, 1, 0] = (2, 1.0, 1.0, 1.0)
    sums[1, 0, 0] = (2, 2.0, 4.0, 16.0)
    sums[1, 1, 0] = (2, 100.0, 100.0, 100.0)          # not identifiable at alpha = 0.5: must not be pooled
    info = np.ones((2, 2, 2))
    info[1, 1, 1] = 0.0
    pooled, bad = rp.pool_sums(sums, info)
    assert bad.tolist() == [0, 1]
    assert pooled[0, 0].tolist() == [4, 4.0, 6.0, 21.0] and pooled[1, 0].tolist() == [2, 2.0, 4.0, 16.0]
    t = rp.path_table(alphas, pooled, ["Energy", "Force"])
    assert list(t.index) == [(0.0, "*ALL"), (0.0, "Energy"), (0.0, "Force"), (0.5, "*ALL"), (0.5, "Energy"), (0.5, "Force")]
    row = t.loc[(0.0, "*ALL")]
    assert row["ncount"] == 5 and row["mae"] == 1.0 and row["rmse"] == np.sqrt(7.0 / 5) and row["w_rmse"] == np.sqrt(5.0)
    row = t.loc[(0.0, "Energy")]
    assert row["ncount"] == 4 and row["mae"] == 1.0 and row["rmse"] == np.sqrt(1.5) and row["w_rmse"] == np.sqrt(21.0 / 4)
    assert t.loc[(0.5, "Force")]["ncount"] == 0 and np.isnan(t.loc[(0.5, "Force")]["rmse"])
    assert t.loc[(0.5, "*ALL")]["w_rmse"] == np.sqrt(8.0)


def test_best_takes_the_smallest_sum_the_smaller_alpha_on_ties_and_no_ineligible_alpha():
    a = np.array([1e-2, 1e-6, 1.0, 1e2])
    none = np.zeros(4, dtype=int)
    assert rp.pick_best(a, np.array([3.0, 2.0, 1.0, 4.0]), none) == 2
    assert rp.pick_best(a, np.array([1.0, 1.0, 1.0, 4.0]), none) == 1                 # tie: the smaller alpha
    assert rp.pick_best(a, np.array([3.0, 2.0, 1.0, 4.0]), np.array([0, 0, 1, 0])) == 1   # the minimum is not eligible
    assert rp.pick_best(a, np.array([3.0, 2.0, 1.0, 4.0]), np.ones(4, dtype=int)) is None
    assert rp.pick_best(a, np.array([np.nan, 2.0, np.nan, 4.0]), none) == 1
    assert rp.pick_best(np.array([0.5, 0.5]), np.array([1.0, 1.0]), none[:2]) == 0   # duplicates: the first


@pytest.mark.parametrize("name", ["ARD", "LASSO", "ANL", "MERR"])
def test_other_solvers_are_refused(name):
    _, s = make(name, {"SOLVER": {"solver": name}})
    with pytest.raises(ValueError, match="has no ridge path"):
        s.ridge_path([1e-8, 1e-4])


@pytest.mark.parametrize("name", ["RIDGE", "SVD"])
def test_apply_transpose_is_refused(name):
    _, s = make(name, {"SOLVER": {"solver": name}, "EXTRAS": {"apply_transpose": 1}})
    with pytest.raises(ValueError, match="apply_transpose"):
        s.ridge_path([1e-8])


def test_row_space_fits_bad_grids_and_bad_methods_are_refused():
    _, s = make("SVD", {"SOLVER": {"solver": "SVD"}})
    s.last_row_space = {"passes": 2}
    with pytest.raises(ValueError, match="row-space"):
        s.ridge_path([1e-8])
    _, s = make("RIDGE", {"SOLVER": {"solver": "RIDGE"}})
    for grid in ([], [-1.0], [np.nan], [np.inf, 1.0]):
        with pytest.raises(ValueError):
            s.ridge_path(grid)
    with pytest.raises(ValueError, match="method"):
        s.ridge_path([1.0], method="fast")
    with pytest.raises(RuntimeError, match="perform_fit"):
        s.ridge_path([1.0])
    with pytest.raises(ValueError, match="K <= 144"):
        rp.choose_method("refit", 145)
    assert rp.choose_method("auto", 144) == "refit" and rp.choose_method("auto", 145) == "woodbury"


def test_rows_that_are_not_those_of_the_fit_are_refused():
    # a solver with statistics of K = 3 and a context that holds other rows: refused before any GPU call
    _, s = make("RIDGE", {"SOLVER": {"solver": "RIDGE"}})
    s.last_statistics = (np.eye(3), np.ones(3), None)
    s.pt.hip = lambda: types.SimpleNamespace(m=7, K=3)
    fs = {"Configs": ["a", "a", "b", "b"], "Groups": ["g"] * 4, "Testing": [False] * 4, "Row_Type": ["Energy"] * 4}
    with pytest.raises(ValueError, match="not those of the fit"):
        s.ridge_path([1.0], fs_dict=fs, b=np.zeros(4), w=np.ones(4))
    with pytest.raises(ValueError, match="pass the truths"):
        s.ridge_path([1.0], fs_dict=fs)
    s.pt.hip = lambda: types.SimpleNamespace(m=4, K=4)
    with pytest.raises(ValueError, match="not those of the fit"):
        s.ridge_path([1.0], fs_dict=fs, b=np.zeros(4), w=np.ones(4))


def test_interior_minimum_of_the_loo_curve():
    A, b, w, labels, alphas = rc.interior_case()
    sums, info, preds, rows, off, units, names, cls = rc.host_path(A, b, w, alphas, labels)
    pooled, bad = rp.pool_sums(sums, info)
    assert not bad.any()
    curve = pooled[:, :, 3].sum(axis=1)
    best = rp.pick_best(alphas, curve, bad)
    assert alphas[best] == 10.0
    # the recorded curve, to the digits it was recorded with
    assert np.all(np.abs(curve[[0, 7, 8]] - [1049.47, 972.29, 1777.9]) <= [0.005, 0.005, 0.05]), curve
    assert curve[7] < curve[6] and curve[7] < curve[8]
    t = rp.path_table(alphas, pooled, names)
    assert t.loc[(10.0, "*ALL")]["ncount"] == 60
    assert t.loc[(10.0, "*ALL")]["w_rmse"] == np.sqrt(curve[7] / 60)


def test_a_unit_that_alone_touches_a_column_is_flagged_at_alpha_zero_only():
    A, b, w, labels = lc.config_rows(11, 31, [30, 25, 40, 35, 50, 45])
    cfg = np.asarray(labels["Configs"])
    A[:, 7] = 0.0
    A[cfg == "cfg2", 7] = 1.0 + 0.05 * np.arange(40)
    sums, info, preds, rows, off, units, names, cls = rc.host_path(A, b, w, [0.0, 1e-4], labels)
    u = units.index("cfg2")
    assert info[0, u, 1] == 0.0 and np.all(np.delete(info[0, :, 1], u) == 1.0) and np.all(info[1, :, 1] == 1.0)
    assert np.all(np.isnan(preds[0, cfg == "cfg2"])) and np.all(np.isfinite(preds[0, cfg != "cfg2"]))
    assert np.all(sums[0, u] == 0.0) and np.all(np.isfinite(preds[1]))

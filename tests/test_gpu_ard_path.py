"""GPU: grouped K-fold ARD threshold paths (fsnap_ard_path, csrc/fsnap_ard.hip; Solver.ard_path) under the acceptance of
tests/ard_path_cases.py: every problem is admitted by its decision margins along the long-double trace (oracle C), then the
kernel must EQUAL the host route (oracle A) and oracle C in support, iteration count and status and stay within the measured
bars in coefficients, lambdas, info and held-out sums; geometry, edges, more problems than compute units, determinism,
argument checks and side effects, the solver surface on the Ta rows against scikit-learn refits (oracle D), two ranks, the
example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import ard_path as ap
from fitsnap_amd.solvers import lasso_path as lp
from fitsnap_amd.solvers import solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ard_path_cases as cs  # noqa: E402

ROOT = cs.ROOT


class Device:
    """A context that holds the rows and the per-category statistics of ``cat`` (one pass), and their download."""

    def __init__(self, A, b, w, cat, ncat):
        self.K = A.shape[1]
        self.ctx = _capi.HipContext(0)
        self.ctx.upload_rows(A, b)
        self.ctx.set_weights(w, None)
        self.layout = self.ctx.cat_prepare(np.asarray(cat, dtype=np.int32), ncat)
        self.dptr = self.ctx.cat_normal_eq(self.layout)
        self.blocks = ap.download_blocks(self.ctx, self.dptr, ncat, self.K)

    def path(self, F, hyper, max_iter=cs.MAX_ITER, tol=cs.TOL, nsub=1):
        return self.ctx.ard_path(self.dptr, self.K, F, nsub, hyper, max_iter, tol)

    def close(self):
        self.ctx.close()


def path_of_blocks(blocks, K, F, hyper, max_iter=cs.MAX_ITER, tol=cs.TOL, nsub=1):
    """The kernel on hand-made blocks."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(blocks, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    ctx = _capi.HipContext(0)
    try:
        return ctx.ard_path(t.data_ptr(), K, F, nsub, hyper, max_iter, tol)
    finally:
        ctx.close()
        del t


def accept(blocks, K, hyper, out, max_iter=cs.MAX_ITER, tol=cs.TOL, nsub=1, rows=None, run=None, where=""):
    """Admits every problem (oracle C's margins), then: the kernel's support, iterations, kept count and status equal oracle
    C's and oracle A's, and its values are within the measured bars of oracle A; with rows (A, b, w, fold) the held-out sums
    are within HELDOUT_REL of the row-wise long-double sums.  Returns the worst figures and oracle A."""
    coef, lam, info, held = out
    C = cs.oracle_c(blocks, K, hyper, run, max_iter, tol, nsub)
    for (f, q), (cc, cl, ci) in C.items():
        assert np.array_equal(info[f, q, [0, 1, 5]], ci[[0, 1, 5]]), (where, K, f, q, "oracle C", info[f, q], ci)
        if ci[5] != 1:
            assert np.array_equal(coef[f, q] != 0, cc != 0), (where, K, f, q, "support of oracle C")
    host = ap.ard_path_host(blocks, K, hyper, max_iter, tol, nsub, run=run)
    worst = cs.compare(K, blocks, hyper, out, host, run=run, nsub=nsub, where=where)
    if rows is not None:
        A, b, w, fold = rows
        for f in range(held.shape[0]):
            r = np.flatnonzero(fold == f)
            for q in range(held.shape[1]):
                if len(r) and (run is None or run[f, q]) and info[f, q, 5] != 1:
                    ref = cs.heldout_ld(A, b, w, r, coef[f, q])
                    assert abs(held[f, q, 1] - ref) <= cs.HELDOUT_REL * ref, (where, K, f, q, "held-out", held[f, q, 1], ref)
    return worst, host


@pytest.mark.gpu
@pytest.mark.parametrize("K", cs.SWEEP_K)
def test_geometry_sweep(K):
    """K on the wave-ownership edges and the LDS-size edge, F = 3, Q = 4 (logcut 0.3, 1, 2, 3), about 3 K + 40 rows per fold."""
    A, b, w, fold, numpy_blocks, grid, _, _ = cs.sweep_problem(K)
    dev = Device(A, b, w, fold, cs.SWEEP_F)
    try:
        hyper, run = cs.hypers(dev.blocks, K, grid)
        out = dev.path(cs.SWEEP_F, hyper)
    finally:
        dev.close()
    np.testing.assert_allclose(dev.blocks, numpy_blocks, rtol=1e-9, atol=1e-9)
    assert run.all()
    worst, host = accept(dev.blocks, K, hyper, out, rows=(A, b, w, fold), where="sweep")
    print(f"K = {K:3d}  kernel vs oracle A: coef {worst['coef']:.2e} (allowed {cs.COEF_REL:.1e})  lambda {worst['lam']:.2e} "
          f"({cs.LAMBDA_REL:.1e})  alpha {worst['alpha']:.2e} ({cs.ALPHA_REL:.1e})  delta {worst['delta']:.2e} ({cs.DELTA_REL:.1e})  "
          f"pivot {worst['pivot']:.2e} ({cs.PIVOT_REL:.1e})  held-out {worst['held']:.2e} ({cs.HELDOUT_REL:.1e})  iterations "
          f"{int(host[2][:, :, 0].min())} ... {int(host[2][:, :, 0].max())}  kept {int(host[2][:, :, 1].min())} ... "
          f"{int(host[2][:, :, 1].max())}", flush=True)


@pytest.mark.gpu
def test_threshold_edges_iteration_caps_and_a_directmethod_grid():
    """On sweep_case(31): a threshold below every lambda (keep empties in the first iteration: coefficients 0, status 0), one
    above every lambda (everything kept), max_iter = 1 and 2 (status 2), Q = 1 (the bits of its column in the wider grid) and a
    ``directmethod`` grid."""
    K, F = 31, cs.SWEEP_F
    A, b, w, fold, _, grid, _, _ = cs.sweep_problem(K)
    dev = Device(A, b, w, fold, F)
    try:
        hyper, run = cs.hypers(dev.blocks, K, grid)
        edge = hyper.copy()
        edge[:, 0, 4] = 1e-12                     # lambda starts at 1 and no update reaches 1e-12
        edge[:, 3, 4] = 1e300
        out = dev.path(F, edge)
        capped = [dev.path(F, hyper, max_iter=cap) for cap in (1, 2)]
        single = dev.path(F, edge[:, 2:3])
        direct = [{"threshold_lambda": t, "alphabig": 1e-12, "lambdasmall": 1e-6} for t in (30.0, 1e4)]
        hd, rd = cs.hypers(dev.blocks, K, direct, direct=True)
        dout = dev.path(F, hd)
    finally:
        dev.close()
    rows = (A, b, w, fold)
    accept(dev.blocks, K, edge, out, rows=rows, where="edges")
    coef, lam, info, held = out
    assert np.all(coef[:, 0] == 0.0) and np.all(info[:, 0, [0, 1, 5]] == [1, 0, 0]) and np.array_equal(held[:, 0, 1], held[:, 0, 2])
    assert np.all(info[:, 3, 1] == K) and np.all(info[:, 3, 5] == 0) and np.all(coef[:, 3] != 0.0)
    for cap, res in zip((1, 2), capped):
        accept(dev.blocks, K, hyper, res, max_iter=cap, rows=rows, where=f"max_iter = {cap}")
        assert np.all(res[2][:, :, 0] == cap) and np.all(res[2][:, :, 5] == 2)
    assert all(np.array_equal(x[:, 0], y[:, 2]) for x, y in zip(single, out))
    assert rd.all()
    accept(dev.blocks, K, hd, dout, rows=rows, where="directmethod")
    assert np.all(dout[2][F, 0, 1] < dout[2][F, 1, 1])


@pytest.mark.gpu
def test_one_kept_column_a_dead_column_and_an_empty_fold():
    """K = 8, four folds of which fold 2 is empty: column 2 no row touches, column 5 fold 1 alone does; the truth sits on
    column 0 alone, so the lowest threshold keeps that column only.  nsub = 3 sub-blocks give the bits of the folds summed
    beforehand; F = 2 with one empty fold; F = 1, whose refit has no rows."""
    K, F = 8, 4
    A, b, w, fold, cls = cs.fold_rows(8, K, [40, 45, 0, 50], nonzero_frac=0.0)
    A[:, 2] = 0.0
    A[fold != 1, 5] = 0.0
    dev = Device(A, b, w, fold * 3 + cls, 3 * F)
    try:
        grid = cs.settings([0.3, 2.0, 4.0])
        hyper, run = cs.hypers(dev.blocks, K, grid, nsub=3)
        sub3 = dev.path(F, hyper, nsub=3)
    finally:
        dev.close()
    assert run.all()
    accept(dev.blocks, K, hyper, sub3, nsub=3, rows=(A, b, w, fold), where="dead")
    coef, lam, info, held = sub3
    assert np.all(info[:, 0, 1] == 1) and np.all(coef[:, 0, 0] != 0.0) and np.all(coef[:, 0, 1:] == 0.0)
    assert np.all(coef[:, :, 2] == 0.0) and np.all(lam[:, :, 2] == 1.0) and np.all(coef[1, :, 5] == 0.0) and np.all(lam[1, :, 5] == 1.0)
    assert np.all(info[:, 2, 1] == [7, 6, 7, 7, 7])
    pre, _ = lp.sum_blocks(dev.blocks, 3)
    one = path_of_blocks(pre, K, F, hyper)
    assert all(np.array_equal(x, y) for x, y in zip(sub3, one))
    # the fold without rows: its refit is the full fit, bit for bit, and it holds nothing out
    assert all(np.array_equal(x[2], x[4]) for x in one[:3]) and np.all(one[3][2] == 0.0)
    # F = 2 with one empty fold: the refit without the other fold has no rows and is not posed
    h2, r2 = cs.hypers(pre[[0, 2]], K, grid)
    two = path_of_blocks(pre[[0, 2]], K, 2, h2)
    accept(pre[[0, 2]], K, h2, two, run=r2, where="F = 2")
    assert np.array_equal(two[0][1], two[0][2]) and not r2[0].any() and r2[1:].all()
    # F = 1: the training system of the only refit is empty; the entry point runs the placeholder, the module voids it
    h1, r1 = cs.hypers(pre[:1], K, grid)
    assert not r1[0].any() and r1[1].all()
    c1, l1, i1, e1 = path_of_blocks(pre[:1], K, 1, h1)
    assert np.all(c1[0] == 0.0) and np.all(i1[0, :, [0, 1, 5]] == 0) and np.array_equal(e1[0, :, 1], e1[0, :, 2])
    accept(pre[:1], K, h1, (c1, l1, i1, e1), run=r1, where="F = 1")


@pytest.mark.gpu
def test_a_system_that_is_not_positive_definite_ends_with_status_one():
    """Hand-made blocks whose total has a negative eigenvalue: its factorisation meets a negative pivot, the problem reports
    status 1 with NaN coefficients and lambdas, the call itself succeeds, and the other problems are untouched by it."""
    K = 3
    G = np.array([[1.0, 3.0, 0.0], [3.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    good = np.eye(3)
    blocks = np.zeros((2, K * K + K + 3))
    blocks[0, :9], blocks[0, 9:12], blocks[0, 12:] = (G - good).ravel(), [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    blocks[1, :9], blocks[1, 9:12], blocks[1, 12:] = good.ravel(), [1.0, 1.0, 1.0], [4.0, 1.0, 10.0]
    hyper = np.tile(np.array([0.0, 0.0, 1e-6, 1e-6, 1e4, 1.0]), (3, 1, 1))
    coef, lam, info, held = path_of_blocks(blocks, K, 2, hyper)
    host = ap.ard_path_host(blocks, K, hyper, cs.MAX_ITER, cs.TOL)
    # problem 0 (without the first block) sees the identity; problem 1 (without the identity) has no positive diagonal left,
    # so every column is dead and nothing runs; problem 2 (all rows) meets the negative pivot in its first factorisation
    assert info[:, 0, 5].tolist() == host[2][:, 0, 5].tolist() == [0.0, 0.0, 1.0]
    assert info[:, 0, 0].tolist() == host[2][:, 0, 0].tolist() and info[1, 0, 0] == 0 and info[2, 0, 0] == 1
    assert np.all(np.isnan(coef[2])) and np.all(np.isnan(lam[2])) and np.all(np.isfinite(coef[0])) and np.all(coef[1] == 0.0)
    assert info[2, 0, 4] <= 0.0 and info[2, 0, 1] == 0 and held[1, 0, 1] == held[1, 0, 2] == 4.0
    assert cs.scaled_diff(good, coef[0, 0], host[0][0, 0]) <= cs.COEF_REL


@pytest.mark.gpu
def test_more_problems_than_compute_units():
    """F = 40, Q = 15, K = 31: 615 problems, every one equal to the host route."""
    K, F = 31, 40
    A, b, w, fold, _ = cs.fold_rows(22, K, [K + 20 - (f % 5) for f in range(F)])
    dev = Device(A, b, w, fold, F)
    try:
        hyper, run = cs.hypers(dev.blocks, K, cs.settings(np.linspace(0.2, 3.0, 15)))
        out = dev.path(F, hyper)
    finally:
        dev.close()
    assert out[0].shape == (F + 1, 15, K) and run.all()
    accept(dev.blocks, K, hyper, out, rows=(A, b, w, fold), where="615 problems")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 142])
def test_determinism_permuted_grids_and_sub_grids(K):
    A, b, w, fold, _ = cs.fold_rows(24 + K, K, [2 * K + 30, 2 * K + 35, 2 * K + 31])
    dev = Device(A, b, w, fold, 3)
    try:
        hyper, _ = cs.hypers(dev.blocks, K, cs.settings([0.3, 0.8, 1.5, 2.2, 3.0]))
        first = dev.path(3, hyper)
        second = dev.path(3, hyper)
        perm = np.array([3, 0, 4, 2, 1])
        permuted = dev.path(3, np.ascontiguousarray(hyper[:, perm]))
        sub = dev.path(3, np.ascontiguousarray(hyper[:, [4, 1]]))
    finally:
        dev.close()
    assert np.all(first[2][:, :, 5] == 0) and first[2][3, 0, 1] < first[2][3, 4, 1]
    for x, y, p, s in zip(first, second, permuted, sub):
        assert np.array_equal(x, y) and np.array_equal(x[:, perm], p) and np.array_equal(x[:, [4, 1]], s)


@pytest.mark.gpu
def test_entry_point_argument_checks_and_side_effects():
    K = 5
    A, b, w, fold, _ = cs.fold_rows(25, K, [20, 22, 21])
    dev = Device(A, b, w, fold, 3)
    ctx = dev.ctx
    try:
        good = cs.hypers(dev.blocks, K, cs.settings([1.0]))[0]
        before, layout = ctx.download_rows(), ctx.cat_info()
        ctx.ard_path(dev.dptr, K, 3, 1, good, 100, 1e-3)
        after = ctx.download_rows()
        assert all(np.array_equal(x, y) for x, y in zip(before, after)) and ctx.cat_info() == layout
        lib, out = ctx._lib, np.zeros(256)

        def status(K=K, F=3, nsub=1, ptr=dev.dptr, hyper=good, Q=1, max_iter=100, tol=1e-3, outs=(out, out, out, out)):
            """The status of the raw entry point: nothing in front of it can refuse first."""
            h = None if hyper is None else np.ascontiguousarray(hyper, dtype=np.float64)
            return lib.fsnap_ard_path(ctx._h, K, F, nsub, _capi.c_void_p(ptr), _capi._ptr(h), Q, max_iter, tol,
                                      *(_capi._ptr(x) for x in outs))

        def changed(i, v):
            h = good.copy()
            h[2, 0, i] = v
            return h

        assert status() == _capi.OK
        big = (2 << 30) // (8 * (K * K + K + 3))          # F * nsub blocks past FSNAP_CAT_STATS_MAX_BYTES
        for bad in (dict(K=0), dict(K=145), dict(F=0), dict(nsub=0), dict(Q=0), dict(max_iter=0), dict(tol=-1.0), dict(tol=np.nan),
                    dict(tol=np.inf), dict(ptr=None), dict(hyper=None), dict(outs=(None, out, out, out)),
                    dict(outs=(out, None, out, out)), dict(outs=(out, out, None, out)), dict(outs=(out, out, out, None)),
                    dict(nsub=big), dict(hyper=changed(0, -1.0)), dict(hyper=changed(1, np.nan)), dict(hyper=changed(2, np.inf)),
                    dict(hyper=changed(3, -1e-9)), dict(hyper=changed(4, 0.0)), dict(hyper=changed(4, -1.0)),
                    dict(hyper=changed(5, 0.0)), dict(hyper=changed(5, np.inf))):
            assert status(**bad) == _capi.E_ARG, bad
        # the binding turns the status into ValueError
        for change in (dict(K=145), dict(max_iter=0), dict(hyper=changed(4, 0.0))):
            args = dict(d_stats_ptr=dev.dptr, K=K, F=3, nsub=1, hyper=good, max_iter=100, tol=1e-3)
            with pytest.raises(ValueError):
                ctx.ard_path(**{**args, **change})
    finally:
        dev.close()


def ard_solver(A, b, w, labels, extra=None):
    """An ARD solver fitted on shared arrays that hold (A, b, w) with the labels in pt.fitsnap_dict."""
    pt = ParallelTools()
    d = {"SOLVER": {"solver": "ARD"}}
    d.update(extra or {})
    s = solver_factory.solver("ARD", pt, Config(pt, d))
    m, K = A.shape
    for name, arr in (("a", A), ("b", b), ("w", w)):
        pt.create_shared_array(name, m, K if name == "a" else 1)
        pt.shared_arrays[name].array[:] = arr
    pt.fitsnap_dict.update(labels)
    s.perform_fit()
    return pt, s


def labels_of(fold, cls, testing=None):
    m = len(fold)
    return {"Configs": [f"c{i // 5}" for i in range(m)], "Groups": [f"g{f}" for f in fold],
            "Testing": [False] * m if testing is None else list(testing),
            "Row_Type": [("Energy", "Force", "Stress")[k] for k in cls]}


@pytest.mark.gpu
def test_side_effects_routes_and_a_directmethod_section_through_the_solver():
    """After ard_path, perform_fit returns the bits it returned before and the resident rows and weights download unchanged;
    the device and the host route agree within the measured bar; with max_iter = 1 every status is 2."""
    K = 20
    A, b, w, fold, cls = cs.fold_rows(26, K, [80, 90, 85, 70])
    testing = np.arange(len(b)) % 11 == 0
    pt, s = ard_solver(A, b, w, labels_of(fold, cls, testing))
    fit0 = s.fit.copy()
    ctx = pt.hip()
    before = ctx.download_rows()
    res = s.ard_path([0.3, 1.0, 3.0], folds=3, seed=1)
    host = s.ard_path([0.3, 1.0, 3.0], folds=3, seed=1, method="host")
    short = s.ard_path([{"logcut": 2.0, "scap": 1e-2}], by="Groups", folds=None, max_iter=1)
    after = ctx.download_rows()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(s.fit, fit0)
    s.perform_fit()
    assert np.array_equal(s.fit, fit0)
    pt.free()
    assert res.fits.shape == (3, K) and res.iterations.shape == (4, 3) and np.all(res.status == 0)
    assert res.grid == [{"logcut": x, "scap": 1e-3, "scai": 1e-3} for x in (0.3, 1.0, 3.0)]
    assert res.table.loc[(0, "*ALL"), "ncount"] == int((~testing).sum()) and list(res.table.index.names) == ["setting", "Row_Type"]
    assert set(res.fold_of_unit.values()) == {0, 1, 2} and res.best is not None and res.best_setting == res.grid[res.best]
    assert np.array_equal(res.nonzeros, np.count_nonzero(res.fits, axis=1)) and np.array_equal(res.nonzeros, host.nonzeros)
    assert np.array_equal(res.iterations, host.iterations) and (res.best, res.sparsest) == (host.best, host.sparsest)
    d = np.sqrt(np.sum((A[~testing] * w[~testing, None]) ** 2, axis=0))
    for q in range(3):
        assert np.max(np.abs(d * (res.fits[q] - host.fits[q]))) <= cs.COEF_REL * np.max(np.abs(d * host.fits[q]))
    np.testing.assert_allclose(res.cv_error, host.cv_error, rtol=2 * cs.HELDOUT_REL)     # each within HELDOUT_REL of the row sums
    assert short.iterations.shape == (5, 1) and np.all(short.iterations == 1) and np.all(short.status == 2)
    assert sorted(short.fold_of_unit.items()) == [(f"g{i}", i) for i in range(4)] and short.grid[0]["scap"] == 1e-2
    # a [ARD] section with directmethod: numbers stand for threshold_lambda
    pt, s = ard_solver(A, b, w, labels_of(fold, cls), {"ARD": {"directmethod": 1}})
    dres = s.ard_path([30.0, 1e5], folds=3)
    pt.free()
    assert dres.grid[1] == {"threshold_lambda": 1e5, "alphabig": 1e-12, "lambdasmall": 1e-6} and np.all(dres.status == 0)
    assert dres.nonzeros[0] <= dres.nonzeros[1]


@pytest.mark.gpu
def test_wider_systems_take_the_host_route_and_refusals():
    K = 160
    A, b, w, fold, cls = cs.fold_rows(27, K, [330, 340, 335])
    pt, s = ard_solver(A, b, w, labels_of(fold, cls))
    with pytest.raises(ValueError, match="K <= 144"):
        s.ard_path([1.0], method="device")
    res = s.ard_path([0.3, 3.0], by="Groups", folds=None, table="stats")
    ctx = pt.hip()
    dptr = ctx.cat_normal_eq(ctx.cat_info()["layout"])
    assert ctx.cat_info()["ncat"] == 9                    # three groups x three row classes: one layout for both tables
    dblocks = ap.download_blocks(ctx, dptr, 9, K)         # the statistics the path was computed from
    with pytest.raises(ValueError):
        ctx.ard_path(dptr, K, 3, 3, np.tile(np.array(ap.VOID_HYPER), (4, 1, 1)), 100, 1e-3)
    pt.free()
    hyper, run = cs.hypers(dblocks, K, res.grid, nsub=3)
    coef, lam, info, held = ap.ard_path_host(dblocks, K, hyper, cs.MAX_ITER, cs.TOL, nsub=3)
    assert np.array_equal(res.fits, coef[3]) and np.array_equal(res.lambdas, lam[3]) and np.array_equal(res.iterations, info[:, :, 0])
    assert list(res.table.index.get_level_values(1)) == ["*ALL", "*ALL"] and np.all(res.status == 0)
    assert res.nonzeros[0] < res.nonzeros[1]
    pt, s = ParallelTools(), None
    for name, extra, match in (("RIDGE", {}, "has no ARD path"), ("LASSO", {}, "has no ARD path"),
                               ("ARD", {"EXTRAS": {"apply_transpose": 1}}, "apply_transpose")):
        s = solver_factory.solver(name, pt, Config(pt, {"SOLVER": {"solver": name}, **extra}))
        with pytest.raises(ValueError, match=match):
            s.ard_path([1.0])
    pt.free()


@pytest.mark.gpu
def test_leave_one_group_out_on_ta_rows_matches_sklearn_refits():
    """Through the solver on the golden Ta rows, by="Groups", folds=None, logcut 0 ... 2: the fits on all rows against
    scikit-learn (oracle D), the cross-validation curve against the held-out errors of scikit-learn refits without each group,
    table="rows" against table="stats", and ``best`` / ``sparsest`` consistent with the table."""
    A, b, w, fold, names, blocks, grid, hyper, run, _ = cs.ta_problem()
    m, K = A.shape
    F = len(names)
    rtype = np.array(["Energy" if i % 5 == 0 else "Force" for i in range(m)])
    fs = {"Groups": [names[f] for f in fold], "Testing": [False] * m, "Row_Type": rtype.tolist(), "Configs": [f"c{i // 7}" for i in range(m)]}
    cs.oracle_c(blocks, K, hyper, run)                    # admits every (group, setting)
    pt, s = ard_solver(A, b, w, fs)
    res = s.ard_path(cs.TA_LOGCUTS, by="Groups", folds=None, table="rows")
    stats = s.ard_path(cs.TA_LOGCUTS, by="Groups", folds=None, table="stats")
    host = s.ard_path(cs.TA_LOGCUTS, by="Groups", folds=None, method="host")
    pt.free()
    Q = len(grid)
    assert res.fold_of_unit == {g: i for i, g in enumerate(names)} and res.grid == grid and np.all(res.status == 0)
    folds, total = lp.sum_blocks(blocks)
    Qm = lp.downdated(folds, total, F, K)[0]
    sse = np.zeros((F, Q))
    for f in range(F + 1):
        for q in range(Q):
            ref, _, nit = cs.sklearn_refit(A, b, w, fold != f, hyper[f, q])
            assert nit == res.iterations[f, q], (f, q, nit, res.iterations[f, q])
            if f == F:
                assert np.array_equal(ref != 0, res.fits[q] != 0) and np.count_nonzero(ref) == res.nonzeros[q]
                diff = cs.scaled_diff(Qm, res.fits[q], ref)
                assert diff <= cs.D_TA_REL, (q, diff)
                continue
            out = fold == f
            sse[f, q] = np.sum((w[out] * (b[out] - A[out] @ ref)) ** 2)
    nf = np.bincount(fold).astype(float)
    held = np.stack([np.repeat(nf[:, None], Q, axis=1), sse, sse], axis=2)
    err, se, best, sparsest = ap.cv_picks(held, np.zeros((F + 1, Q)), res.nonzeros)
    # the refits agree to 1e-5 (scaled) in the coefficients; the errors of held-out rows are smooth in them
    np.testing.assert_allclose(res.cv_error, err, rtol=1e-4)
    assert (res.best, res.sparsest) == (best, sparsest) == ap.pick(res.cv_error, res.cv_se, res.nonzeros)
    assert res.best_setting == grid[best] and res.sparsest_setting == grid[sparsest]
    allrows = [k for k in res.table.index if k[1] == "*ALL"]
    rows2, stats2 = res.table.loc[allrows, "w_rmse"].to_numpy() ** 2, stats.table.loc[allrows, "w_rmse"].to_numpy() ** 2
    print("table='rows' against table='stats', weighted squared error, relative:", np.abs(stats2 / rows2 - 1), flush=True)
    np.testing.assert_allclose(stats2, rows2, rtol=cs.HELDOUT_TA_REL)
    np.testing.assert_allclose(res.cv_error, rows2, rtol=cs.HELDOUT_TA_REL)
    assert sorted(set(k[1] for k in res.table.index)) == ["*ALL", "Energy", "Force"]
    # both tables come from one layout: the same statistics, the same bits; the host route: the same decisions
    assert np.array_equal(stats.fits, res.fits) and np.array_equal(stats.cv_error, res.cv_error)
    assert np.array_equal(host.iterations, res.iterations) and np.array_equal(host.nonzeros, res.nonzeros)
    assert (host.best, host.sparsest) == (res.best, res.sparsest)
    for q in range(Q):
        assert cs.scaled_diff(Qm, res.fits[q], host.fits[q]) <= cs.TA_C_REL


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_and_a_forced_communicator_of_one(tmp_path):
    """Two ranks (peer-to-peer transport, rows dealt round-robin so that every unit spans both): the same bits on both ranks,
    the decisions and -- within the measured bar -- the values of the single-rank run.  One rank with FSNAP_FORCE_MULTI=1: the
    single-rank coefficients bit for bit and the table to 1e-12."""
    import ard_path_dist_worker as wk

    def launch(world, extra, sub):
        out = tmp_path / sub
        out.mkdir()
        procs = []
        for rank in range(world):
            env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
            env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                       FSNAP_COMM_FILE=str(out / "comm_id"), FSNAP_COMM_TOKEN="ard path ranks",
                       HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p", **extra)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ard_path_dist_worker.py"), str(out)],
                                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=out))
        logs = []
        for p in procs:
            try:
                logs.append(p.communicate(timeout=600)[0])
            except subprocess.TimeoutExpired:
                p.kill()
                logs.append(p.communicate()[0] + "\n[killed after 600 s]")
        assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
        return [dict(np.load(out / f"ard_rank{r}.npz")) for r in range(world)]

    two = launch(2, {}, "two")
    forced = launch(1, {"FSNAP_FORCE_MULTI": "1"}, "forced")[0]
    A, b, w, labels = wk.rows()
    pt, s = ard_solver(A, b, w, labels)
    one = wk.path_of(s)
    pt.free()
    folds = np.array([f"{k}={v}" for k, v in sorted(one.fold_of_unit.items())])
    index = [str(x) for x in one.table.index]
    assert np.array_equal(forced["fits"], one.fits) and np.array_equal(forced["lambdas"], one.lambdas)
    assert np.array_equal(forced["iterations"], one.iterations) and np.array_equal(forced["cv_error"], one.cv_error)
    np.testing.assert_allclose(forced["table"], one.table.to_numpy(dtype=float), rtol=1e-12)
    assert forced["index"].tolist() == index and forced["best"] == one.best and forced["sparsest"] == one.sparsest
    for key in two[0]:
        assert np.array_equal(two[0][key], two[1][key], equal_nan=two[0][key].dtype.kind == "f"), key
    # the two-rank statistics differ from the single-rank ones by the rounding of another summation order: the decisions are
    # the same (the cases keep their margins) and the values are within the bar of two routes on one system
    assert two[0]["folds"].tolist() == folds.tolist() and two[0]["index"].tolist() == index
    assert np.array_equal(two[0]["iterations"], one.iterations) and np.array_equal(two[0]["status"], one.status)
    assert np.array_equal(two[0]["fits"] != 0, one.fits != 0)
    train = ~np.asarray(labels["Testing"])
    d = np.sqrt(np.sum((A[train] * w[train, None]) ** 2, axis=0))
    for q in range(one.fits.shape[0]):
        assert np.max(np.abs(d * (two[0]["fits"][q] - one.fits[q]))) <= cs.COEF_REL * np.max(np.abs(d * one.fits[q]))
    np.testing.assert_allclose(two[0]["table"], one.table.to_numpy(dtype=float), rtol=2 * cs.HELDOUT_REL)
    np.testing.assert_allclose(two[0]["cv_error"], one.cv_error, rtol=2 * cs.HELDOUT_REL)
    assert two[0]["best"] == one.best and two[0]["sparsest"] == one.sparsest


@pytest.mark.gpu
def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ard_threshold_path.py")], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]

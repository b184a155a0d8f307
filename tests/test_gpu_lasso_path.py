"""GPU: grouped K-fold LASSO alpha paths (fsnap_lasso_path, csrc/fsnap_lasso.hip; Solver.lasso_path) under the acceptance of
tests/lasso_path_cases.py: oracle A (``lasso_path_host`` on the downloaded blocks), oracle B (scikit-learn refits without the
fold), the long-double duality gap and the row-wise long-double held-out sums; geometry, grid and fold edges, values that steer
the iteration, determinism, side effects, refusals, the solver surface on the Ta rows, two ranks, the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import lasso_path as lp
from fitsnap_amd.solvers import ridge_path as rp
from fitsnap_amd.solvers import solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lasso_path_cases as cs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = cs.EPS


class Device:
    """A context that holds the rows and the per-category statistics of ``cat`` (one pass), and their download."""

    def __init__(self, A, b, w, cat, ncat):
        self.K = A.shape[1]
        self.ctx = _capi.HipContext(0)
        self.ctx.upload_rows(A, b)
        self.ctx.set_weights(w, None)
        self.layout = self.ctx.cat_prepare(np.asarray(cat, dtype=np.int32), ncat)
        self.dptr = self.ctx.cat_normal_eq(self.layout)
        self.blocks = download_blocks(self.ctx, self.dptr, ncat, self.K)

    def path(self, F, alphas, max_iter=cs.MAX_ITER, tol=1e-4, nsub=1):
        return self.ctx.lasso_path(self.dptr, self.K, F, nsub, alphas, max_iter, tol)

    def close(self):
        self.ctx.close()


def download_blocks(ctx, dptr, ncat, K):
    """The ncat packed blocks at the device address ``dptr`` as rows of an array."""
    T = K * K + K + 3
    blocks = np.empty((ncat, T))
    for i in range(ncat):
        G, c, s = ctx.download_packed(dptr + i * T * 8, K)
        blocks[i] = np.concatenate([G.ravel(), c, s])
    return blocks


def on_device(blocks):
    """(tensor that owns the memory, device address) of hand-made blocks."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(blocks, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr()


def path_of_blocks(blocks, K, F, alphas, max_iter=cs.MAX_ITER, tol=1e-4, nsub=1):
    t, ptr = on_device(blocks)
    ctx = _capi.HipContext(0)
    try:
        return ctx.lasso_path(ptr, K, F, nsub, alphas, max_iter, tol)
    finally:
        ctx.close()
        del t


def accept(blocks, K, alphas, out, max_iter, tol, nsub=1, rows=None, tight=False, gap_clause=True):
    """Acceptance 1 (the first clause only with ``gap_clause``: at tol = 1e-12 the threshold tol y2 is within the 64 K eps y2
    rounding of a float64 gap that the second clause itself grants), acceptance 2 against oracle A and -- with rows (A, b, w,
    fold) -- oracle B, acceptance 3 with ``tight``, and the held-out sums.  Returns the worst relative figures."""
    coef, info, held = out
    folds, total = lp.sum_blocks(blocks, nsub)
    F, Q = folds.shape[0], len(alphas)
    hc, hi, hh = lp.lasso_path_host(blocks, K, alphas, max_iter, tol, nsub)
    worst = {"A": 0.0, "B": 0.0, "held": 0.0}
    for f in range(F + 1):
        Qm, qv, y2, n, dead = lp.downdated(folds, total, f, K)
        for q, alpha in enumerate(alphas):
            where = (K, f, q)
            beta, l1 = coef[f, q], alpha * n
            assert info[f, q, 2] == l1 and info[f, q, 3] == n and 1 <= info[f, q, 0] <= max_iter, where
            assert np.all(beta[dead] == 0.0), where
            true = float(cs.gap_ld(Qm, qv, y2, l1, beta))
            if dead.all():                    # nothing to fit: one sweep, zeros (y2 may be 0, so no gap is below tol y2)
                assert info[f, q, 0] == 1 and not beta.any(), where
            if gap_clause and not dead.all():
                cs.check_gap(Qm, qv, y2, l1, beta, info[f, q, 0], info[f, q, 1], max_iter, tol, where)
            else:
                assert abs(info[f, q, 1] - true) <= max(1e-6 * abs(true), 64 * K * EPS * y2), (where, info[f, q, 1], true)
            dA = float(np.linalg.norm(beta - hc[f, q]))
            gA = float(cs.gap_ld(Qm, qv, y2, l1, hc[f, q]))
            assert dA <= cs.bound2(Qm, dead, true, gA, beta), (where, "oracle A", dA)
            nrm = float(np.linalg.norm(hc[f, q]))
            if nrm > 0:
                worst["A"] = max(worst["A"], dA / nrm)
            else:
                assert not beta.any(), where
            if rows is not None and n > K:
                A, b, w, fold = rows
                ref = cs.sklearn_refit(A, b, w, fold != f, alpha)
                dB = float(np.linalg.norm(beta - ref))
                assert dB <= cs.bound2(Qm, dead, true, float(cs.gap_ld(Qm, qv, y2, l1, ref)), beta), (where, "oracle B", dB)
                if np.linalg.norm(ref) > 0:
                    worst["B"] = max(worst["B"], dB / float(np.linalg.norm(ref)))
            if f < F:
                _, _, bb, nf = lp.unpack(folds[f], K)
                assert held[f, q, 0] == nf and held[f, q, 2] == bb, where
                if rows is not None and nf > 0:
                    A, b, w, fold = rows
                    ref = cs.heldout_ld(A, b, w, np.flatnonzero(fold == f), beta)
                    err = abs(held[f, q, 1] - ref) / ref
                    worst["held"] = max(worst["held"], err)
                    assert err <= cs.HELDOUT_REL, (where, "held-out", held[f, q, 1], ref, err)
    if tight:
        assert worst["A"] <= cs.TIGHT_REL, (K, "tight", worst["A"])
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("K", cs.SWEEP_K)
def test_geometry_sweep(K):
    """K on the lane-ownership edges of a 64-lane wave and the LDS-size edge, F = 3, Q = 4, about 3 K + 40 rows per fold.  At
    the default tol = 1e-4: acceptance 1 and 2 (oracle A).  At tol = 1e-12: the reported gap, acceptance 2 against both
    oracles, acceptance 3 against oracle A and the held-out sums against the row-wise long-double sums."""
    A, b, w, fold, _ = cs.sweep_case(K)
    dev = Device(A, b, w, fold, cs.SWEEP_F)
    try:
        alphas = cs.alpha_grid(dev.blocks, K, cs.GRID4)
        loose = dev.path(cs.SWEEP_F, alphas)
        tight = dev.path(cs.SWEEP_F, alphas, tol=cs.TIGHT_TOL)
    finally:
        dev.close()
    np.testing.assert_allclose(dev.blocks, cs.blocks_numpy(A, b, w, fold, cs.SWEEP_F), rtol=1e-9, atol=1e-9)
    accept(dev.blocks, K, alphas, loose, cs.MAX_ITER, 1e-4, rows=(A, b, w, fold))
    worst = accept(dev.blocks, K, alphas, tight, cs.MAX_ITER, cs.TIGHT_TOL, rows=(A, b, w, fold), tight=True, gap_clause=False)
    print(f"K = {K:3d}  kernel vs oracle A {worst['A']:.2e} (allowed {cs.TIGHT_REL:.1e})  vs oracle B {worst['B']:.2e}  "
          f"held-out vs long double {worst['held']:.2e} (allowed {cs.HELDOUT_REL:.1e})  max sweeps {int(tight[1][:, :, 0].max())}",
          flush=True)


@pytest.mark.gpu
def test_grid_and_fold_edges():
    K = 12
    A, b, w, fold, cls = cs.fold_rows(21, K, [50, 0, 61, 47])
    dev = Device(A, b, w, fold * 3 + cls, 12)
    try:
        alphas = cs.alpha_grid(dev.blocks, K, cs.GRID4, nsub=3)
        sub3 = dev.path(4, alphas, nsub=3, tol=1e-10)
    finally:
        dev.close()
    pre, total = lp.sum_blocks(dev.blocks, 3)
    rows = (A, b, w, fold)
    accept(dev.blocks, K, alphas, sub3, cs.MAX_ITER, 1e-10, nsub=3, rows=rows)
    # nsub = 3 against the same folds summed beforehand: the same bits
    one = path_of_blocks(pre, K, 4, alphas, tol=1e-10)
    assert all(np.array_equal(x, y) for x, y in zip(sub3, one))
    # the fold without rows: its refit is the full fit, bit for bit, and it holds nothing out
    assert np.array_equal(one[0][1], one[0][4]) and np.array_equal(one[1][1], one[1][4]) and np.all(one[2][1] == 0.0)
    # Q = 1
    q1 = path_of_blocks(pre, K, 4, alphas[2:3], tol=1e-10)
    assert all(np.array_equal(x[:, 0], y[:, 2]) for x, y in zip(q1, one))
    # F = 2
    two = path_of_blocks(pre[[0, 2]], K, 2, alphas, tol=1e-10)
    accept(pre[[0, 2]], K, alphas, two, cs.MAX_ITER, 1e-10)
    # F = 1: the training system is empty
    coef, info, held = path_of_blocks(pre[:1], K, 1, alphas, max_iter=50)
    assert np.all(coef[0] == 0.0) and np.all(info[0, :, 3] == 0.0) and np.all(info[0, :, 0] >= 1)
    assert np.array_equal(held[0, :, 1], held[0, :, 2]) and np.all(held[0, :, 0] == 50)
    accept(pre[:1], K, alphas, (coef, info, held), 50, 1e-4)


@pytest.mark.gpu
def test_more_problems_than_compute_units():
    """F = 40, Q = 9, K = 8: 369 problems."""
    K, F = 8, 40
    A, b, w, fold, _ = cs.fold_rows(22, K, [3 * K + 40 - (f % 5) for f in range(F)])
    dev = Device(A, b, w, fold, F)
    try:
        alphas = cs.alpha_grid(dev.blocks, K, np.logspace(-0.3, -5, 9))
        out = dev.path(F, alphas, tol=cs.TIGHT_TOL)
    finally:
        dev.close()
    assert out[0].shape == (F + 1, 9, K)
    accept(dev.blocks, K, alphas, out, cs.MAX_ITER, cs.TIGHT_TOL, rows=(A, b, w, fold), tight=True, gap_clause=False)


@pytest.mark.gpu
def test_values_that_steer_the_iteration():
    K, F = 10, 3
    A, b, w, fold, _ = cs.fold_rows(23, K, [60, 70, 65])
    A[:, 3] = 0.0                                 # no row touches column 3
    A[fold != 1, 7] = 0.0                         # fold 1 alone touches column 7
    b = b + 0.7 * A[:, 7]
    dev = Device(A, b, w, fold, F)
    try:
        folds, total = lp.sum_blocks(dev.blocks)
        _, c, _, n = lp.unpack(total, K)
        systems = [lp.downdated(folds, total, f, K) for f in range(F + 1)]
        big = 1.01 * max(float(np.max(np.abs(qv))) / nn for _, qv, _, nn, _ in systems)
        small = 1e-3 * float(np.max(np.abs(c))) / n
        alphas = np.array([big, small, 0.0, small])
        out = dev.path(F, alphas, tol=1e-10)
        short = dev.path(F, alphas[1:2], max_iter=3, tol=1e-14)
    finally:
        dev.close()
    coef, info, held = out
    pen = [0, 1, 3]                               # the penalised alphas
    accept(dev.blocks, K, alphas[pen], tuple(x[:, pen] for x in out), cs.MAX_ITER, 1e-10)
    assert np.all(coef[:, 0] == 0.0) and np.all(info[:, 0, 0] >= 1)          # alpha above max |qv| / n
    assert np.all(coef[:, :, 3] == 0.0)                                       # the all-zero column
    assert np.all(coef[1, :, 7] == 0.0) and np.all(coef[[0, 2, 3], 1:, 7] != 0.0)   # dead in fold 1's refit only
    assert all(np.array_equal(x[:, 1], x[:, 3]) for x in out)                 # duplicate alphas
    # alpha = 0: the solution of the normal equations on the live columns, within acceptance 2.  The gap formula is
    # discontinuous there (l1_reg / dual is 0 until the dual norm is exactly 0, so the gap is half the residual until the sweeps
    # reach their fixed point), which makes the bound vacuous and acceptance 1 meaningless; so also: converged to the rounding
    # of a K x K solve
    for f, (Qm, qv, y2, nn, dead) in enumerate(systems):
        live = ~dead
        ref = np.zeros(K)
        ref[live] = np.linalg.solve(Qm[np.ix_(live, live)], qv[live])
        true = float(cs.gap_ld(Qm, qv, y2, 0.0, coef[f, 2]))
        diff = float(np.linalg.norm(coef[f, 2] - ref))
        assert diff <= cs.bound2(Qm, dead, true, float(cs.gap_ld(Qm, qv, y2, 0.0, ref)), coef[f, 2])
        assert diff <= 64 * K * EPS * np.linalg.cond(Qm[np.ix_(live, live)]) * np.linalg.norm(ref), (f, diff)
    # max_iter = 3 where three sweeps are not enough: the sweeps stop there and the reported gap is the true one
    c3, i3, _ = short
    accept(dev.blocks, K, alphas[1:2], short, 3, 1e-14, gap_clause=False)
    for f, (_, _, y2, _, _) in enumerate(systems):
        assert i3[f, 0, 0] == 3 and i3[f, 0, 1] >= 1e-14 * y2


@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 142])
def test_determinism_permuted_grids_and_sub_grids(K):
    A, b, w, fold, _ = cs.fold_rows(24 + K, K, [2 * K + 30, 2 * K + 35, 2 * K + 31])
    dev = Device(A, b, w, fold, 3)
    try:
        alphas = cs.alpha_grid(dev.blocks, K, [0.3, 0.05, 5e-3, 5e-4, 5e-5])
        first = dev.path(3, alphas, tol=1e-9)
        second = dev.path(3, alphas, tol=1e-9)
        perm = np.array([3, 0, 4, 2, 1])
        permuted = dev.path(3, alphas[perm], tol=1e-9)
        sub = dev.path(3, alphas[[4, 1]], tol=1e-9)
    finally:
        dev.close()
    for x, y, p, s in zip(first, second, permuted, sub):
        assert np.array_equal(x, y) and np.array_equal(x[:, perm], p) and np.array_equal(x[:, [4, 1]], s)


@pytest.mark.gpu
def test_entry_point_argument_checks():
    K = 5
    A, b, w, fold, _ = cs.fold_rows(25, K, [20, 22, 21])
    dev = Device(A, b, w, fold, 3)
    ctx = dev.ctx
    try:
        ok = dict(d_stats_ptr=dev.dptr, K=K, F=3, nsub=1, alphas=[1e-3], max_iter=100, tol=1e-4)
        ctx.lasso_path(**ok)
        lib, out = ctx._lib, np.zeros(256)

        def status(K=K, F=3, nsub=1, ptr=dev.dptr, alphas=(1e-3,), Q=None, max_iter=100, tol=1e-4, outs=(out, out, out)):
            """The status of the raw entry point: nothing in front of it can refuse first."""
            al = None if alphas is None else np.array(alphas if len(alphas) else [1e-3], dtype=np.float64)
            return lib.fsnap_lasso_path(ctx._h, K, F, nsub, _capi.c_void_p(ptr), _capi._ptr(al), len(alphas) if Q is None else Q,
                                        max_iter, tol, *(_capi._ptr(x) for x in outs))

        assert status() == _capi.OK
        big = (2 << 30) // (8 * (K * K + K + 3))          # F * nsub blocks past FSNAP_CAT_STATS_MAX_BYTES
        for bad in (dict(K=0), dict(K=145), dict(F=0), dict(nsub=0), dict(Q=0), dict(alphas=()), dict(max_iter=0),
                    dict(alphas=(-1.0,)), dict(alphas=(np.nan,)), dict(alphas=(1.0, np.inf)), dict(tol=-1.0), dict(tol=np.nan),
                    dict(tol=np.inf), dict(ptr=None), dict(alphas=None, Q=1), dict(outs=(None, out, out)),
                    dict(outs=(out, None, out)), dict(outs=(out, out, None)), dict(nsub=big)):
            assert status(**bad) == _capi.E_ARG, bad
        # the binding turns the status into ValueError
        for change in ({"K": 145}, {"alphas": [-1.0]}, {"max_iter": 0}):
            with pytest.raises(ValueError):
                ctx.lasso_path(**{**ok, **change})
    finally:
        dev.close()


def lasso_solver(A, b, w, labels, extra=None):
    """A LASSO solver fitted on shared arrays that hold (A, b, w) with the labels in pt.fitsnap_dict."""
    pt = ParallelTools()
    d = {"SOLVER": {"solver": "LASSO"}}
    d.update(extra or {})
    s = solver_factory.solver("LASSO", pt, Config(pt, d))
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
def test_side_effects_and_short_runs_through_the_solver():
    """After lasso_path, perform_fit returns the bits it returned before and the resident rows and weights download unchanged;
    with max_iter = 3 at a tolerance three sweeps cannot reach, ``converged`` is False everywhere and sweeps == 3."""
    K = 20
    A, b, w, fold, cls = cs.fold_rows(26, K, [80, 90, 85, 70])
    testing = np.arange(len(b)) % 11 == 0
    pt, s = lasso_solver(A, b, w, labels_of(fold, cls, testing), {"LASSO": {"alpha": 1e-3}})
    fit0 = s.fit.copy()
    ctx = pt.hip()
    before = ctx.download_rows()
    res = s.lasso_path([1e-2, 1e-3, 1e-4], folds=3, seed=1)
    short = s.lasso_path([1e-5], by="Groups", folds=None, tol=1e-15, max_iter=3)
    after = ctx.download_rows()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(s.fit, fit0)
    s.perform_fit()
    assert np.array_equal(s.fit, fit0)
    pt.free()
    assert res.fits.shape == (3, K) and res.sweeps.shape == (4, 3) and res.converged.all()
    assert res.table.loc[(1e-2, "*ALL"), "ncount"] == int((~testing).sum())
    assert set(res.fold_of_unit.values()) == {0, 1, 2} and res.best is not None
    assert short.sweeps.shape == (5, 1) and np.all(short.sweeps == 3) and not short.converged.any()
    assert sorted(short.fold_of_unit.items()) == [(f"g{i}", i) for i in range(4)]


@pytest.mark.gpu
def test_wider_systems_take_the_host_route_and_refusals():
    K = 145
    A, b, w, fold, cls = cs.fold_rows(27, K, [330, 340, 335])
    labels = labels_of(fold, cls)
    pt, s = lasso_solver(A, b, w, labels, {"LASSO": {"alpha": 1e-3}})
    with pytest.raises(ValueError, match="K <= 144"):
        s.lasso_path([1e-3], method="device")
    blocks = cs.blocks_numpy(A, b, w, fold, 3)
    alphas = cs.alpha_grid(blocks, K, [0.05, 1e-3])
    res = s.lasso_path(alphas, by="Groups", folds=None, tol=1e-10, table="stats")
    ctx = pt.hip()
    info = ctx.cat_info()
    dptr = ctx.cat_normal_eq(info["layout"])
    assert info["ncat"] == 9                              # three groups x three row classes: one layout for both tables
    dblocks = download_blocks(ctx, dptr, 9, K)            # the statistics the path was computed from
    with pytest.raises(ValueError):
        ctx.lasso_path(dptr, K, 3, 3, alphas, 100, 1e-4)
    pt.free()
    np.testing.assert_allclose(lp.sum_blocks(dblocks, 3)[0], blocks, rtol=1e-9, atol=1e-9)
    folds, total = lp.sum_blocks(dblocks, 3)
    Qm, qv, y2, n, dead = lp.downdated(folds, total, 3, K)
    for q, alpha in enumerate(alphas):
        ref = cs.sklearn_refit(A, b, w, np.ones(len(b), dtype=bool), alpha)
        gaps = [float(cs.gap_ld(Qm, qv, y2, alpha * n, x)) for x in (res.fits[q], ref)]
        assert abs(res.gaps[3, q] - gaps[0]) <= max(1e-6 * abs(gaps[0]), 64 * K * EPS * y2)
        assert np.linalg.norm(res.fits[q] - ref) <= cs.bound2(Qm, dead, gaps[0], gaps[1], res.fits[q]), (q, gaps)
    assert list(res.table.index.get_level_values(1)) == ["*ALL", "*ALL"] and res.converged.all()
    pt, s = ParallelTools(), None
    for name, extra, match in (("RIDGE", {}, "has no LASSO path"), ("SVD", {}, "has no LASSO path"),
                               ("LASSO", {"EXTRAS": {"apply_transpose": 1}}, "apply_transpose")):
        s = solver_factory.solver(name, pt, Config(pt, {"SOLVER": {"solver": name}, **extra}))
        with pytest.raises(ValueError, match=match):
            s.lasso_path([1e-3])
    pt.free()


@pytest.mark.gpu
def test_leave_one_group_out_on_ta_rows_matches_sklearn_refits(ta, ta_fits):
    """Through the solver on the golden Ta rows, by="Groups", folds=None, five alphas: the coefficients against scikit-learn
    refits without each group (acceptance 2), the per-class table against numpy on those refits, table="rows" against
    table="stats" on the weighted error, and ``best`` / ``sparsest`` against the oracle's picks."""
    A, b, w = ta
    groups = ta_fits["ea_groups"]
    m, K = A.shape
    rtype = np.array(["Energy" if i % 5 == 0 else "Force" for i in range(m)])
    fs = {"Groups": groups.tolist(), "Testing": [False] * m, "Row_Type": rtype.tolist(), "Configs": [f"c{i // 7}" for i in range(m)]}
    pt, s = lasso_solver(A, b, w, fs, {"LASSO": {"alpha": 1e-4, "max_iter": 100000}})
    names = sorted(set(groups.tolist()))
    fold = np.array([names.index(g) for g in groups])
    F = len(names)
    blocks = cs.blocks_numpy(A, b, w, fold, F)
    alphas = cs.alpha_grid(blocks, K, [0.5, 0.3, 0.1, 0.03, 0.01])
    tol = 1e-9
    res = s.lasso_path(alphas, by="Groups", folds=None, tol=tol, table="rows")
    ctx = pt.hip()
    dblocks = download_blocks(ctx, ctx.cat_normal_eq(ctx.cat_info()["layout"]), 2 * F, K)   # what the path was computed from
    stats = s.lasso_path(alphas, by="Groups", folds=None, tol=tol, table="stats")
    host = s.lasso_path(alphas, by="Groups", folds=None, tol=tol, method="host")
    pt.free()
    assert res.fold_of_unit == {g: i for i, g in enumerate(names)}
    folds, total = lp.sum_blocks(blocks)
    sse = np.zeros((F, len(alphas)))
    pooled = np.zeros((len(alphas), 2, 4))
    for f in range(F + 1):
        Qm, qv, y2, n, dead = lp.downdated(folds, total, f, K)
        for q, alpha in enumerate(alphas):
            ref = cs.sklearn_refit(A, b, w, fold != f, alpha)
            if f == F:
                # acceptance 2 on the statistics the path was computed from
                Qd, qd, y2d, nd, dd = lp.downdated(*lp.sum_blocks(dblocks, 2), F, K)
                gaps = [float(cs.gap_ld(Qd, qd, y2d, alpha * nd, x)) for x in (res.fits[q], ref)]
                assert abs(res.gaps[F, q] - gaps[0]) <= max(1e-6 * abs(gaps[0]), 64 * K * EPS * y2d)
                diff = float(np.linalg.norm(res.fits[q] - ref))
                assert diff <= cs.bound2(Qd, dd, gaps[0], gaps[1], res.fits[q]), (q, diff, gaps)
                continue
            out = fold == f
            r = b[out] - A[out] @ ref
            sse[f, q] = np.sum((w[out] * r) ** 2)
            for k, name in enumerate(("Energy", "Force")):
                sel = rtype[out] == name
                pooled[q, k] += (sel.sum(), np.abs(r[sel]).sum(), (r[sel] ** 2).sum(), ((w[out][sel] * r[sel]) ** 2).sum())
    oracle = rp.path_table(alphas, pooled, ["Energy", "Force"])
    assert list(res.table.index) == list(oracle.index)
    assert np.array_equal(res.table["ncount"].to_numpy(), oracle["ncount"].to_numpy())
    # the refits agree to sqrt(tol)-level in the coefficients; the errors of held-out rows are smooth in them
    np.testing.assert_allclose(res.table[["mae", "rmse", "w_rmse"]].to_numpy(), oracle[["mae", "rmse", "w_rmse"]].to_numpy(), rtol=1e-4)
    allrows = [k for k in res.table.index if k[1] == "*ALL"]
    rows2, stats2 = res.table.loc[allrows, "w_rmse"].to_numpy() ** 2, stats.table.loc[allrows, "w_rmse"].to_numpy() ** 2
    print("table='rows' against table='stats', weighted squared error, relative:", np.abs(stats2 / rows2 - 1), flush=True)
    np.testing.assert_allclose(stats2, rows2, rtol=cs.HELDOUT_REL)
    np.testing.assert_allclose(res.cv_error, rows2, rtol=cs.HELDOUT_REL)
    # both tables come from one layout: the same statistics, the same bits
    assert np.array_equal(stats.fits, res.fits) and np.array_equal(stats.cv_error, res.cv_error)
    assert np.array_equal(host.fits, res.fits) or np.max(np.abs(host.fits - res.fits)) <= 1e-6 * np.max(np.abs(res.fits))
    assert np.array_equal(host.nonzeros, res.nonzeros) and stats.best == res.best and stats.sparsest == res.sparsest
    nf = np.bincount(fold).astype(float)
    held = np.stack([np.repeat(nf[:, None], len(alphas), axis=1), sse, sse], axis=2)
    err, se, best, sparsest = lp.cv_curve(alphas, held)
    np.testing.assert_allclose(res.cv_error, err, rtol=1e-4)
    assert res.best == best and res.sparsest == sparsest and res.best_alpha == alphas[best]


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_and_a_forced_communicator_of_one(tmp_path):
    """Two ranks (peer-to-peer transport, rows dealt round-robin so that every unit spans both): the same bits on both ranks,
    within acceptance 2 of the single-rank run.  One rank with FSNAP_FORCE_MULTI=1: the single-rank coefficients bit for bit
    and the table to 1e-12."""
    import lasso_path_dist_worker as wk

    def launch(world, extra, sub):
        out = tmp_path / sub
        out.mkdir()
        procs = []
        for rank in range(world):
            env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
            env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                       FSNAP_COMM_FILE=str(out / "comm_id"), FSNAP_COMM_TOKEN="lasso path ranks",
                       HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p", **extra)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "lasso_path_dist_worker.py"), str(out)],
                                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=out))
        logs = []
        for p in procs:
            try:
                logs.append(p.communicate(timeout=600)[0])
            except subprocess.TimeoutExpired:
                p.kill()
                logs.append(p.communicate()[0] + "\n[killed after 600 s]")
        assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
        return [dict(np.load(out / f"lasso_rank{r}.npz")) for r in range(world)]

    two = launch(2, {}, "two")
    forced = launch(1, {"FSNAP_FORCE_MULTI": "1"}, "forced")[0]
    A, b, w, labels = wk.rows()
    pt, s = lasso_solver(A, b, w, labels, {"LASSO": {"alpha": 1e-3}})
    G, c, sc = s.last_statistics
    alphas = np.asarray(wk.ALPHA_FRACTIONS) * float(np.max(np.abs(c))) / float(sc[2])
    one = wk.path_of(s, alphas)
    pt.free()
    folds = np.array([f"{k}={v}" for k, v in sorted(one.fold_of_unit.items())])
    index = [str(x) for x in one.table.index]
    assert np.array_equal(forced["alphas"], alphas) and np.array_equal(forced["fits"], one.fits)
    assert np.array_equal(forced["sweeps"], one.sweeps) and np.array_equal(forced["cv_error"], one.cv_error)
    np.testing.assert_allclose(forced["table"], one.table.to_numpy(dtype=float), rtol=1e-12)
    assert forced["index"].tolist() == index and forced["best"] == one.best and forced["sparsest"] == one.sparsest
    for key in two[0]:
        assert np.array_equal(two[0][key], two[1][key], equal_nan=two[0][key].dtype.kind == "f"), key
    # the alphas come from each run's own statistics and may differ in the last bit: compare the Row_Type level of the index
    assert two[0]["folds"].tolist() == folds.tolist()
    assert [x.split(", ")[1] for x in two[0]["index"].tolist()] == [x.split(", ")[1] for x in index]
    np.testing.assert_allclose(two[0]["alphas"], alphas, rtol=1e-12)
    train = ~np.asarray(labels["Testing"])
    Aw, bw = A[train] * w[train, None], b[train] * w[train]
    Qm, qv, y2, n = Aw.T @ Aw, Aw.T @ bw, float(bw @ bw), float(train.sum())
    lam = float(np.linalg.eigvalsh(Qm)[0])
    for q in range(len(alphas)):
        # both runs stop at gap < 1e-10 y2 on statistics that differ by rounding
        bound = 2 * np.sqrt(2 * 1e-10 * y2 / lam) + 64 * 31 * EPS * np.linalg.cond(Qm) * np.linalg.norm(one.fits[q])
        assert np.linalg.norm(two[0]["fits"][q] - one.fits[q]) <= bound
    np.testing.assert_allclose(two[0]["table"], one.table.to_numpy(dtype=float), rtol=1e-4)
    np.testing.assert_allclose(two[0]["cv_error"], one.cv_error, rtol=1e-4)


@pytest.mark.gpu
def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "lasso_alpha_path.py")], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]

"""GPU: grouped K-fold BCS sparsity paths (fsnap_bcs_path, csrc/fsnap_bcs.hip; Solver.bcs_path; the BCS solver) against the host
route (``bcs_path.bcs_path_host``: fsnap_bcs_gram per problem on the same statistics) -- identical picks, active sets, status and
iterations on cases whose margin the host route qualifies, values within ``bcs_cases.DEVICE_BAR`` --, the dead-column rule and
an empty training set, determinism, refusals, the solver surface, two ranks, the example.  Cases: tests/bcs_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import bcs_path as bp
from fitsnap_amd.solvers import solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bcs_cases as cs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("coef", "active", "alpha", "errbars", "picks", "info", "heldout", "Sig")


def on_device(blocks):
    """(tensor that owns the memory, device address) of hand-made blocks."""
    import torch

    t = torch.from_numpy(np.array(blocks, dtype=np.float64, order="C")).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr()


def path_of_blocks(blocks, K, F, nsub, hyper, max_active, deletion, ctx=None):
    t, ptr = on_device(blocks)
    own = ctx is None
    ctx = _capi.HipContext(0) if own else ctx
    try:
        return ctx.bcs_path(ptr, K, F, nsub, hyper, max_active, deletion)
    finally:
        if own:
            ctx.close()
        del t


def agree(dev, host, where):
    """The kernel's outputs against the host route's: the discrete ones equal, the values within DEVICE_BAR of the largest
    entry of each problem's output.  Returns the largest relative difference."""
    d, h = dict(zip(NAMES, dev)), dict(zip(NAMES, host))
    assert np.array_equal(d["picks"], h["picks"]), where
    assert np.array_equal(d["active"], h["active"]), where
    assert np.array_equal(d["info"][:, :, :2], h["info"][:, :, :2]), where            # iterations, status
    assert np.array_equal(d["heldout"][:, :, [0, 2]], h["heldout"][:, :, [0, 2]]), where
    worst = 0.0
    nprob, Q = d["coef"].shape[0], d["coef"].shape[1]
    for f in range(nprob):
        for q in range(Q):
            pairs = [(d[k][f, q], h[k][f, q]) for k in ("coef", "alpha", "errbars")]
            pairs += [(d["info"][f, q, j], h["info"][f, q, j]) for j in (2, 3, 4)]    # sigma2 used, re-estimated, rss
            if f < nprob - 1:
                pairs.append((d["heldout"][f, q, 1], h["heldout"][f, q, 1]))
            else:
                pairs.append((d["Sig"][q], h["Sig"][q]))
            for x, y in pairs:
                y = np.asarray(y, dtype=np.float64)
                if y.size and np.max(np.abs(y)) > 0:
                    worst = max(worst, float(np.max(np.abs(np.asarray(x) - y)) / np.max(np.abs(y))))
                else:
                    assert not np.asarray(x).any(), where
            dm, hm = d["info"][f, q, 5], h["info"][f, q, 5]
            assert (np.isinf(dm) and np.isinf(hm)) or abs(dm - hm) <= 1e-6 * abs(hm), (where, "margin", dm, hm)
    assert worst <= cs.DEVICE_BAR, (where, worst)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cs.PATH_CASES))
def test_kernel_against_the_host_route(name):
    """K in {1, 2, 63, 64, 65, 128, 129, 144}, F in {2, 5, 40}, nsub in {1, 3}, Q in {1, 3}, itermax in {1, 10, 80},
    max_active in {1, 2, 33, 63, 64} (``fill``: 64 columns enter), both deletions (``del_ref`` / ``del_exact``: ten deletions
    or more each).  Every case qualifies (margin >= 1e-3 on the host
    route: asserted first), then picks, active sets, status and iterations are equal and the values agree within DEVICE_BAR."""
    blocks, K, F, nsub, hyper, ma, deletion = cs.case_blocks(name)
    host = cs.case_host(name)
    assert host[5][:, :, 5].min() >= cs.MIN_MARGIN, (name, host[5][:, :, 5].min())
    dev = path_of_blocks(blocks, K, F, nsub, hyper, ma, deletion)
    worst = agree(dev, host, name)
    na = (dev[1] >= 0).sum(axis=2)
    print(f"{name}: K = {K} F = {F} nsub = {nsub} Q = {hyper.shape[0]} max_active = {ma} {deletion}: largest relative difference "
          f"{worst:.3e}, active sets {na.min()} ... {na.max()}, iterations up to {int(dev[5][:, :, 0].max())}", flush=True)
    for mode in ("reference", "exact"):
        # the deletion branch of the kernel runs in either mode: its cases are in the list, with the deletions they stand for
        assert any(cs.PATH_CASES[n][6] == mode for n in cs.DELETION_CASES)
    if name in cs.DELETION_CASES:
        ndel = int((dev[4][..., 1] == _capi.BCS_DEL).sum())
        print(f"{name}: {ndel} deletions on the device", flush=True)
        assert ndel >= cs.DELETION_CASES[name] and ndel == int((host[4][..., 1] == _capi.BCS_DEL).sum())
    if name == "fill":
        assert na.max() == 64 and (dev[4][..., 1] == _capi.BCS_ADD).sum(axis=2).max() == 63


@pytest.mark.gpu
def test_dead_column_and_an_empty_training_set():
    blocks, K = cs.edge_blocks(3)
    hyper = bp.hyper_of(bp.resolve_grid([0.01, {"sigma2": 0.2, "itermax": 30}], type("S", (), dict(sigma2=None, scale=0.01, eta=1e-18,
                                                                                                    itermax=12))))
    for deletion in ("reference", "exact"):
        dev = path_of_blocks(blocks, K, 3, 1, hyper, K, deletion)
        host = bp.bcs_path_host(blocks, K, hyper, K, deletion)
        assert host[5][:, :, 5].min() >= cs.MIN_MARGIN
        agree(dev, host, f"edges {deletion}")
        coef, active = dev[0], dev[1]
        assert np.all(coef[:, :, 3] == 0.0) and not (active == 3).any()        # the zero column is dead everywhere
        assert np.all(coef[1, :, 7] == 0.0) and not (active[1] == 7).any()     # fold 1 alone touches column 7
        assert all(coef[f, 0, 7] != 0.0 for f in (0, 2, 3))
    # one fold holds every row: its refit has no training rows and no live column, and predicts zero
    one = blocks.sum(axis=0, keepdims=True)
    dev = path_of_blocks(one, K, 1, 1, hyper, K, "reference")
    host = bp.bcs_path_host(one, K, hyper, K, "reference")
    assert np.array_equal(dev[4], host[4]) and np.array_equal(dev[1], host[1])
    assert not dev[0][0].any() and np.all(dev[1][0] == -1) and np.all(dev[5][0, :, :2] == 0.0) and np.all(dev[4][0] == -1)
    assert np.all(dev[6][0, :, 1] == dev[6][0, :, 2]) and np.count_nonzero(dev[0][1]) > 0
    np.testing.assert_allclose(dev[0][1], host[0][1], rtol=0, atol=cs.DEVICE_BAR * np.max(np.abs(host[0][1])))


@pytest.mark.gpu
@pytest.mark.parametrize("poison,where", [(np.nan, "G"), (np.inf, "c")])
def test_non_finite_statistics_end_every_problem_with_status_1(poison, where):
    """A NaN in G_33 or an Inf in c_3 of one fold's block reaches the total and so every problem: each one ends within its
    itermax with status 1 and NaN coefficients, and the call returns FSNAP_OK (a failed problem is its own status, as in
    fsnap_ard_path).  (An Inf in G_33 alone is not such a case: where it does not meet itself in a downdate it is a column of
    infinite norm, which never scores, and the problem ends finite.)"""
    name = "k65"
    blocks, K, F, nsub, hyper, ma, deletion = cs.case_blocks(name)
    bad = np.array(blocks)
    bad[1, 3 * K + 3 if where == "G" else K * K + 3] = poison         # of fold 1
    hyper = np.concatenate([hyper, [[0.05, 0.0, 1e-18, 80.0]]])
    coef, active, alpha, err, picks, info, held, Sig = path_of_blocks(bad, K, F, nsub, hyper, ma, deletion)
    assert np.all(info[:, :, 1] == 1.0) and np.all(info[:, :, 0] <= hyper[None, :, 3])
    assert np.isnan(coef).all() and np.isnan(held[:, :, 1]).all()
    assert np.all((active >= -1) & (active < K)) and np.all((picks[..., 0] >= -1) & (picks[..., 0] < K))
    # the same call on the clean blocks still gives the host route's picks: nothing was left behind
    clean = path_of_blocks(blocks, K, F, nsub, hyper[:1], ma, deletion)
    assert np.array_equal(clean[4], cs.case_host(name)[4])


@pytest.mark.gpu
def test_bit_identical_runs_permuted_grids_and_folds():
    """Integer rows with unit weights: every sum of blocks is exact, so the total is the same bits whatever the order of the
    folds or the presence of an empty one, and a problem's result must then be the same bits wherever it stands in the call."""
    K, F = 70, 5
    rng = np.random.default_rng(41)
    m = 1200
    A = rng.integers(-3, 4, (m, K)).astype(np.float64)
    b = (A[:, :9] @ rng.integers(-2, 3, 9) + rng.integers(-1, 2, m)).astype(np.float64)
    fold = rng.integers(0, F, m)
    fold[fold == 3] = 0                                   # fold 3 is empty
    blocks = cs.blocks_ld(A, b, np.ones(m), fold, F)
    section = type("S", (), dict(sigma2=None, scale=0.01, eta=1e-18, itermax=10))
    hyper = bp.hyper_of(bp.resolve_grid([1e-3, {"sigma2": 0.5, "itermax": 40}, {"scale": 0.1, "itermax": 3}], section))
    ctx = _capi.HipContext(0)
    try:
        for deletion in ("reference", "exact"):
            first = path_of_blocks(blocks, K, F, 1, hyper, 64, deletion, ctx)
            second = path_of_blocks(blocks, K, F, 1, hyper, 64, deletion, ctx)
            assert all(np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(first, second))
            # the grid permuted and cut: P, the stride of the pick lists, follows the largest itermax
            qperm = np.array([2, 0, 1])
            permuted = path_of_blocks(blocks, K, F, 1, hyper[qperm], 64, deletion, ctx)
            sub = path_of_blocks(blocks, K, F, 1, hyper[[0, 2]], 64, deletion, ctx)
            for i, (x, p, s) in enumerate(zip(first, permuted, sub)):
                ax = 0 if NAMES[i] == "Sig" else 1
                assert np.array_equal(np.take(x, qperm, axis=ax), p), (deletion, NAMES[i])
                xs = np.take(x, [0, 2], axis=ax)
                if NAMES[i] == "picks":
                    assert np.array_equal(xs[:, :, :s.shape[2]], s) and np.all(xs[:, :, s.shape[2]:] == -1)
                else:
                    assert np.array_equal(xs, s), (deletion, NAMES[i])
            # the folds permuted and cut
            fperm = np.array([4, 2, 0, 3, 1])
            fp = path_of_blocks(blocks[fperm], K, F, 1, hyper, 64, deletion, ctx)
            fsub = [0, 1, 2, 4]
            fs = path_of_blocks(blocks[fsub], K, 4, 1, hyper, 64, deletion, ctx)
            for i, (x, p, s) in enumerate(zip(first, fp, fs)):
                if NAMES[i] == "Sig":
                    assert np.array_equal(x, p) and np.array_equal(x, s)
                    continue
                nf = F if NAMES[i] == "heldout" else F + 1
                assert np.array_equal(x[np.r_[fperm, F][:nf]], p), (deletion, NAMES[i])
                assert np.array_equal(x[np.r_[fsub, F][:nf - 1]], s), (deletion, NAMES[i])
            # the empty fold's refit is the full fit and it holds nothing out
            assert np.array_equal(first[0][3], first[0][F]) and np.array_equal(first[4][3], first[4][F])
            assert np.all(first[6][3] == 0.0)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_entry_point_argument_checks():
    K, F = 6, 3
    A, b, w, conf, _ = cs.rows(77, K)
    blocks = cs.blocks_ld(A, b, w, conf % F, F)
    t, ptr = on_device(blocks)
    ctx = _capi.HipContext(0)
    try:
        good = np.array([[0.0, 0.01, 1e-18, 10.0], [0.3, 0.0, 0.0, 4.0]])
        ctx.bcs_path(ptr, K, F, 1, good, K)
        lib = ctx._lib
        io, do = np.zeros(4096, dtype=np.int32), np.zeros(4096)

        def status(K=K, F=F, nsub=1, ptr=ptr, hyper=good, Q=None, ma=K, deletion=0, outs=(do, io, do, do, io, do, do, do)):
            """The status of the raw entry point: nothing in front of it can refuse first."""
            hy = None if hyper is None else np.ascontiguousarray(hyper, dtype=np.float64)
            return lib.fsnap_bcs_path(ctx._h, K, F, nsub, _capi.c_void_p(ptr), _capi._ptr(hy), len(hyper) if Q is None else Q, ma,
                                      deletion, *(_capi._ptr(x) for x in outs))

        assert status() == _capi.OK and status(deletion=1) == _capi.OK and status(ma=1) == _capi.OK
        big = (2 << 30) // (8 * (K * K + K + 3))          # F * nsub blocks past FSNAP_CAT_STATS_MAX_BYTES

        def row(**kw):
            h = dict(sigma2=0.0, scale=0.01, eta=1e-18, itermax=10.0)
            h.update(kw)
            return np.array([[h["sigma2"], h["scale"], h["eta"], h["itermax"]]])

        bads = [dict(K=0), dict(K=145), dict(F=0), dict(nsub=0), dict(Q=0), dict(ptr=None), dict(hyper=None, Q=1), dict(ma=0),
                dict(ma=K + 1), dict(deletion=2), dict(deletion=-1), dict(nsub=big), dict(hyper=row(sigma2=-1.0)),
                dict(hyper=row(scale=0.0)), dict(hyper=row(scale=-1.0)), dict(hyper=row(eta=-1.0)), dict(hyper=row(itermax=0.0)),
                dict(hyper=row(itermax=2.5)), dict(hyper=row(itermax=65537.0)), dict(hyper=row(sigma2=np.nan)),
                dict(hyper=row(scale=np.inf)), dict(hyper=row(eta=np.nan)), dict(hyper=row(itermax=np.nan))]
        for i in range(8):
            outs = [do, io, do, do, io, do, do, do]
            outs[i] = None
            bads.append(dict(outs=tuple(outs)))
        for bad in bads:
            assert status(**bad) == _capi.E_ARG, bad
        # max_active stops at 64 whatever K
        wide = np.zeros((2, 140 * 140 + 140 + 3))
        t2, ptr2 = on_device(wide)
        big_i, big_d = np.zeros(3 * 140 * 64, dtype=np.int32), np.zeros(3 * 140 * 140)
        outs = (big_d, big_i, big_d, big_d, big_i, big_d, big_d, big_d)
        assert status(K=140, F=2, ptr=ptr2, ma=65, outs=outs) == _capi.E_ARG
        assert status(K=140, F=2, ptr=ptr2, ma=64, outs=outs) == _capi.OK
        del t2
        # the binding turns the status into ValueError
        for change in ({"K": 145}, {"max_active": 7}, {"hyper": row(scale=-1.0)}, {"deletion": "textbook"},
                       {"hyper": np.zeros((2, 3))}):
            kw = {**dict(d_stats_ptr=ptr, K=K, F=F, nsub=1, hyper=good, max_active=K, deletion="reference"), **change}
            with pytest.raises(ValueError):
                ctx.bcs_path(**kw)
    finally:
        ctx.close()
        del t


def bcs_solver(A, b, w, labels, section=None, extra=None):
    """A BCS solver fitted on shared arrays that hold (A, b, w) with the labels in pt.fitsnap_dict."""
    pt = ParallelTools()
    d = {"SOLVER": {"solver": "BCS"}, "BCS": dict(section or {})}
    d.update(extra or {})
    s = solver_factory.solver("BCS", pt, Config(pt, d))
    m, K = A.shape
    for name, arr in (("a", A), ("b", b), ("w", w)):
        pt.create_shared_array(name, m, K if name == "a" else 1)
        pt.shared_arrays[name].array[:] = arr
    pt.fitsnap_dict.update(labels)
    s.perform_fit()
    return pt, s


def labels_of(conf, cls, testing):
    return {"Configs": [f"c{i:03d}" for i in conf], "Groups": [f"g{i % 4}" for i in conf], "Testing": list(testing),
            "Row_Type": [("Energy", "Force", "Stress")[k] for k in cls]}


GRID = [{"scale": 0.01}, {"scale": 1e-3, "itermax": 30}, {"sigma2": 0.05, "itermax": 60, "eta": 1e-8}]


def surface(A, b, w, labels, section, grid, folds, where):
    """Solver.bcs_path on a fitted BCS solver, both routes and both tables; the checks the two end-to-end tests share."""
    pt, s = bcs_solver(A, b, w, labels, section)
    fit0, cov0, used0 = s.fit.copy(), s.cov.copy(), s.used.copy()
    ctx = pt.hip()
    before = ctx.download_rows()
    res = s.bcs_path(grid, folds=folds, seed=2, method="device", table="rows")
    stats = s.bcs_path(grid, folds=folds, seed=2, method="device", table="stats")
    host = s.bcs_path(grid, folds=folds, seed=2, method="host", table="rows")
    auto = s.bcs_path(grid, folds=folds, seed=2)
    after = ctx.download_rows()
    assert all(np.array_equal(x, y) for x, y in zip(before, after)) and np.array_equal(s.fit, fit0)
    K, Q, F = A.shape[1], len(grid), folds
    assert host.margin.min() >= cs.MIN_MARGIN, (where, host.margin.min())
    # The two routes read the same fold statistics: they are held to DEVICE_BAR whatever the condition number of the rows
    # (measured on the MI355X: fits and covs bit-identical on the Ta rows, condition number 7e10, and on the synthetic rows).
    # perform_fit is another matter: its statistics are the same sums in ANOTHER ORDER, and rounding the statistics moves the
    # solution of a system by up to its condition number x eps, so that comparison alone gets max(DEVICE_BAR, cond x eps)
    # (Ta: 1.9e-8 after Jacobi scaling; measured there 2.5e-11 in the fit and 3.1e-11 in the covariance; synthetic 3e-16, 2e-14).
    G = s.last_statistics[0]
    d = np.sqrt(np.diag(G))
    fit_bar = max(cs.DEVICE_BAR, float(np.linalg.cond(G / d[:, None] / d[None, :])) * np.finfo(np.float64).eps)
    scale = np.max(np.abs(host.fits), axis=1, keepdims=True)
    print(f"{where}: device - host: fits {np.max(np.abs(res.fits - host.fits) / scale):.2e} covs "
          f"{np.max(np.abs(res.covs - host.covs)) / np.max(np.abs(host.covs)):.2e} sigma2 "
          f"{np.max(np.abs(res.sigma2 - host.sigma2) / np.abs(host.sigma2)):.2e} (bar {cs.DEVICE_BAR:.2e}); device - perform_fit: fit "
          f"{np.max(np.abs(res.fits[0] - fit0)) / np.max(np.abs(fit0)):.2e} cov {np.max(np.abs(res.covs[0] - cov0)) / np.max(np.abs(cov0)):.2e} "
          f"(bar {fit_bar:.2e})", flush=True)
    assert res.fits.shape == (Q, K) and res.covs.shape == (Q, K, K) and res.status.shape == (F + 1, Q)
    assert res.picks.shape[:2] == (F + 1, Q) and res.sigma2.shape == (F + 1, Q) and len(res.fold_of_unit) == len(set(labels["Configs"]))
    # the device route against the host route
    assert np.array_equal(res.picks, host.picks) and np.array_equal(res.active, host.active)
    assert np.array_equal(res.status, host.status) and np.array_equal(res.iterations, host.iterations)
    assert np.max(np.abs(res.fits - host.fits) / scale) <= cs.DEVICE_BAR
    assert np.max(np.abs(res.covs - host.covs)) <= cs.DEVICE_BAR * np.max(np.abs(host.covs))
    assert np.max(np.abs(res.errbars - host.errbars)) <= cs.DEVICE_BAR * np.max(np.abs(host.errbars))
    assert np.max(np.abs(res.sigma2 - host.sigma2) / np.abs(host.sigma2)) <= cs.DEVICE_BAR
    np.testing.assert_allclose(res.cv_error, host.cv_error, rtol=1e-7)
    assert res.best == host.best and res.sparsest == host.sparsest and res.best_setting == grid_full(res, res.best)
    assert np.array_equal(res.frequency, host.frequency) and np.array_equal(res.nonzeros, host.nonzeros)
    assert np.array_equal(auto.fits, res.fits) and np.array_equal(stats.fits, res.fits)
    # the f = F fit of the section's own setting is BCS.perform_fit (its statistics are summed in another order)
    assert res.active[0][res.active[0] >= 0].tolist() == used0.tolist()
    assert np.max(np.abs(res.fits[0] - fit0)) <= fit_bar * np.max(np.abs(fit0))
    assert np.max(np.abs(res.covs[0] - cov0)) <= fit_bar * np.max(np.abs(cov0))
    # the tables: rows and statistics agree on the weighted error, and the curve is the table
    for q in range(Q):
        np.testing.assert_allclose(stats.table.loc[(q, "*ALL"), "w_rmse"] ** 2, stats.cv_error[q], rtol=1e-12)
        np.testing.assert_allclose(res.table.loc[(q, "*ALL"), "w_rmse"] ** 2, stats.cv_error[q], rtol=1e-7)
        assert res.table.loc[(q, "*ALL"), "ncount"] == stats.table.loc[(q, "*ALL"), "ncount"]
    assert list(res.table.index.names) == ["setting", "Row_Type"]
    assert res.nonzeros[res.sparsest] <= res.nonzeros[res.best]
    assert res.cv_error[res.sparsest] <= res.cv_error[res.best] + res.cv_se[res.best]
    s.perform_fit()
    assert np.array_equal(s.fit, fit0)
    pt.free()
    return res


def grid_full(res, q):
    return res.grid[q]


@pytest.mark.gpu
def test_solver_surface_on_the_ta_rows(ta):
    A, b, w = ta
    m = len(b)
    conf = np.arange(m) // 50
    testing = np.zeros(m, dtype=bool)
    testing[1::4] = True
    labels = labels_of(conf, np.arange(m) % 3, testing)
    res = surface(A, b, w, labels, {}, [{"scale": 0.01}, {"scale": 1e-3, "itermax": 20}], 5, "ta")
    want = cs.expected("ta_testing")
    assert res.active[0][res.active[0] >= 0].tolist() == want["used"].tolist()
    fit = np.zeros(A.shape[1])
    fit[want["used"]] = want["weights"]
    # the reference's own fit of these rows: its bar plus the device's, both relative to the largest coefficient
    assert np.max(np.abs(res.fits[0] - fit)) <= (cs.REF_BAR + cs.DEVICE_BAR) * np.max(np.abs(fit))


@pytest.mark.gpu
def test_solver_surface_on_synthetic_rows():
    A, b, w, conf, cls = cs.rows(916, 33, per=50)              # 2 000 x 33
    testing = np.arange(len(b)) % 13 == 0
    res = surface(A, b, w, labels_of(conf, cls, testing), {"deletion": "exact"}, GRID, 5, "synthetic")
    assert res.grid[2] == {"scale": 0.01, "sigma2": 0.05, "eta": 1e-8, "itermax": 60}
    assert 0.0 <= res.frequency.min() and res.frequency.max() <= 1.0


@pytest.mark.gpu
def test_wider_systems_take_the_host_route():
    A, b, w, conf, cls = cs.rows(901, 150, per=20)
    pt, s = bcs_solver(A, b, w, labels_of(conf, cls, np.zeros(len(b), dtype=bool)), {"max_active": 70})
    with pytest.raises(ValueError, match="K <= 144"):
        s.bcs_path([0.01], method="device")
    res = s.bcs_path([0.01, 0.1], by="Groups", folds=None, table="stats")
    pt.free()
    assert res.status.shape == (5, 2) and res.active.shape == (2, 70)
    assert res.active[0][res.active[0] >= 0].tolist() == s.used.tolist()
    np.testing.assert_allclose(res.fits[0], s.fit, rtol=0, atol=1e-9 * np.max(np.abs(s.fit)))
    pt = ParallelTools()
    sol = solver_factory.solver("BCS", pt, Config(pt, {"SOLVER": {"solver": "BCS"}}))
    with pytest.raises(RuntimeError, match="perform_fit first"):
        sol.bcs_path([0.01])
    pt.free()


@pytest.mark.gpu
def test_two_ranks_on_one_gpu(tmp_path):
    """Two ranks (peer-to-peer transport, rows dealt round-robin so that every unit spans both): the same bits on both ranks and
    the one-process result (equal picks; numbers to the rounding of statistics summed in another order)."""
    import bcs_path_dist_worker as wk

    procs = []
    for rank in range(2):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE="2",
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="bcs path ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "bcs_path_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    two = [dict(np.load(tmp_path / f"bcs_rank{r}.npz")) for r in range(2)]
    for key in two[0]:
        assert np.array_equal(two[0][key], two[1][key], equal_nan=two[0][key].dtype.kind == "f"), key
    A, b, w, labels = wk.rows()
    pt, s = bcs_solver(A, b, w, labels, wk.SECTION)
    one = wk.path_of(s)
    pt.free()
    got = two[0]
    assert one.margin.min() >= cs.MIN_MARGIN
    assert np.array_equal(got["picks"], one.picks) and np.array_equal(got["active"], one.active)
    assert np.array_equal(got["status"], one.status) and np.array_equal(got["iterations"], one.iterations)
    assert np.array_equal(got["solver_used"], s.used)
    assert got["folds"].tolist() == [f"{k}={v}" for k, v in sorted(one.fold_of_unit.items())]
    assert got["index"].tolist() == [str(x) for x in one.table.index]
    assert got["best"] == one.best and got["sparsest"] == one.sparsest and np.array_equal(got["frequency"], one.frequency)
    np.testing.assert_allclose(got["fits"], one.fits, rtol=0, atol=1e-9 * np.max(np.abs(one.fits)))
    np.testing.assert_allclose(got["covs"], one.covs, rtol=0, atol=1e-9 * np.max(np.abs(one.covs)))
    np.testing.assert_allclose(got["cv_error"], one.cv_error, rtol=1e-8)
    np.testing.assert_allclose(got["table"], one.table.to_numpy(dtype=float), rtol=1e-7)


@pytest.mark.gpu
def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "bcs_sparse_path.py")], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]

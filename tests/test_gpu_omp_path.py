"""GPU: grouped K-fold greedy sparse-selection paths (fsnap_omp_path, csrc/fsnap_omp.hip; Solver.omp_path; the OMP solver)
against the long-double yardstick and the bars of tests/omp_path_cases.py and against the host route
(``omp_path.omp_path_host``): lane-ownership edges, fold and sub-block counts, dead / struck / forced columns and the early end,
determinism, refusals, the solver surface, two ranks, the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import lasso_path as lp
from fitsnap_amd.solvers import omp_path as op
from fitsnap_amd.solvers import solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import omp_path_cases as cs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = cs.LD


def on_device(blocks):
    """(tensor that owns the memory, device address) of hand-made blocks."""
    import torch

    t = torch.from_numpy(np.array(blocks, dtype=np.float64, order="C")).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr()


def path_of_blocks(blocks, K, F, nsub, criterion, forced, S, levels, ctx=None):
    t, ptr = on_device(blocks)
    own = ctx is None
    ctx = _capi.HipContext(0) if own else ctx
    try:
        return ctx.omp_path(ptr, K, F, nsub, criterion, forced, S, levels)
    finally:
        if own:
            ctx.close()
        del t


def accept(blocks, K, F, nsub, criterion, forced, S, levels, out, where):
    """The kernel's (order, path, heldout, coef) against the host route (order, path and coefficients bit for bit: the same
    statements; the held-out sums run in another order) and, problem by problem, against the yardstick within the bars.
    Returns the worst error / bar ratios (coefficients, e_s, held-out)."""
    order, path, held, coef = out
    ho, hp, hh, hc = op.omp_path_host(blocks, K, criterion, forced, S, levels, nsub)
    assert np.array_equal(order, ho), where
    assert np.array_equal(path, hp) and np.array_equal(coef, hc), where
    folds, total = lp.sum_blocks(blocks, nsub)
    tdiag = np.diag(lp.unpack(total, K)[0])
    worst = [0.0, 0.0, 0.0]
    for f in range(F + 1):
        Qm, qv, y2, _, _ = lp.downdated(folds, total, f, K)
        at = {int(lv): coef[f, i] for i, lv in enumerate(levels)}
        wc, we, _, c_ld = cs.check_problem(Qm, qv, y2, tdiag, criterion, forced, S, order[f], path[f], at, where=f"{where} f={f}")
        worst[0], worst[1] = max(worst[0], wc), max(worst[1], we)
        if f < F:
            _, _, bb, nf = lp.unpack(folds[f], K)
            h_ld, bar = cs.heldout_ld(folds[f], K, c_ld)
            for name, h in (("kernel", held), ("host", hh)):
                err = np.abs((np.asarray(h[f, :, 1], dtype=LD) - h_ld).astype(np.float64))
                assert np.all(err <= bar), (where, f, name, "held-out", float(np.max(err / bar)))
                assert np.all(h[f, :, 0] == nf) and np.all(h[f, :, 2] == bb), (where, f, name)
                if name == "kernel":
                    worst[2] = max(worst[2], float(np.max(err / bar)))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("criterion", ["omp", "ols"])
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 128, 129, 144])
def test_kernel_against_the_yardstick_and_the_host_route(K, criterion):
    """K on the per-lane column ownership boundaries, S in {1, min(K, 128)}, F in {2, 5}, nsub in {1, 3}: equal orders at every
    step of every problem, path, held-out errors and the coefficients at the levels {1, S / 2, S} within the bars."""
    ctx = _capi.HipContext(0)
    worst = [0.0, 0.0, 0.0]
    try:
        for F in (2, 5):
            for nsub in (1, 3):
                blocks = cs.case_blocks(500 + K, K, F, nsub)
                for S in sorted({1, min(K, 128)}):
                    levels = sorted({1, max(S // 2, 1), S})
                    out = path_of_blocks(blocks, K, F, nsub, criterion, (), S, levels, ctx)
                    w = accept(blocks, K, F, nsub, criterion, (), S, levels, out, f"K={K} {criterion} F={F} nsub={nsub} S={S}")
                    worst = [max(a, b) for a, b in zip(worst, w)]
    finally:
        ctx.close()
    print(f"K = {K:3d} {criterion}: worst error / bar  coefficients {worst[0]:.3f}  e_s {worst[1]:.3f}  held-out {worst[2]:.3f}", flush=True)


@pytest.mark.gpu
@pytest.mark.parametrize("criterion", ["omp", "ols"])
def test_dead_struck_forced_columns_and_the_early_end(criterion):
    F = 3
    K, A, b, w, fold = cs.edge_rows(F)
    blocks = cs.blocks_ld(A, b, w, fold, F)
    forced = (9, 3, 2)                    # 9 first, the dead 3 skipped without a step, then 2; its duplicate 5 is struck
    levels = [1, 2, 9, 10, K]
    out = path_of_blocks(blocks, K, F, 1, criterion, forced, K, levels)
    accept(blocks, K, F, 1, criterion, forced, K, levels, out, f"edges {criterion}")
    order, path, held, coef = out
    for f in range(F + 1):
        live = K - 2 - (1 if f == 1 else 0)       # column 3 is dead, 5 struck, 7 dead where fold 1 is left out
        assert order[f, :2].tolist() == [9, 2] and 3 not in order[f] and 5 not in order[f]
        assert (7 in order[f]) == (f != 1)
        assert np.all(order[f, :live] >= 0) and np.all(order[f, live:] == -1)
        assert np.all(path[f, live:, 0] == path[f, live - 1, 0]) and np.all(path[f, live:, 1:] == 0.0)
        assert np.array_equal(coef[f, 4], coef[f, 3] if live == 10 else coef[f, 2])
        assert np.all(coef[f][:, [3, 5]] == 0.0)
        if f < F:
            assert np.all(held[f, live:, 1] == held[f, live - 1, 1])
    # a training system without a live column takes no step: e_s = y2 = 0, h = bb_f, zero coefficients (F = 1)
    o1, p1, h1, c1 = path_of_blocks(blocks[:1], K, 1, 1, criterion, (), 4, [1, 4])
    assert np.all(o1[0] == -1) and np.all(p1[0] == 0.0) and not c1[0].any() and np.all(h1[0, :, 1] == h1[0, :, 2])
    assert o1[1, 0] >= 0


@pytest.mark.gpu
def test_bit_identical_runs_permuted_folds_and_sub_sets():
    """Integer rows with unit weights: every sum of blocks is exact, so the total is the same bits whatever the order of the
    folds or the presence of an empty one, and a problem's result must then be the same bits wherever it stands in the call."""
    K, F, S = 70, 5, 40
    rng = np.random.default_rng(41)
    m = 1200
    A = rng.integers(-3, 4, (m, K)).astype(np.float64)
    b = (A[:, :9] @ rng.integers(-2, 3, 9) + rng.integers(-1, 2, m)).astype(np.float64)
    fold = rng.integers(0, F, m)
    fold[fold == 3] = 0                                   # fold 3 is empty
    blocks = cs.blocks_ld(A, b, np.ones(m), fold, F)
    levels = [1, 7, S]
    ctx = _capi.HipContext(0)
    try:
        for criterion in ("omp", "ols"):
            first = path_of_blocks(blocks, K, F, 1, criterion, (2,), S, levels, ctx)
            second = path_of_blocks(blocks, K, F, 1, criterion, (2,), S, levels, ctx)
            assert all(np.array_equal(x, y) for x, y in zip(first, second))
            perm = np.array([4, 2, 0, 3, 1])
            permuted = path_of_blocks(blocks[perm], K, F, 1, criterion, (2,), S, levels, ctx)
            sub = [0, 1, 2, 4]
            subset = path_of_blocks(blocks[sub], K, 4, 1, criterion, (2,), S, levels, ctx)
            for i, (x, p, s) in enumerate(zip(first, permuted, subset)):
                nf = F if i == 2 else F + 1               # the held-out sums have no row for the full problem
                assert np.array_equal(x[np.r_[perm, F][:nf]], p), (criterion, i)
                assert np.array_equal(x[np.r_[sub, F][:nf - 1]], s), (criterion, i)
            # the empty fold's refit is the full fit and it holds nothing out
            assert np.array_equal(first[0][3], first[0][F]) and np.array_equal(first[3][3], first[3][F])
            assert np.all(first[2][3] == 0.0)
            assert len(set(first[0][F].tolist())) == S and first[0][F][0] == 2
    finally:
        ctx.close()


@pytest.mark.gpu
def test_entry_point_argument_checks():
    K, F = 6, 3
    blocks = cs.case_blocks(77, K, F)
    t, ptr = on_device(blocks)
    ctx = _capi.HipContext(0)
    try:
        ctx.omp_path(ptr, K, F, 1, "ols", (1,), 4, [1, 4])
        lib = ctx._lib
        io, do = np.zeros(256, dtype=np.int32), np.zeros(2048)

        def status(K=K, F=F, nsub=1, ptr=ptr, criterion=_capi.OMP_OLS, forced=(), nforced=None, S=4, levels=(1, 4), Q=None,
                   outs=(io, do, do, do)):
            """The status of the raw entry point: nothing in front of it can refuse first."""
            fo = None if forced is None else np.array(list(forced) or [0], dtype=np.int32)
            lv = None if levels is None else np.array(list(levels) or [1], dtype=np.int32)
            return lib.fsnap_omp_path(ctx._h, K, F, nsub, _capi.c_void_p(ptr), criterion, _capi._ptr(fo),
                                      len(forced) if nforced is None else nforced, S, _capi._ptr(lv),
                                      len(levels) if Q is None else Q, *(_capi._ptr(x) for x in outs))

        assert status() == _capi.OK and status(forced=(5, 0)) == _capi.OK and status(levels=(2, 2, 3)) == _capi.OK
        big = (2 << 30) // (8 * (K * K + K + 3))          # F * nsub blocks past FSNAP_CAT_STATS_MAX_BYTES
        for bad in (dict(K=0), dict(K=145), dict(S=0), dict(S=K + 1), dict(F=0), dict(nsub=0), dict(Q=0), dict(levels=()),
                    dict(levels=(2, 1)), dict(levels=(0,)), dict(levels=(5,)), dict(forced=(K,)), dict(forced=(-1,)),
                    dict(forced=(1, 2, 1)), dict(forced=(), nforced=-1), dict(forced=None, nforced=1), dict(criterion=2),
                    dict(criterion=-1), dict(ptr=None), dict(levels=None, Q=1), dict(outs=(None, do, do, do)),
                    dict(outs=(io, None, do, do)), dict(outs=(io, do, None, do)), dict(outs=(io, do, do, None)), dict(nsub=big)):
            assert status(**bad) == _capi.E_ARG, bad
        # S stops at 128 whatever K
        wide = np.zeros((2, 140 * 140 + 140 + 3))
        t2, ptr2 = on_device(wide)
        big_i, big_d = np.zeros(3 * 140, dtype=np.int32), np.zeros(3 * 140 * 140)
        assert status(K=140, F=2, ptr=ptr2, S=129, levels=(1,), outs=(big_i, big_d, big_d, big_d)) == _capi.E_ARG
        assert status(K=140, F=2, ptr=ptr2, S=128, levels=(1,), outs=(big_i, big_d, big_d, big_d)) == _capi.OK
        del t2
        # the binding turns the status into ValueError
        for change in ({"K": 145}, {"steps": 7}, {"levels": [3, 2]}, {"forced": (9,)}, {"criterion": "lars"}):
            kw = {**dict(d_stats_ptr=ptr, K=K, F=F, nsub=1, criterion="ols", forced=(), steps=4, levels=[1, 4]), **change}
            with pytest.raises(ValueError):
                ctx.omp_path(**kw)
    finally:
        ctx.close()
        del t


def omp_solver(A, b, w, labels, section=None, extra=None):
    """An OMP solver fitted on shared arrays that hold (A, b, w) with the labels in pt.fitsnap_dict."""
    pt = ParallelTools()
    d = {"SOLVER": {"solver": "OMP"}, "OMP": dict(section or {})}
    d.update(extra or {})
    s = solver_factory.solver("OMP", pt, Config(pt, d))
    m, K = A.shape
    for name, arr in (("a", A), ("b", b), ("w", w)):
        pt.create_shared_array(name, m, K if name == "a" else 1)
        pt.shared_arrays[name].array[:] = arr
    pt.fitsnap_dict.update(labels)
    s.perform_fit()
    return pt, s


def labels_of(conf, cls, testing):
    return {"Configs": [f"c{i:02d}" for i in conf], "Groups": [f"g{i % 4}" for i in conf], "Testing": list(testing),
            "Row_Type": [("Energy", "Force", "Stress")[k] for k in cls]}


@pytest.mark.gpu
@pytest.mark.parametrize("criterion", ["omp", "ols"])
def test_solver_surface_tables_and_the_fit(criterion):
    """Solver.omp_path on an OMP solver: table="rows" against numpy on least-squares refits on the returned fold orders,
    table="stats" against the held-out sums, the device route against the host route, OMP.perform_fit against the full problem
    at ``terms``; neither the fit nor the resident rows change."""
    K, S, terms = 31, 24, 9
    A, b, w, conf, cls = cs.rows(800, K)
    testing = np.arange(len(b)) % 13 == 0
    pt, s = omp_solver(A, b, w, labels_of(conf, cls, testing), {"terms": terms, "criterion": criterion, "forced": "6"})
    fit0, order0 = s.fit.copy(), s.order.copy()
    ctx = pt.hip()
    before = ctx.download_rows()
    levels = [1, 4, terms, S]
    res = s.omp_path(S, levels=levels, criterion=criterion, forced=(6,), folds=5, seed=2, method="device", table="rows")
    stats = s.omp_path(S, levels=levels, criterion=criterion, forced=(6,), folds=5, seed=2, method="device", table="stats")
    host = s.omp_path(S, levels=levels, criterion=criterion, forced=(6,), folds=5, seed=2, method="host", table="rows")
    auto = s.omp_path(S, criterion=criterion, folds=None, table="auto")            # 60 configurations, each its own fold
    after = ctx.download_rows()
    assert all(np.array_equal(x, y) for x, y in zip(before, after)) and np.array_equal(s.fit, fit0)
    s.perform_fit()
    assert np.array_equal(s.fit, fit0) and np.array_equal(s.order, order0)
    pt.free()
    F = 5
    assert res.terms.tolist() == list(range(1, S + 1)) and res.levels.tolist() == levels and res.fits.shape == (4, K)
    assert res.order.shape == (S,) and res.fold_orders.shape == (F, S) and res.order[0] == 6 and np.all(res.fold_orders[:, 0] == 6)
    assert set(res.fold_of_unit.values()) == set(range(F)) and len(res.fold_of_unit) == 60
    # the device and the host route: the same bits in orders, fits and training errors
    assert np.array_equal(host.order, res.order) and np.array_equal(host.fold_orders, res.fold_orders)
    assert np.array_equal(host.fits, res.fits) and np.array_equal(host.train_sse, res.train_sse)
    np.testing.assert_allclose(host.cv_error, res.cv_error, rtol=1e-11)
    assert host.best == res.best and host.sparsest == res.sparsest
    # the OMP fit is the full problem at ``terms`` (its statistics are summed in another order than the folds')
    assert np.array_equal(order0, res.order[:terms]) and np.count_nonzero(fit0) == terms
    np.testing.assert_allclose(fit0, res.fits[2], rtol=1e-9, atol=1e-12 * np.max(np.abs(fit0)))
    assert np.all(np.diff(res.train_sse) <= 0)
    # table="rows": refit every fold's support by least squares in numpy and score the held-out rows
    train = ~testing
    fold = np.array([res.fold_of_unit[f"c{i:02d}"] for i in conf])
    names = ["Energy", "Force", "Stress"]
    for lv in levels:
        pooled = np.zeros((3, 4))
        for f in range(F):
            sup = res.fold_orders[f, :lv]
            tr = train & (fold != f)
            beta = np.linalg.lstsq(A[tr][:, sup] * w[tr, None], b[tr] * w[tr], rcond=None)[0]
            out = train & (fold == f)
            r = b[out] - A[out][:, sup] @ beta
            for k in range(3):
                sel = cls[out] == k
                pooled[k] += (sel.sum(), np.abs(r[sel]).sum(), (r[sel] ** 2).sum(), ((w[out][sel] * r[sel]) ** 2).sum())
        for k, name in enumerate(names):
            row = res.table.loc[(lv, name)]
            assert row["ncount"] == pooled[k, 0]
            np.testing.assert_allclose([row["mae"], row["rmse"], row["w_rmse"]],
                                       [pooled[k, 1] / pooled[k, 0], np.sqrt(pooled[k, 2] / pooled[k, 0]),
                                        np.sqrt(pooled[k, 3] / pooled[k, 0])], rtol=1e-8)
        allrow = res.table.loc[(lv, "*ALL")]
        assert allrow["ncount"] == train.sum()
        # the statistics form of the weighted error: the table, the curve and the rows agree
        np.testing.assert_allclose(allrow["w_rmse"] ** 2, pooled[:, 3].sum() / train.sum(), rtol=1e-8)
        np.testing.assert_allclose(stats.table.loc[(lv, "*ALL"), "w_rmse"] ** 2, stats.cv_error[lv - 1], rtol=1e-13)
        np.testing.assert_allclose(stats.cv_error[lv - 1], allrow["w_rmse"] ** 2, rtol=1e-8)
    assert list(stats.table.index.names) == ["terms", "Row_Type"] and list(res.table.index.names) == ["terms", "Row_Type"]
    assert np.array_equal(stats.fits, res.fits) and np.array_equal(stats.cv_error, res.cv_error)
    # the picks
    err, se, best, sparsest = op.cv_picks(res.terms, np.stack([np.ones((F, S)), np.tile(res.cv_error, (F, 1)), np.ones((F, S))], axis=2))
    assert res.best == int(np.argmin(res.cv_error)) == best and res.best_terms == res.best + 1
    assert res.sparsest_terms <= res.best_terms and res.cv_error[res.sparsest] <= res.cv_error[res.best] + res.cv_se[res.best]
    assert all(res.cv_error[q] > res.cv_error[res.best] + res.cv_se[res.best] for q in range(res.sparsest))
    np.testing.assert_array_equal(res.frequency, op.selection_frequency(res.fold_orders, res.best_terms, K))
    assert res.frequency[6] == 1.0 and 0.0 <= res.frequency.min() and res.frequency.max() <= 1.0
    # every configuration its own fold: 61 problems, the default ladder, the statistics table past 512 vectors
    assert auto.fold_orders.shape == (60, S) and auto.levels.tolist() == op.default_levels(S).tolist()
    assert set(k[1] for k in auto.table.index) == {"*ALL"} and auto.best is not None


@pytest.mark.gpu
def test_wider_systems_take_the_host_route_and_refusals():
    K, S = 160, 40
    A, b, w, conf, cls = cs.rows(801, K)
    labels = labels_of(conf, cls, np.zeros(len(b), dtype=bool))
    pt, s = omp_solver(A, b, w, labels, {"terms": 30})
    with pytest.raises(ValueError, match="K <= 144"):
        s.omp_path(S, method="device")
    with pytest.raises(ValueError, match="max_terms"):
        s.omp_path(K + 1)
    res = s.omp_path(S, levels=[30, S], by="Groups", folds=None, table="stats")
    pt.free()
    assert res.fold_orders.shape == (4, S) and np.array_equal(res.order[:30], s.order)
    np.testing.assert_allclose(res.fits[0], s.fit, rtol=1e-9, atol=1e-12 * np.max(np.abs(s.fit)))
    fold = conf % 4
    blocks = cs.blocks_ld(A, b, w, fold, 4)
    order = op.omp_path_host(blocks, K, "ols", (), S, [30, S])[0]
    assert np.array_equal(order[4], res.order) and np.array_equal(order[:4], res.fold_orders)
    pt = ParallelTools()
    for name, extra, match in (("RIDGE", {}, "has no selection path"), ("LASSO", {}, "has no selection path"),
                               ("OMP", {"EXTRAS": {"apply_transpose": 1}}, "apply_transpose")):
        sol = solver_factory.solver(name, pt, Config(pt, {"SOLVER": {"solver": name}, **extra}))
        with pytest.raises(ValueError, match=match):
            sol.omp_path(5)
    sol = solver_factory.solver("OMP", pt, Config(pt, {"SOLVER": {"solver": "OMP"}}))
    with pytest.raises(RuntimeError, match="perform_fit first"):
        sol.omp_path(5)
    pt.free()


@pytest.mark.gpu
def test_two_ranks_on_one_gpu(tmp_path):
    """Two ranks (peer-to-peer transport, rows dealt round-robin so that every unit spans both): the same bits on both ranks and
    the one-process result (equal orders; numbers to the rounding of statistics summed in another order)."""
    import omp_path_dist_worker as wk

    procs = []
    for rank in range(2):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE="2",
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="omp path ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "omp_path_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    two = [dict(np.load(tmp_path / f"omp_rank{r}.npz")) for r in range(2)]
    for key in two[0]:
        assert np.array_equal(two[0][key], two[1][key], equal_nan=two[0][key].dtype.kind == "f"), key
    A, b, w, labels = wk.rows()
    pt, s = omp_solver(A, b, w, labels, wk.SECTION)
    one = wk.path_of(s)
    pt.free()
    got = two[0]
    assert np.array_equal(got["order"], one.order) and np.array_equal(got["fold_orders"], one.fold_orders)
    assert np.array_equal(got["solver_order"], s.order) and np.array_equal(got["levels"], one.levels)
    assert got["folds"].tolist() == [f"{k}={v}" for k, v in sorted(one.fold_of_unit.items())]
    assert got["index"].tolist() == [str(x) for x in one.table.index]
    assert got["best"] == one.best and got["sparsest"] == one.sparsest and np.array_equal(got["frequency"], one.frequency)
    np.testing.assert_allclose(got["fits"], one.fits, rtol=1e-9, atol=1e-12 * np.max(np.abs(one.fits)))
    np.testing.assert_allclose(got["train_sse"], one.train_sse, rtol=1e-9)
    np.testing.assert_allclose(got["cv_error"], one.cv_error, rtol=1e-9)
    np.testing.assert_allclose(got["table"], one.table.to_numpy(dtype=float), rtol=1e-8)


@pytest.mark.gpu
def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "omp_sparse_path.py")], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]

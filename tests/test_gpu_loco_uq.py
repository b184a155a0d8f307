"""GPU: leave-one-configuration-out predictive variances (fsnap_loco_rows_uq, csrc/fsnap_loco_uq.hip;
Solver.loco_predictive) against long-double refits (tests/loco_uq_cases.py) under a-priori rounding bars and an RMS
comparison with loco_uq_host: a sweep of K, J (J = K and J < K factors) and unit sizes on every tile and bin edge, the
predictions bit for bit those of fsnap_loco_rows, the layout and edge cases (empty units, unlisted and zero-weight rows, a
unit that is not identifiable, shuffled units and subsets, repeats, argument errors), the three entry points that share one
staging front on one context in both orders, the solver method against its host route, and two ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import loco, loco_uq, solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loco_cases as lc  # noqa: E402
import loco_uq_cases as uc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = lc.EPS


def make_solver(name, extra=None):
    pt = ParallelTools()
    d = {"SOLVER": {"solver": name}}
    d.update(extra or {})
    return pt, solver_factory.solver(name, pt, Config(pt, d))


def upload(A, b, w, mask=None):
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w, None if mask is None else mask.astype(np.uint8))
    return ctx


def same_bits(x, y):
    return np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 17, 33, 64, 128, 145])
@pytest.mark.parametrize("alpha", [0.0, 1e-4])
def test_kernel_matches_long_double_refits(K, alpha):
    """Every q_i, D_c and l_c of the sweep of loco_cases (unit sizes on every tile and bin edge, the n / J space switch at
    J - 1, J, J + 1 and the global-scratch path, in shuffled order; J = K and J in {1, 15, K - 1}; K = 145 takes kernel L1's
    NT = 0 form) against the long-double refit -- all units below K = 128, the boundary-size units from there on, loco_uq_host
    for the fillers -- under the a-priori bars and the RMS condition of loco_uq_cases; the predictions and the first four
    info columns are those of fsnap_loco_rows bit for bit."""
    A, b, w, G, c, stats = lc.sweep_rows(K)
    m = len(b)
    rows = np.arange(m, dtype=np.int32)
    ctx = upload(A, b, w)
    try:
        for J in [J for J in lc.sweep_js(K) if J in (K, 1, 15, K - 1)]:
            off, boundary = lc.sweep_units(K, J, m)
            M, beta = lc.sweep_factor(G, c, alpha, J, stats)
            pred0, info0 = ctx.loco_rows(M, beta, rows, off)
            pred, lev, info = ctx.loco_rows_uq(M, beta, rows, off)
            tag = f"sweep K={K} alpha={alpha:g} J={J}"
            assert same_bits(pred, pred0) and same_bits(info[:, :4], info0), tag
            assert np.all(info[:, 2] == 1.0), tag
            res = uc.measure_cell(A, b, w, alpha, M, beta, rows, off, lev, info, stats, None if K < 128 else boundary)
            uc.check_cell(tag, res)
            ld = np.isfinite(res["truth_pred"])
            assert np.max(np.abs(pred[ld] - res["truth_pred"][ld])) <= 1e-9 * np.max(np.abs(b)), tag
    finally:
        ctx.close()


def edge_problem(alpha):
    """K = 33: units of 20 (zero-weight rows inside), 0, 40 (alone on column 7), 33, 34, 70 and 16 rows; the rows of the last
    unit are left unlisted when asked."""
    sizes = [20, 0, 40, 33, 34, 70, 16]
    A, b, w, labels = lc.config_rows(21, 33, sizes)
    cfg = np.asarray(labels["Configs"])
    A[:, 7] = 0.0
    A[cfg == "cfg2", 7] = 1.0 + 0.05 * np.arange(40)
    w[[3, 11]] = 0.0                                             # inside unit 0 (n space at J = 33, J space at J = 15)
    Aw, bw = A * w[:, None], b * w
    G, c = Aw.T @ Aw, Aw.T @ bw
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return A, b, w, G, c, off


@pytest.mark.gpu
@pytest.mark.parametrize("J", [33, 15])
def test_layout_and_edge_cases(J):
    K = 33
    for alpha in (0.0, 1e-4):
        A, b, w, G, c, off = edge_problem(alpha)
        m = len(b)
        if J == K:
            M = loco.factor_cholesky(G, alpha)
            beta = np.linalg.solve(G + alpha * np.eye(K), c)
        else:
            M = loco.factor_eigen(G, alpha, rank=J)
            beta = M @ (M.T @ c)
        rows = np.arange(off[-2], dtype=np.int32)               # the 16 rows of the last unit are not listed
        offs = off[:-1]
        ctx = upload(A, b, w)
        try:
            pred0, info0 = ctx.loco_rows(M, beta, rows, offs)
            pred, lev, info = ctx.loco_rows_uq(M, beta, rows, offs)
            again = ctx.loco_rows_uq(M, beta, rows, offs)
            # shuffled units, and a subset of them
            perm = np.array([4, 0, 5, 2, 1, 3])
            prow = np.concatenate([rows[offs[u]:offs[u + 1]] for u in perm]).astype(np.int32)
            poff = np.concatenate([[0], np.cumsum(np.diff(offs)[perm])]).astype(np.int64)
            shuffled = ctx.loco_rows_uq(M, beta, prow, poff)
            keep = np.array([5, 0, 3])
            srow = np.concatenate([rows[offs[u]:offs[u + 1]] for u in keep]).astype(np.int32)
            soff = np.concatenate([[0], np.cumsum(np.diff(offs)[keep])]).astype(np.int64)
            subset = ctx.loco_rows_uq(M, beta, srow, soff)
        finally:
            ctx.close()
        hpred, hlev, hinfo = loco_uq.loco_uq_host(A, b, w, M, beta, rows, offs)
        assert same_bits(pred, pred0) and same_bits(info[:, :4], info0)
        for x, y in zip((pred, lev, info), again):
            assert same_bits(x, y)                                                     # two runs
        assert same_bits(shuffled[0], pred) and same_bits(shuffled[1], lev) and same_bits(shuffled[2], info[perm])
        listed = np.zeros(m, dtype=bool)
        listed[srow] = True
        assert same_bits(subset[0][listed], pred[listed]) and same_bits(subset[1][listed], lev[listed])
        assert np.all(np.isnan(subset[1][~listed])) and same_bits(subset[2], info[keep])
        assert info[1].tolist() == [0, np.inf, 1, 1, 0, 0]                             # the empty unit
        assert np.all(np.isnan(lev[off[-2]:])) and np.all(np.isnan(pred[off[-2]:]))   # rows that are not listed
        # the unit that alone touches column 7: not identifiable without a ridge (J = K), and the call still succeeds
        ident = bool(hinfo[2, 2])
        assert info[2, 2] == hinfo[2, 2] and (ident or alpha == 0.0) and not (ident and alpha == 0.0 and J == K)
        r2 = rows[offs[2]:offs[3]]
        if not ident:
            assert np.all(np.isnan(lev[r2])) and np.all(np.isnan(pred[r2])) and np.all(np.isnan(info[2, 4:]))
        good = np.array([u for u in range(6) if u != 1 and (ident or u != 2)])
        fin = np.concatenate([rows[offs[u]:offs[u + 1]] for u in good])
        assert np.all(np.isfinite(lev[fin])) and np.all(lev[[3, 11]] > 0.0)           # zero-weight rows have a leverage
        assert np.array_equal(info[:, 3], hinfo[:, 3]) and np.array_equal(info[:, 0], hinfo[:, 0])
        for u in good:
            r = rows[offs[u]:offs[u + 1]]
            mid = lc.unit_reference(A, b, w, r, M, beta, precise=False)
            bq, bd, bl = uc.uq_bars(A[r], b[r], w[r], M, beta, mid["lam_min"], mid["d"], w[r] * (b[r] - hpred[r]), hinfo[u, 4])
            assert np.all(np.abs(lev[r] - hlev[r]) <= 2 * bq), (alpha, u)              # two float64 routes: each within its bar
            assert abs(info[u, 5] - hinfo[u, 5]) <= 2 * bd and abs(info[u, 4] - hinfo[u, 4]) <= 2 * bl, (alpha, u)


@pytest.mark.gpu
def test_entry_points_share_buffers_and_leave_no_state():
    """fsnap_loco_rows, fsnap_loco_rows_uq and fsnap_influence_rows (FULL) on one context, in that order and then in the
    reverse order, at K = J = 144 with one unit in each bin (8, 40, 100 rows: the LDS classes 32, 64, 128; 140 rows: global
    scratch, dmax = 140, whose slice differs between the first and the other two).  They stage the same buffers: the
    predictions and the first four info columns have the same bits from all three and in both orders, and so has everything
    else an entry point returns (leverages, unit records, vectors, sums) between the two orders."""
    K, alpha, sizes = 144, 1e-4, [8, 40, 100, 140]
    A, b, w, _ = lc.config_rows(33, K, sizes)
    Aw, bw = A * w[:, None], b * w
    G, c = Aw.T @ Aw, Aw.T @ bw
    M = loco.factor_cholesky(G, alpha)
    beta = np.linalg.solve(G + alpha * np.eye(K), c)
    rows = np.arange(len(b), dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    calls = {
        "loco": lambda ctx: dict(zip(("pred", "info"), ctx.loco_rows(M, beta, rows, off))),
        "uq": lambda ctx: dict(zip(("pred", "lev", "info"), ctx.loco_rows_uq(M, beta, rows, off))),
        "infl": lambda ctx: ctx.influence_rows(M, beta, rows, off, mode=_capi.INFL_FULL),
    }
    ctx = upload(A, b, w)
    try:
        forward = {name: calls[name](ctx) for name in ("loco", "uq", "infl")}
        backward = {name: calls[name](ctx) for name in ("infl", "uq", "loco")}
    finally:
        ctx.close()
    ref = forward["loco"]
    assert ref["info"][:, 0].tolist() == sizes and np.all(ref["info"][:, 2] == 1.0)      # d_c = n_c: one unit per bin
    assert np.all(np.isfinite(ref["pred"]))
    for order in (forward, backward):
        for name, out in order.items():
            assert same_bits(out["pred"], ref["pred"]) and same_bits(out["info"][:, :4], ref["info"]), name
    assert np.all(np.isfinite(forward["uq"]["lev"])) and np.all(np.isfinite(forward["infl"]["unit"]))
    for name, out in forward.items():
        for key, x in out.items():
            assert same_bits(x, backward[name][key]), (name, key)


@pytest.mark.gpu
def test_entry_point_argument_checks():
    K = 5
    A, b, w, labels = lc.config_rows(2, K, [6, 7, 8])
    ctx = upload(A, b, w)
    try:
        m = len(b)
        lib = ctx._lib
        M, beta = np.eye(K) * 0.01, np.zeros(K)
        rows, off = np.arange(m, dtype=np.int32), np.array([0, 6, 13, 21], dtype=np.int64)
        pred, lev, info = np.empty(m), np.empty(m), np.empty((3, 6))

        def status(K=K, J=K, M=M, beta=beta, rows=rows, off=off, ncfg=3, outs=(pred, lev, info)):
            """The status of the raw entry point: nothing in front of it can refuse first."""
            return lib.fsnap_loco_rows_uq(ctx._h, K, J, _capi._ptr(M), _capi._ptr(beta), _capi._ptr(rows), _capi._ptr(off), ncfg,
                                          *(_capi._ptr(x) for x in outs))

        assert status() == _capi.OK
        dup = rows.copy()
        dup[1] = 0
        far = rows.copy()
        far[2] = m
        for bad in (dict(K=0), dict(K=K + 1), dict(J=0), dict(ncfg=-1), dict(M=None), dict(beta=None), dict(off=None),
                    dict(rows=None), dict(outs=(None, lev, info)), dict(outs=(pred, None, info)), dict(outs=(pred, lev, None)),
                    dict(off=np.array([1, 6, 13, 21], dtype=np.int64)), dict(off=np.array([0, 7, 6, 21], dtype=np.int64)),
                    dict(off=np.array([0, 6, 13, 22], dtype=np.int64)), dict(rows=dup), dict(rows=far)):
            assert status(**bad) == _capi.E_ARG, bad
            # fsnap_loco_rows refuses the same arguments
            if "outs" not in bad:
                a = dict(K=K, J=K, M=M, beta=beta, rows=rows, off=off, ncfg=3)
                a.update(bad)
                assert lib.fsnap_loco_rows(ctx._h, a["K"], a["J"], _capi._ptr(a["M"]), _capi._ptr(a["beta"]), _capi._ptr(a["rows"]),
                                           _capi._ptr(a["off"]), a["ncfg"], _capi._ptr(pred), _capi._ptr(info)) == _capi.E_ARG, bad
    finally:
        ctx.close()


def class_problem():
    sizes = [9 + (5 * c) % 37 for c in range(18)]
    return lc.config_rows(9, 12, sizes, testing_frac=0.15)


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra", [("ANL", {}), ("RIDGE", {"RIDGE": {"alpha": 1e-6}})])
def test_solver_method_device_against_host(name, extra, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                                  # ANL saves covariance.npy / mean.npy into the cwd
    A, b, w, labels = class_problem()
    test = np.asarray(labels["Testing"])
    w[np.flatnonzero(~test)[5]] = 0.0
    pt, s = make_solver(name, extra)
    if name == "ANL":                                            # fits the shared rows; labels, truths and weights from pt
        pt.create_shared_array("a", *A.shape)
        pt.create_shared_array("b", len(b))
        pt.create_shared_array("w", len(b))
        pt.shared_arrays["a"].array[:] = A
        pt.shared_arrays["b"].array[:] = b
        pt.shared_arrays["w"].array[:] = w
        pt.fitsnap_dict = dict(labels)
        s.save_files = False
        s.perform_fit()
        given = {}
    else:
        s.perform_fit(A, b, w[~test], fs_dict=labels)
        given = dict(fs_dict=labels, b=b, w=w[~test])
    dev = s.loco_predictive(method="device", **given)
    host = s.loco_predictive(method="host", **given)
    auto = s.loco_predictive(**given)
    errs = s.loco_errors(**given)
    assert same_bits(dev.pred, errs.preds) and same_bits(auto.pred, dev.pred) and same_bits(auto.leverage, dev.leverage)
    if name == "ANL":
        assert dev.noise == s.sigmahat
    else:
        wf = np.zeros(len(b))
        wf[~test] = w[~test]
        res = wf * (b - A @ s.fit)
        M = loco.smoother_factor(s)[1]
        np.testing.assert_allclose(dev.noise, (res @ res) / ((~test).sum() - loco_uq.smoother_trace(s.last_statistics[0], M)),
                                   rtol=1e-9)
    assert dev.noise == host.noise and dev.summary["unidentifiable"] == 0 and dev.summary["units"] == 18
    assert np.all(np.isnan(dev.pred[test])) and np.all(np.isnan(dev.var[test])) and np.all(np.isnan(dev.z[test]))
    zero = np.flatnonzero(~test)[5]
    assert np.isfinite(dev.leverage[zero]) and np.isnan(dev.z[zero]) and np.isnan(dev.var[zero])
    # tolerance: every q_i, D_c, l_c of either route lies within its bar of the truth, the bars of these 12-column units of
    # lambda_min >= 0.05 are at most 4 eps (K + J + d) / 0.05^2 = 6e4 eps relative to the quantities' own scale, and a
    # table entry is a mean of n such terms: 1e-10 relative, with the same absolute floor
    tol = dict(rtol=1e-10, atol=1e-10)
    assert list(dev.tables.index) == list(host.tables.index) and list(dev.tables.columns) == loco_uq.TABLE_COLUMNS
    np.testing.assert_allclose(dev.tables.to_numpy(dtype=float), host.tables.to_numpy(dtype=float), **tol)
    for k in ("logdens", "mean_z2", "calibrated_noise"):
        np.testing.assert_allclose(dev.summary[k], host.summary[k], **tol)
    num = ["rows", "rows_weighted", "d", "distance", "logdet", "logdens"]
    np.testing.assert_allclose(dev.units[num].to_numpy(dtype=float), host.units[num].to_numpy(dtype=float), **tol)
    assert dev.tables.loc[("*ALL", "*ALL"), "n"] == int((~test).sum()) - 1
    assert dev.units["rows_weighted"].sum() == int((~test).sum()) - 1
    live = ~test & (w > 0)
    np.testing.assert_allclose(dev.var[live], dev.noise * (1 / w[live] ** 2 + dev.leverage[live]), rtol=1e-14)
    pt.free()


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path, monkeypatch):
    world = 2
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="loco uq two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "loco_uq_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    parts = [dict(np.load(tmp_path / f"loco_uq_rank{r}.npz")) for r in range(world)]
    assert all(str(p["split"]) == "refused" for p in parts)          # a unit with rows on both ranks raises on every rank
    sizes = [12 + (7 * c) % 90 for c in range(40)]
    A, b, w, labels = lc.config_rows(5, 31, sizes, testing_frac=0.1)
    test = np.asarray(labels["Testing"])
    monkeypatch.chdir(tmp_path)
    pt, s = make_solver("RIDGE", {"RIDGE": {"alpha": 1e-6}})
    s.perform_fit(A, b, w[~test], fs_dict=labels)
    one = s.loco_predictive(fs_dict=labels, b=b, w=w[~test])
    assert parts[1]["noise"] == parts[0]["noise"]
    np.testing.assert_allclose(parts[0]["noise"], one.noise, rtol=1e-10)
    # per row: the ranks' statistics are summed in another order than one rank's, so M and beta differ in the last bits
    for p in parts:
        for k, x in (("pred", one.pred), ("leverage", one.leverage), ("z", one.z)):
            np.testing.assert_allclose(p[k], x[p["rows"]], rtol=1e-9, atol=1e-9, equal_nan=True)
    assert [str(x) for x in one.tables.index] == parts[0]["index"].tolist()
    np.testing.assert_allclose(parts[0]["tables"], one.tables.to_numpy(dtype=float), rtol=1e-9, atol=1e-9)
    for k in ("logdens", "mean_z2", "calibrated_noise", "units", "unidentifiable"):
        np.testing.assert_allclose(parts[0]["summary_" + k], one.summary[k], rtol=1e-9)
    # the pooled unit frame holds every unit once
    assert sorted(parts[0]["unit_names"].tolist()) == sorted(one.units["Configs"].tolist())
    pt.free()

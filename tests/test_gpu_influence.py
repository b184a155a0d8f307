"""GPU: influence vectors and the sums of the cluster-robust covariances (fsnap_influence_rows, csrc/fsnap_influence.hip;
Solver.influence) against long double (tests/influence_cases.py) under a-priori rounding bars and an RMS comparison with
influence_host: loco_cases' sweep of K, J and unit sizes on every tile and bin edge with the predictions bit for bit those of
fsnap_loco_rows, SCORES against FULL mode, the layout and edge cases (an empty unit, unlisted and zero-weight rows, a unit that
is not identifiable, shuffled units and subsets, repeats, ncfg = 0, argument errors), the solver method against its host route,
two ranks, and one statistical sanity case."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import influence as infl
from fitsnap_amd.solvers import solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import influence_cases as ic  # noqa: E402
import loco_cases as lc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("pred", "info", "unit", "S", "V", "Ws", "Wv")


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
def test_kernel_matches_long_double(K, alpha):
    """Every s_c, v_c, unit record, W_s and W_v of the sweep of loco_cases (unit sizes on every tile and bin edge, the n / J
    space switch at J - 1, J, J + 1 and the global-scratch path, in shuffled order; J = K and J in {1, 15, K - 1}; K = 145 takes
    kernel L1's NT = 0 form) against long double -- all units below K = 128, the boundary-size units from there on,
    influence_host for the fillers -- under the a-priori bars and the RMS condition of influence_cases; pred and info are those
    of fsnap_loco_rows bit for bit, and SCORES mode gives FULL mode's S, |s_c|^2 and W_s bit for bit."""
    A, b, w, G, c, stats = lc.sweep_rows(K)
    m = len(b)
    rows = np.arange(m, dtype=np.int32)
    ctx = upload(A, b, w)
    try:
        for J in ic.sweep_js(K):
            off, boundary = lc.sweep_units(K, J, m)
            M, beta = lc.sweep_factor(G, c, alpha, J, stats)
            pred0, info0 = ctx.loco_rows(M, beta, rows, off)
            out = ctx.influence_rows(M, beta, rows, off)
            scores = ctx.influence_rows(M, beta, rows, off, mode=_capi.INFL_SCORES)
            tag = f"sweep K={K} alpha={alpha:g} J={J}"
            assert same_bits(out["pred"], pred0) and same_bits(out["info"], info0), tag
            assert np.all(out["info"][:, 2] == 1.0), tag
            assert same_bits(scores["S"], out["S"]) and same_bits(scores["Ws"], out["Ws"]), tag
            assert same_bits(scores["unit"][:, 1], out["unit"][:, 1]) and np.all(np.isnan(scores["unit"][:, [0, 2]])), tag
            assert np.array_equal(scores["info"][:, [0, 2, 3]], info0[:, [0, 2, 3]]) and np.all(np.isinf(scores["info"][:, 1]))
            assert same_bits(out["Ws"], out["Ws"].T) and same_bits(out["Wv"], out["Wv"].T), tag
            res = ic.measure_cell(A, b, w, M, beta, rows, off, out, None if K < 128 else boundary)
            ic.check_cell(tag, res)
    finally:
        ctx.close()


def permuted(rows, offs, order):
    prow = np.concatenate([rows[offs[u]:offs[u + 1]] for u in order]).astype(np.int32)
    poff = np.concatenate([[0], np.cumsum(np.diff(offs)[order])]).astype(np.int64)
    return prow, poff


@pytest.mark.gpu
@pytest.mark.parametrize("J", [33, 15])
def test_layout_and_edge_cases(J):
    K = 33
    for alpha in (0.0, 1e-4):
        A, b, w, G, c, off = ic.edge_problem(alpha)
        m = len(b)
        M, beta = ic.edge_factor(G, c, alpha, J)
        rows = np.arange(off[-2], dtype=np.int32)               # the 16 rows of the last unit are not listed
        offs = off[:-1]
        perm, keep = np.array([4, 0, 5, 2, 1, 3]), np.array([5, 0, 3])
        ctx = upload(A, b, w)
        try:
            pred0, info0 = ctx.loco_rows(M, beta, rows, offs)
            out = ctx.influence_rows(M, beta, rows, offs)
            again = ctx.influence_rows(M, beta, rows, offs)
            scores = ctx.influence_rows(M, beta, rows, offs, mode=_capi.INFL_SCORES)
            shuffled = ctx.influence_rows(M, beta, *permuted(rows, offs, perm))
            srow, soff = permuted(rows, offs, keep)
            subset = ctx.influence_rows(M, beta, srow, soff)
            none = ctx.influence_rows(M, beta, np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64))
        finally:
            ctx.close()
        host = infl.influence_host(A, b, w, M, beta, rows, offs)
        assert same_bits(out["pred"], pred0) and same_bits(out["info"], info0)
        for k in KEYS:
            assert same_bits(out[k], again[k]), k                                     # two runs, W included
        assert same_bits(scores["S"], out["S"]) and same_bits(scores["Ws"], out["Ws"])
        assert same_bits(scores["unit"][:, 1], out["unit"][:, 1])
        # per-unit outputs under a shuffle and a subset of the units (W depends on the order of the units: under its bar only)
        assert same_bits(shuffled["pred"], out["pred"])
        for k in ("info", "unit", "S", "V"):
            assert same_bits(shuffled[k], out[k][perm]) and same_bits(subset[k], out[k][keep]), k
        listed = np.zeros(m, dtype=bool)
        listed[srow] = True
        assert same_bits(subset["pred"][listed], out["pred"][listed]) and np.all(np.isnan(subset["pred"][~listed]))
        assert none["info"].shape == (0, 4) and not none["Ws"].any() and not none["Wv"].any() and none["Ws"].shape == (J, J)
        assert np.all(np.isnan(none["pred"])) and none["S"].shape == (0, J)
        # the empty unit, and rows that are not listed
        assert out["info"][1].tolist() == [0, np.inf, 1, 1] and not out["unit"][1].any()
        assert not out["S"][1].any() and not out["V"][1].any() and np.all(np.isnan(out["pred"][off[-2]:]))
        # the unit that alone touches column 7: not identifiable without a ridge (J = K), and the call still succeeds
        ident = bool(host["info"][2, 2])
        assert out["info"][2, 2] == host["info"][2, 2] and (ident or alpha == 0.0) and not (ident and alpha == 0.0 and J == K)
        if not ident:
            assert not out["V"][2].any() and np.isnan(out["unit"][2, 0]) and np.isnan(out["unit"][2, 2])
            assert np.all(np.isfinite(out["S"][2])) and out["S"][2].any() and out["unit"][2, 1] > 0
        good = np.array([u for u in range(6) if u != 1 and (ident or u != 2)])
        assert np.all(np.isfinite(out["V"][good])) and np.all(np.isfinite(out["unit"][good]))
        # against the reference: every unit under its bar, W_s over all units and W_v over the identifiable ones
        res = ic.measure_cell(A, b, w, M, beta, rows, offs, out, host=host)
        print(ic.cell_line(f"layout J={J} alpha={alpha:g}", res), flush=True)
        for k in ("s", "ss"):
            assert np.max(res["ratio_" + k]) <= 1.0, (alpha, k)
        for k in ("v", "vv", "sv"):
            assert np.max(res["ratio_" + k][good]) <= 1.0, (alpha, k)
        assert res["ratio_Ws"] <= 1.0 and res["ratio_Wv"] <= 1.0
        # W of the shuffled units: another order of the same terms, under the same bar
        prow, poff = permuted(rows, offs, perm)
        pres = ic.measure_cell(A, b, w, M, beta, prow, poff, shuffled)
        assert pres["ratio_Ws"] <= 1.0 and pres["ratio_Wv"] <= 1.0


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
        pred, info, unit = np.empty(m), np.empty((3, 4)), np.empty((3, 3))
        S, V, Ws, Wv = np.empty((3, K)), np.empty((3, K)), np.empty((K, K)), np.empty((K, K))

        def status(mode=_capi.INFL_FULL, K=K, J=K, M=M, beta=beta, rows=rows, off=off, ncfg=3,
                   outs=(pred, info, unit, S, V, Ws, Wv)):
            """The status of the raw entry point: nothing in front of it can refuse first."""
            return lib.fsnap_influence_rows(ctx._h, mode, K, J, _capi._ptr(M), _capi._ptr(beta), _capi._ptr(rows),
                                            _capi._ptr(off), ncfg, *(_capi._ptr(x) for x in outs))

        assert status() == _capi.OK
        assert status(outs=(None, info, unit, None, None, None, None)) == _capi.OK
        assert status(mode=_capi.INFL_SCORES, outs=(None, info, unit, S, None, Ws, None)) == _capi.OK
        dup = rows.copy()
        dup[1] = 0
        far = rows.copy()
        far[2] = m
        for bad in (dict(mode=2), dict(mode=-1), dict(K=0), dict(K=K + 1), dict(J=0), dict(ncfg=-1), dict(M=None), dict(beta=None),
                    dict(off=None), dict(rows=None), dict(outs=(pred, None, unit, S, V, Ws, Wv)),
                    dict(outs=(pred, info, None, S, V, Ws, Wv)),
                    dict(mode=_capi.INFL_SCORES, outs=(None, info, unit, S, V, Ws, None)),
                    dict(mode=_capi.INFL_SCORES, outs=(None, info, unit, S, None, Ws, Wv)),
                    dict(mode=_capi.INFL_SCORES, outs=(pred, info, unit, S, None, Ws, None)),
                    dict(off=np.array([1, 6, 13, 21], dtype=np.int64)), dict(off=np.array([0, 7, 6, 21], dtype=np.int64)),
                    dict(off=np.array([0, 6, 13, 22], dtype=np.int64)), dict(rows=dup), dict(rows=far)):
            assert status(**bad) == _capi.E_ARG, bad
        with pytest.raises(ValueError, match="mode"):
            ctx.influence_rows(M, beta, rows, off, mode=7)
        # ncfg = 0: zero matrices, nothing else is written
        Ws[:], Wv[:], info[:] = 1.0, 1.0, 5.0
        assert status(ncfg=0, off=np.zeros(1, dtype=np.int64), rows=None) == _capi.OK
        assert not Ws.any() and not Wv.any() and np.all(info == 5.0)
    finally:
        ctx.close()


def class_problem():
    sizes = [9 + (5 * c) % 37 for c in range(18)]
    return lc.config_rows(9, 12, sizes, testing_frac=0.15)


def fit_solver(name, extra, A, b, w, labels):
    test = np.asarray(labels["Testing"])
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
        return pt, s, {}
    s.perform_fit(A, b, w[~test], fs_dict=labels)
    return pt, s, dict(fs_dict=labels, b=b, w=w[~test])


def compare_results(dev, host, kinds):
    """The frames are equal (labels and integers exactly, the floating columns to 1e-10) and the covariances agree to 1e-10
    relative to their largest entry: both routes are float64 forms of the same closed forms on units of lambda_min >= 0.05,
    whose bars are at most 4 eps (2 K + J + d + n) / 0.05^2 = 1e-10 of the quantities' scale."""
    assert list(dev.units.columns) == list(host.units.columns) and len(dev.units) == len(host.units)
    exact = [c for c in dev.units.columns if c not in ("min_pivot", "cook", "shift", "score")]
    assert dev.units[exact].equals(host.units[exact])
    for col in ("min_pivot", "cook", "shift", "score"):
        np.testing.assert_allclose(dev.units[col].to_numpy(dtype=float), host.units[col].to_numpy(dtype=float), rtol=1e-10,
                                   atol=1e-10 * np.nanmax(np.abs(host.units[col].to_numpy(dtype=float))), equal_nan=True)
    assert sorted(dev.cov) == sorted(host.cov) == sorted(("classical",) + tuple(kinds))
    for k in dev.cov:
        assert np.max(np.abs(dev.cov[k] - host.cov[k])) <= 1e-10 * np.max(np.abs(host.cov[k])), k
    assert list(dev.stderr.columns) == list(host.stderr.columns)
    np.testing.assert_allclose(dev.stderr.to_numpy(dtype=float), host.stderr.to_numpy(dtype=float), rtol=1e-9)
    assert dev.noise == host.noise and dev.unidentifiable == host.unidentifiable


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra", [("ANL", {}), ("RIDGE", {"RIDGE": {"alpha": 1e-6}}), ("SVD", {})])
def test_solver_method_device_against_host(name, extra, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                                  # ANL saves covariance.npy / mean.npy into the cwd
    A, b, w, labels = class_problem()
    test = np.asarray(labels["Testing"])
    w[np.flatnonzero(~test)[5]] = 0.0
    pt, s, given = fit_solver(name, extra, A, b, w, labels)
    kinds = ("cr0", "cr1", "jack")
    dev = s.influence(kinds=kinds, method="device", want_dfbeta=True, **given)
    host = s.influence(kinds=kinds, method="host", want_dfbeta=True, **given)
    compare_results(dev, host, kinds)
    np.testing.assert_allclose(dev.dfbeta, host.dfbeta, rtol=1e-8, atol=1e-10 * np.max(np.abs(host.dfbeta)))
    assert dev.dfbeta.shape == (18, 12) and dev.unidentifiable == 0
    assert dev.units["rows_weighted"].sum() == int((~test).sum()) - 1 and dev.units["rows"].sum() == int((~test).sum())
    # dfbeta is the coefficient change of the refit without the unit
    u = 4
    cfg = np.asarray(labels["Configs"])
    wf = np.where(~test, w, 0.0)
    alpha = {"RIDGE": 1e-6, "ANL": float(s.config.sections["SOLVER"].cov_nugget)}.get(name, 0.0)
    Aw, bw = A * wf[:, None], b * wf
    full = np.linalg.solve(Aw.T @ Aw + alpha * np.eye(12), Aw.T @ bw)
    out_u = cfg == dev.units["Configs"][u]
    Ao, bo = Aw[~out_u], bw[~out_u]
    refit = np.linalg.solve(Ao.T @ Ao + alpha * np.eye(12), Ao.T @ bo)
    np.testing.assert_allclose(dev.dfbeta[u], refit - full, rtol=1e-6, atol=1e-9 * np.max(np.abs(full)))
    # the scores-only route: the same cr0 / cr1, no v
    few = s.influence(kinds=("cr1",), **given)
    assert sorted(few.cov) == ["classical", "cr1"] and few.dfbeta is None
    assert np.max(np.abs(few.cov["cr1"] - dev.cov["cr1"])) <= 1e-12 * np.max(np.abs(dev.cov["cr1"]))
    assert np.all(np.isnan(few.units["cook"])) and np.array_equal(few.units["score"], dev.units["score"])
    # a robust covariance under prediction_variance
    s.use_covariance(dev.cov["cr1"])
    pv = s.prediction_variance(a=A, method="fullcov", want_preds=False)
    want = np.einsum("ik,kl,il->i", A, dev.cov["cr1"], A)
    np.testing.assert_allclose(pv["var"], want, rtol=1e-11, atol=1e-13 * np.max(want))
    pt.free()


@pytest.mark.gpu
def test_an_ill_conditioned_svd_fit_takes_the_row_space_triangle(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(13)                             # one singular value of 1e-8: tests/test_gpu_loco.py's family
    m, K = 2000, 32
    Q, _ = np.linalg.qr(rng.standard_normal((m, K)))
    V, _ = np.linalg.qr(rng.standard_normal((K, K)))
    sv = np.ones(K)
    sv[-1] = 1e-8
    A = np.ascontiguousarray((Q * sv) @ V.T)
    b = A @ rng.standard_normal(K) + 1e-3 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    cfg = np.arange(m) // 50                                    # 40 units of 50 rows: J space
    labels = {"Configs": [f"cfg{c}" for c in cfg], "Groups": [f"g{c % 3}" for c in cfg], "Testing": [False] * m,
              "Row_Type": [("Energy", "Force", "Stress")[i % 3] for i in range(m)]}
    pt, s = make_solver("SVD")
    s.perform_fit(A, b, w, fs_dict=labels)
    assert s.last_row_space is not None
    given = dict(fs_dict=labels, b=b, w=w)
    dev = s.influence(kinds=("cr0", "jack"), method="device", **given)
    host = s.influence(kinds=("cr0", "jack"), method="host", **given)
    compare_results(dev, host, ("cr0", "jack"))
    assert dev.unidentifiable == 0 and np.all(np.isfinite(dev.cov["jack"]))
    pt.free()


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path, monkeypatch):
    world = 2
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="influence two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "influence_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    parts = [dict(np.load(tmp_path / f"influence_rank{r}.npz")) for r in range(world)]
    assert all(str(p["split"]) == "refused" for p in parts)          # a unit with rows on both ranks raises on every rank
    sizes = [12 + (7 * c) % 90 for c in range(40)]
    A, b, w, labels = lc.config_rows(5, 31, sizes, testing_frac=0.1)
    test = np.asarray(labels["Testing"])
    monkeypatch.chdir(tmp_path)
    pt, s = make_solver("RIDGE", {"RIDGE": {"alpha": 1e-6}})
    s.perform_fit(A, b, w[~test], fs_dict=labels)
    one = s.influence(kinds=("cr0", "cr1", "jack"), noise=0.01, fs_dict=labels, b=b, w=w[~test])
    # the ranks' statistics are summed in another order than one rank's, so M and beta differ in the last bits; the
    # covariances are sums of 40 outer products of vectors within 1e-13 of the one-rank ones: 1e-12 relative to the largest entry
    for k in ("classical", "cr0", "cr1", "jack"):
        assert np.max(np.abs(parts[0]["cov_" + k] - one.cov[k])) <= 1e-12 * np.max(np.abs(one.cov[k])), k
    np.testing.assert_allclose(parts[0]["stderr"], one.stderr.to_numpy(dtype=float), rtol=1e-12)
    assert parts[0]["stderr_columns"].tolist() == list(one.stderr.columns)
    # the pooled unit frame is the union of the two ranks' frames: every unit once, the same on both ranks
    names = parts[0]["unit_names"].tolist()
    assert sorted(names) == sorted(one.units["Configs"].tolist()) and names == parts[1]["unit_names"].tolist()
    cook = dict(zip(one.units["Configs"], one.units["cook"]))
    np.testing.assert_allclose(parts[0]["cook"], [cook[n] for n in names], rtol=1e-9)
    pt.free()


@pytest.mark.gpu
def test_cluster_robust_errors_exceed_the_classical_ones_on_clustered_noise(tmp_path, monkeypatch):
    """Seed influence_cases.CLUSTER_SEED, 10 000 x 17 in 400 units of 25 rows with a per-unit random effect:
    se_cr1 / se_classical > 1 on every coefficient and cov_jack >= cov_cr0 in the Loewner order (up to rounding)."""
    monkeypatch.chdir(tmp_path)
    A, b, w, labels = ic.clustered_problem()
    pt, s = make_solver("SVD")
    s.perform_fit(A, b, w, fs_dict=labels)
    res = s.influence(kinds=("cr0", "cr1", "jack"), fs_dict=labels, b=b, w=w)
    assert res.unidentifiable == 0 and len(res.units) == 400
    assert np.all(res.stderr["ratio_cr1"].to_numpy() > 1.0)
    gap = np.linalg.eigvalsh(res.cov["jack"] - res.cov["cr0"])
    assert gap[0] >= -1e-12 * np.max(np.abs(np.linalg.eigvalsh(res.cov["jack"])))
    pt.free()

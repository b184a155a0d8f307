"""GPU: exact leave-one-configuration-out predictions (fsnap_loco_rows, csrc/fsnap_loco.hip; Solver.loco_errors) against
brute-force refits, on synthetic configurations of 10 to 420 rows (both solve spaces, the LDS and the global-scratch
paths), the Ta golden rows (leave-one-group-out against lstsq), a column that one configuration alone touches,
determinism, residency, two ranks and 10^6 rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import loco, solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loco_cases import config_rows, downdated  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def make_solver(name, extra=None):
    pt = ParallelTools()
    d = {"SOLVER": {"solver": name}}
    d.update(extra or {})
    return pt, solver_factory.solver(name, pt, Config(pt, d))


def kernel(A, b, w, mask, M, beta, labels):
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w, None if mask is None else mask.astype(np.uint8))
    train = np.ones(len(b), dtype=bool) if mask is None else mask.astype(bool)
    rows, off, units = loco.unit_index(labels, train)
    pred, info = ctx.loco_rows(M, beta, rows, off)
    ctx.close()
    return pred, info, rows, off, units


SIZES = [10, 17, 33, 64, 100, 130, 200, 420, 150, 150, 150, 150, 150, 150]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 128, 142, 480])
@pytest.mark.parametrize("alpha", [0.0, 1e-8, 1e-4])
def test_kernel_matches_brute_force_refits(K, alpha):
    A, b, w, labels = config_rows(K, K, SIZES)
    Aw, bw = A * w[:, None], b * w
    G, c = Aw.T @ Aw, Aw.T @ bw
    beta = np.linalg.solve(G + alpha * np.eye(K), c)
    M = loco.factor_cholesky(G, alpha)
    pred, info, rows, off, _ = kernel(A, b, w, None, M, beta, labels["Configs"])
    assert np.all(info[:, 2] == 1.0)
    n = np.diff(off)
    assert np.array_equal(info[:, 0], np.minimum(n, K))
    assert np.array_equal(info[:, 3], (n <= K).astype(float))
    host, hinfo = loco.loco_host(A, b, w, M, beta, rows, off)
    bar = 1e-9 * np.max(np.abs(b))
    for u in range(len(off) - 1):
        r = rows[off[u]:off[u + 1]]
        ref = downdated(A, b, w, r, alpha, G, c)
        assert np.max(np.abs(pred[r] - ref)) <= bar, (u, len(r))
        assert np.max(np.abs(pred[r] - host[r])) <= bar
    np.testing.assert_allclose(info[:, 1], hinfo[:, 1], rtol=1e-8, atol=1e-12)


@pytest.mark.gpu
def test_zero_weight_and_testing_rows():
    A, b, w, labels = config_rows(3, 31, [20, 40, 25, 60, 35, 30, 45])
    w[::7] = 0.0
    mask = np.ones(len(b), dtype=bool)
    mask[3::11] = False
    w_eff = np.where(mask, w, 0.0)
    Aw, bw = A * w_eff[:, None], b * w_eff
    G = Aw.T @ Aw
    beta = np.linalg.solve(G + 1e-6 * np.eye(31), Aw.T @ bw)
    M = loco.factor_cholesky(G, 1e-6)
    pred, info, rows, off, _ = kernel(A, b, w, mask, M, beta, labels["Configs"])
    assert np.all(np.isnan(pred[~mask]))
    cfg = np.asarray(labels["Configs"])
    for u in dict.fromkeys(labels["Configs"]):
        r = np.flatnonzero((cfg == u) & mask)
        ref = downdated(A, b, w_eff, r, 1e-6)
        assert np.max(np.abs(pred[r] - ref)) <= 1e-9 * np.max(np.abs(b))


@pytest.mark.gpu
def test_leave_one_group_out_on_ta_rows_matches_lstsq_refits(ta, ta_fits):
    A, b, w = ta
    groups = ta_fits["ea_groups"]
    m = len(b)
    fs = {"Groups": groups.tolist(), "Testing": [False] * m, "Row_Type": ["Energy" if i % 5 == 0 else "Force" for i in range(m)],
          "Configs": [f"c{i // 7}" for i in range(m)]}
    pt, s = make_solver("SVD")
    s.perform_fit(A, b, w, fs_dict=fs)
    res = s.loco_errors(by="Groups", fs_dict=fs, b=b, w=w)
    assert res.unidentifiable == 0
    Aw, bw = A * w[:, None], b * w
    eps = np.finfo(float).eps
    for g in sorted(set(groups)):
        out = groups == g
        beta = np.linalg.lstsq(Aw[~out], bw[~out], rcond=1e-13)[0]
        ref = A[out] @ beta
        kappa = np.linalg.cond(Aw[~out])
        rel = np.max(np.abs(res.preds[out] - ref)) / np.max(np.abs(ref))
        assert rel <= max(1e-6, 50 * kappa * eps), (g, rel, kappa)
    # the *ALL training rows of the LOO table next to error_analysis's in-sample ones: same row layout
    s.error_analysis(A, b, w, fs_dict=fs)
    assert list(res.errors.index) == list(s.errors.index)
    pt.free()


@pytest.mark.gpu
def test_a_column_one_configuration_alone_touches():
    A, b, w, labels = config_rows(11, 31, [30, 25, 40, 35, 50, 45])
    cfg = np.asarray(labels["Configs"])
    A[:, 7] = 0.0
    A[cfg == "cfg2", 7] = 1.0 + 0.05 * np.arange(40)
    Aw, bw = A * w[:, None], b * w
    G = Aw.T @ Aw
    for alpha, ident in ((0.0, 0.0), (1e-4, 1.0)):
        beta = np.linalg.solve(G + alpha * np.eye(31), Aw.T @ bw)
        pred, info, rows, off, units = kernel(A, b, w, None, loco.factor_cholesky(G, alpha), beta, labels["Configs"])
        u = units.index("cfg2")
        assert info[u, 2] == ident
        assert np.all(np.delete(info[:, 2], u) == 1.0)
        if ident:
            assert np.all(np.isfinite(pred))
            r = rows[off[u]:off[u + 1]]
            assert np.max(np.abs(pred[r] - downdated(A, b, w, r, alpha))) <= 1e-8 * np.max(np.abs(b))
        else:
            assert np.all(np.isnan(pred[cfg == "cfg2"])) and np.all(np.isfinite(pred[cfg != "cfg2"]))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 142])
def test_bit_identical_repeats_and_permutation_of_configurations(K):
    sizes = [10, 33, 130, 64, 200, 17, 150, 150]
    A, b, w, labels = config_rows(2, K, sizes)
    Aw = A * w[:, None]
    G = Aw.T @ Aw
    beta = np.linalg.solve(G + 1e-6 * np.eye(K), Aw.T @ (b * w))
    M = loco.factor_cholesky(G, 1e-6)
    p1, i1, *_ = kernel(A, b, w, None, M, beta, labels["Configs"])
    p2, i2, *_ = kernel(A, b, w, None, M, beta, labels["Configs"])
    assert np.array_equal(p1, p2) and np.array_equal(i1, i2)
    # the configurations' row blocks in another order (rows within a configuration keep their order)
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    order = np.concatenate([np.flatnonzero(cfg == c) for c in np.random.default_rng(0).permutation(len(sizes))])
    p3, *_ = kernel(A[order], b[order], w[order], None, M, beta, [labels["Configs"][i] for i in order])
    assert np.array_equal(p3, p1[order])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["RIDGE", "SVD", "ANL"])
def test_resident_rows_stay_and_a_following_fit_is_unchanged(name):
    A, b, w, labels = config_rows(9, 31, [15 + (5 * c) % 60 for c in range(30)], testing_frac=0.1)
    pt, s = make_solver(name, {"RIDGE": {"alpha": 1e-6}} if name == "RIDGE" else None)
    if name == "ANL":
        pt.create_shared_array("a", *A.shape)
        pt.create_shared_array("b", len(b))
        pt.create_shared_array("w", len(b))
        pt.shared_arrays["a"].array[:] = A
        pt.shared_arrays["b"].array[:] = b
        pt.shared_arrays["w"].array[:] = w
        pt.fitsnap_dict = dict(labels)
        s.save_files = False
        s.perform_fit()
        fit1 = np.array(s.fit)
        res = s.loco_errors()
        s.perform_fit()
    else:
        test = np.asarray(labels["Testing"])
        s.keep_resident = True
        s.perform_fit(A, b, w[~test], fs_dict=labels)
        fit1 = np.array(s.fit)
        res = s.loco_errors(fs_dict=labels, b=b, w=w[~test])
        s.perform_fit(A, b, w[~test], fs_dict=labels)
    assert np.array_equal(np.asarray(s.fit), fit1)
    assert res.unidentifiable == 0
    assert np.all(np.isnan(res.preds[np.asarray(labels["Testing"])]))
    assert np.all(np.isfinite(res.preds[~np.asarray(labels["Testing"])]))
    assert len(res.units) == 30 and np.all(res.units["identifiable"])
    pt.free()


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path):
    world = 2
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="loco two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "loco_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    parts = [dict(np.load(tmp_path / f"loco_rank{r}.npz")) for r in range(world)]
    sizes = [12 + (7 * c) % 90 for c in range(40)]
    A, b, w, labels = config_rows(5, 31, sizes, testing_frac=0.1)
    test = np.asarray(labels["Testing"])
    # per row, bit for bit: the same M and beta on one context holding all rows
    M, beta = parts[0]["M"], parts[0]["beta"]
    assert np.array_equal(parts[1]["M"], M) and np.array_equal(parts[1]["beta"], beta)
    one, *_ = kernel(A, b, w, (~test), M, beta, labels["Configs"])
    for p in parts:
        assert np.array_equal(p["preds"], one[p["rows"]], equal_nan=True)
    # tables: one rank's own fit and LOCO
    pt, s = make_solver("RIDGE", {"RIDGE": {"alpha": 1e-6}})
    s.perform_fit(A, b, w[~test], fs_dict=labels)
    res = s.loco_errors(fs_dict=labels, b=b, w=w[~test])
    assert [str(x) for x in res.errors.index] == parts[0]["index"].tolist()
    np.testing.assert_allclose(parts[0]["errors"], res.errors.to_numpy(dtype=float), rtol=1e-12, atol=0)
    pt.free()


@pytest.mark.gpu
def test_million_rows_ten_thousand_configurations():
    rng = np.random.default_rng(0)
    K = 128
    sizes = rng.integers(32, 171, 10_000)
    m = int(sizes.sum())
    A = rng.standard_normal((m, K))
    b = A @ rng.standard_normal(K) + 0.05 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    Aw = A * w[:, None]
    G, c = Aw.T @ Aw, Aw.T @ (b * w)
    beta = np.linalg.solve(G, c)
    M = loco.factor_cholesky(G)
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pred, info = ctx.loco_rows(M, beta, np.arange(m, dtype=np.int32), off)
    ctx.close()
    assert np.all(info[:, 2] == 1.0) and np.all(np.isfinite(pred))
    for u in rng.choice(len(sizes), 12, replace=False):
        r = np.arange(off[u], off[u + 1])
        ref = downdated(A, b, w, r, 0.0, G, c)
        assert np.max(np.abs(pred[r] - ref)) <= 1e-9 * np.max(np.abs(b)), u
    assert m >= 10**6


@pytest.mark.gpu
def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "loco_validation.py")], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "*ALL" in r.stdout

"""GPU: predictive variance of rows (fsnap_row_variance, kernels of csrc/fsnap_uq.hip; Solver._compute_stdev and
Solver.prediction_variance) -- the kernel against a long-double numpy reference over K, J, m and lda, determinism under
repeats, subsets and permutations, the category sums, the reference's own _compute_stdev on the Ta rows, residency of
the training rows, 10^6 rows, two ranks and the active-learning example."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import solver_factory, uq

from conftest import ROOT

EPS = np.finfo(np.float64).eps
GOLDEN = os.path.join(ROOT, "tests", "golden")


def rows(m, K, seed, lda=None):
    rng = np.random.default_rng(seed)
    big = rng.standard_normal((m, lda or K))
    return big[:, :K]                       # lda > K: a strided view, uploaded with its own leading dimension


def psd(K, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((K + 3, K))
    return X.T @ X / (K + 3)


def ref_long(a, mode, M):
    al, Ml = a.astype(np.longdouble), M.astype(np.longdouble)
    T = al @ Ml
    v = (T * al).sum(axis=1) if mode == uq.QUAD else (T * T).sum(axis=1)
    aa, MM = np.abs(a), np.abs(M)
    if mode == uq.QUAD:
        bar = 4 * a.shape[1] * EPS * ((aa @ MM) * aa).sum(axis=1)
    else:
        bar = 4 * (a.shape[1] + M.shape[1]) * EPS * ((aa @ MM) ** 2).sum(axis=1)
    return v.astype(np.float64), bar


def ctx_with(a):
    ctx = _capi.HipContext(0)
    ctx.upload_rows(a, np.zeros(a.shape[0]))
    return ctx


def make_solver(name="ANL", extra=None):
    pt = ParallelTools()
    d = {"SOLVER": {"solver": name}}
    d.update(extra or {})
    return pt, solver_factory.solver(name, pt, Config(pt, d))


KS = [1, 4, 15, 16, 17, 31, 64, 128, 142, 144, 145, 256, 480, 1595]
MS = [1, 63, 64, 65, 1000, 15213]


# ---------------------------------------------------------------------------------------
# 1. kernel against long double
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_quad_and_preds_against_long_double(K):
    M = psd(K, K)
    beta = np.random.default_rng(K + 1).standard_normal(K)
    for i, m in enumerate(MS if K <= 256 else [1, 65, 1000]):
        lda = K + 3 if i % 2 else None
        a = rows(m, K, 100 * K + m, lda)
        ctx = ctx_with(a)
        out = ctx.row_variance(M, _capi.UQ_QUAD, beta=beta, want_preds=True)
        sel = np.arange(m) if K <= 256 else np.random.default_rng(m).choice(m, min(m, 64), replace=False)
        ref, bar = ref_long(np.ascontiguousarray(a[sel]), uq.QUAD, M)
        assert np.all(np.abs(out["var"][sel] - ref) <= bar), (K, m)
        # the predictive mean: a per-lane fma chain over k = ks, ks + 4, ... then two shuffles -- another summation order than
        # fsnap_predict's GEMV, so it is checked against predict_rows' values at the bar of either order
        pr, _ = ctx.predict(beta)
        pbar = 2 * K * EPS * np.linalg.norm(a, axis=1) * np.linalg.norm(beta)
        assert np.all(np.abs(out["preds"] - pr) <= pbar), (K, m)
        # var only / preds only give the same bits
        o2 = ctx.row_variance(M, _capi.UQ_QUAD, beta=beta, want_var=False, want_preds=True)
        o3 = ctx.row_variance(M, _capi.UQ_QUAD)
        assert np.array_equal(o2["preds"], out["preds"]) and np.array_equal(o3["var"], out["var"])
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 17, 31, 128, 145, 480])
@pytest.mark.parametrize("J", [1, 15, 16, 17, 133, 300])
def test_norm_against_long_double(K, J):
    M = np.random.default_rng(K * 1000 + J).standard_normal((K, J))
    m = 1000 if K <= 145 else 200
    a = rows(m, K, K + J, K + 5 if J % 2 else None)
    ctx = ctx_with(a)
    out = ctx.row_variance(M, _capi.UQ_NORM)
    ref, bar = ref_long(np.ascontiguousarray(a), uq.NORM, M)
    assert np.all(np.abs(out["var"] - ref) <= bar), (K, J)
    ctx.close()


@pytest.mark.gpu
def test_argument_errors_and_empty():
    a = rows(100, 16, 1)
    ctx = ctx_with(a)
    with pytest.raises(ValueError):
        ctx.row_variance(np.eye(17), _capi.UQ_QUAD)                 # K != resident width
    with pytest.raises(ValueError):
        ctx.row_variance(np.ones((16, 3)), _capi.UQ_QUAD)           # QUAD needs J = K
    cat = np.zeros(100, dtype=np.int32)
    cat[5] = 4
    with pytest.raises(ValueError):
        ctx.row_variance(np.eye(16), _capi.UQ_QUAD, cat=cat, ncat=4)  # id >= ncat
    ctx.close()
    ctx = _capi.HipContext(0)
    ctx.upload_rows(a, np.zeros(100))
    ctx.drop_rows()
    out = ctx.row_variance(np.eye(16), _capi.UQ_QUAD, cat=np.zeros(0, dtype=np.int32), ncat=3)
    assert out["var"].shape == (0,)
    assert np.array_equal(out["cat_count"], [0, 0, 0]) and np.all(out["cat_sum"] == 0) and np.all(out["cat_max"] == -np.inf)
    ctx.close()


# ---------------------------------------------------------------------------------------
# 2. determinism and the category sums
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 128, 1595])
def test_bit_identical_under_repeat_subset_and_permutation(K):
    m = 15213 if K != 1595 else 3000
    a = np.ascontiguousarray(rows(m, K, 7 * K))
    M = psd(K, 3)
    L = np.linalg.cholesky(M)
    beta = np.random.default_rng(2).standard_normal(K)
    ctx = ctx_with(a)
    base = {mode: ctx.row_variance(Mx, mode, beta=beta, want_preds=True) for mode, Mx in ((uq.QUAD, M), (uq.NORM, L))}
    for mode, Mx in ((uq.QUAD, M), (uq.NORM, L)):
        again = ctx.row_variance(Mx, mode, beta=beta, want_preds=True)
        assert np.array_equal(again["var"], base[mode]["var"]) and np.array_equal(again["preds"], base[mode]["preds"])
    rng = np.random.default_rng(5)
    perm = rng.permutation(m)
    sub = np.sort(rng.choice(m, m // 3, replace=False))
    for idx in (perm, sub, perm[: 1 + m // 7]):
        c2 = ctx_with(np.ascontiguousarray(a[idx]))
        for mode, Mx in ((uq.QUAD, M), (uq.NORM, L)):
            o = c2.row_variance(Mx, mode, beta=beta, want_preds=True)
            assert np.array_equal(o["var"], base[mode]["var"][idx]) and np.array_equal(o["preds"], base[mode]["preds"][idx])
        c2.close()
    ctx.close()


@pytest.mark.gpu
def test_category_sums_max_count():
    m, K, ncat = 15213, 31, 50
    a = np.ascontiguousarray(rows(m, K, 11))
    M = psd(K, 4)
    rng = np.random.default_rng(9)
    cat = rng.integers(-1, ncat - 3, m).astype(np.int32)        # scattered, some rows skipped, the last 3 categories empty
    cat[:3000] = 7                                               # one category over several chunks
    scale = rng.uniform(0.1, 3.0, m)
    ctx = ctx_with(a)
    o1 = ctx.row_variance(M, uq.QUAD, scale=scale, cat=cat, ncat=ncat)
    o2 = ctx.row_variance(M, uq.QUAD, scale=scale, cat=cat, ncat=ncat)
    for k in ("var", "cat_sum", "cat_max", "cat_count"):
        assert np.array_equal(o1[k], o2[k]), k
    sv = scale * o1["var"]
    for c in range(ncat):
        sel = cat == c
        assert o1["cat_count"][c] == sel.sum()
        if sel.any():
            ref = math.fsum(sv[sel])
            assert abs(o1["cat_sum"][c] - ref) <= 1e-15 * ref * max(1, np.log2(sel.sum())), c
            assert o1["cat_max"][c] == sv[sel].max()
        else:
            assert o1["cat_sum"][c] == 0.0 and o1["cat_max"][c] == -np.inf
    # no scale: the sums of var itself; a row permutation keeps counts and maxima exact
    o3 = ctx.row_variance(M, uq.QUAD, cat=cat, ncat=ncat)
    perm = rng.permutation(m)
    c2 = ctx_with(np.ascontiguousarray(a[perm]))
    o4 = c2.row_variance(M, uq.QUAD, cat=cat[perm], ncat=ncat)
    assert np.array_equal(o3["cat_count"], o4["cat_count"]) and np.array_equal(o3["cat_max"], o4["cat_max"])
    nz = o3["cat_count"] > 0
    assert np.all(np.abs(o3["cat_sum"] - o4["cat_sum"])[nz] <= 2e-15 * o3["cat_sum"][nz] * np.log2(o3["cat_count"][nz] + 1))
    c2.close()
    ctx.close()


@pytest.mark.gpu
def test_device_twin_matches_host_form():
    import torch

    m, K = 5000, 64
    a = np.ascontiguousarray(rows(m, K, 13))
    M = psd(K, 6)
    beta = np.random.default_rng(1).standard_normal(K)
    cat = (np.arange(m) % 17).astype(np.int32)
    scale = np.linspace(0.5, 2.0, m)
    ctx = ctx_with(a)
    host = ctx.row_variance(M, uq.QUAD, beta=beta, scale=scale, cat=cat, ncat=17, want_preds=True)
    dev = torch.device("cuda", 0)
    dv, dp = torch.empty(m, dtype=torch.float64, device=dev), torch.empty(m, dtype=torch.float64, device=dev)
    ds, dm = torch.empty(17, dtype=torch.float64, device=dev), torch.empty(17, dtype=torch.float64, device=dev)
    dc = torch.empty(17, dtype=torch.int64, device=dev)
    dscale = torch.from_numpy(scale).to(dev)
    torch.cuda.synchronize()
    ctx.row_variance_device(M, uq.QUAD, dv.data_ptr(), dp.data_ptr(), beta=beta, d_scale=dscale.data_ptr(), cat=cat, ncat=17,
                            d_cat_sum=ds.data_ptr(), d_cat_max=dm.data_ptr(), d_cat_count=dc.data_ptr())
    ctx.sync()
    assert np.array_equal(dv.cpu().numpy(), host["var"]) and np.array_equal(dp.cpu().numpy(), host["preds"])
    assert np.array_equal(ds.cpu().numpy(), host["cat_sum"]) and np.array_equal(dm.cpu().numpy(), host["cat_max"])
    assert np.array_equal(dc.cpu().numpy(), host["cat_count"])
    ctx.close()


# ---------------------------------------------------------------------------------------
# 3. the reference's own _compute_stdev on the Ta rows
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_compute_stdev_matches_reference_fixture(ta):
    A, b, w = ta
    g = np.load(os.path.join(GOLDEN, "ta_stdev_reference.npz"))
    pt, s = make_solver("ANL")
    s.cov, s.fit, s.fit_sam = g["cov"], g["fit"], g["fit_sam"]
    for meth in [str(x) for x in g["methods"]]:
        ref = g[f"stdev_{meth}"]
        got = s._compute_stdev(A, method=meth)
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(got)), meth
        bar = 1e-12 * np.abs(ref)
        if meth == "sam":
            # np.std(fit_sam @ a.T) subtracts the samples' mean AFTER the products; the ANL samples sit close to their
            # mean, so the reference value itself carries an absolute error of a few eps max_s |x_s . a| (up to 5e-12
            # relative on these rows).  Centring first (M = (X - mean)^T / sqrt(nsam)) does not.
            bar = bar + 8 * EPS * np.abs(g["fit_sam"] @ A.T).max(axis=0)
        assert np.all((np.abs(got - ref) <= bar)[fin]), meth
    assert np.array_equal(s._compute_stdev(A, method="nope"), np.zeros(len(b)))
    s.cov = None
    with pytest.raises(AssertionError):
        s._compute_stdev(A, method="chol")
    pt.free()


@pytest.mark.gpu
def test_stdev_after_bzeroflag_offset(ta):
    A, b, w = ta
    g = np.load(os.path.join(GOLDEN, "ta_stdev_reference.npz"))
    pt, s = make_solver("ANL", {"BISPECTRUM": {"numTypes": 1, "twojmax": 6, "bzeroflag": 1, "type": "Ta", "wj": 1.0,
                                              "radelem": 0.5},
                                 "CALCULATOR": {"calculator": "LAMMPSSNAP"}})
    bis = s.config.sections["BISPECTRUM"]
    assert bis.ncoeff == A.shape[1] - 1
    A = np.ascontiguousarray(A[:, 1:])            # a fit without the constant column, as bzeroflag gives it
    s.cov, s.fit, s.fit_sam = g["cov"][1:, 1:].copy(), g["fit"][1:].copy(), g["fit_sam"][:, 1:].copy()
    before = {m: s._compute_stdev(A, method=m) for m in ("sam", "fullcov")}
    pred0 = s.prediction_variance(A)["preds"]
    s._offset()
    assert s.fit.shape[0] == A.shape[1] + 1 and s.fit_sam.shape[1] == A.shape[1] + 1
    for m in ("sam", "fullcov"):
        assert np.array_equal(s._compute_stdev(A, method=m), before[m]), m
    assert np.array_equal(s.prediction_variance(A)["preds"], pred0)
    pt.free()


# ---------------------------------------------------------------------------------------
# 4. residency: an explicit pool does not evict the training rows, and is uploaded once
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pool_keeps_training_rows_resident(ta):
    A, b, w = ta
    train, pool = np.arange(0, 12000), np.arange(12000, len(b))
    pt, s = make_solver("ANL")
    s.save_files = False
    pt.create_shared_array("a", len(train), A.shape[1])
    pt.create_shared_array("b", len(train))
    pt.create_shared_array("w", len(train))
    pt.shared_arrays["a"].array[:] = A[train]
    pt.shared_arrays["b"].array[:] = b[train]
    pt.shared_arrays["w"].array[:] = w[train]
    pt.fitsnap_dict["Testing"] = [False] * len(train)
    s.keep_resident = True
    s.perform_fit()
    Ap = np.ascontiguousarray(A[pool])
    main = pt.hip()
    calls = {"main": 0, "pool": 0}
    real_main = main.upload_rows

    def count_main(*x, **k):
        calls["main"] += 1
        return real_main(*x, **k)

    main.upload_rows = count_main
    sd1 = s._compute_stdev(Ap, method="fullcov")
    real_pool = s._uq_ctx.upload_rows

    def count_pool(*x, **k):
        calls["pool"] += 1
        return real_pool(*x, **k)

    s._uq_ctx.upload_rows = count_pool
    res = s.prediction_variance(Ap, categories=[str(x) for x in np.asarray(pool) // 100])
    assert np.array_equal(np.sqrt(res["var"]), sd1) and calls["pool"] == 0
    ref = ((Ap @ s.cov) * Ap).sum(-1)
    assert np.allclose(res["var"], ref, rtol=1e-12, atol=0)
    assert np.allclose(res["preds"], Ap @ s.fit, rtol=1e-12, atol=1e-12 * np.abs(Ap @ s.fit).max())
    s.perform_fit()
    assert calls["main"] == 0
    # the shared rows themselves
    sd_train = s._compute_stdev(method="fullcov")
    assert np.allclose(sd_train ** 2, ((A[train] @ s.cov) * A[train]).sum(-1), rtol=1e-12)
    pt.free()


# ---------------------------------------------------------------------------------------
# 5. full size
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_million_rows_k128_and_wide():
    m, K = 1_000_000, 128
    a = np.random.default_rng(0).standard_normal((m, K))
    C = psd(K, 1)
    L = np.linalg.cholesky(C)
    ctx = ctx_with(a)
    sel = np.random.default_rng(1).choice(m, 10_000, replace=False)
    for mode, M in ((uq.QUAD, C), (uq.NORM, L)):
        out = ctx.row_variance(M, mode)
        ref, bar = ref_long(a[sel], mode, M)
        ref64 = uq.fold(a[sel], mode, M)
        assert np.all(np.abs(out["var"][sel] - ref) <= bar) and np.all(np.abs(out["var"][sel] - ref64) <= 2 * bar), mode
    ctx.close()
    del a
    m, K = 15213, 1595
    a = np.random.default_rng(2).standard_normal((m, K))
    C = psd(K, 2)
    ctx = ctx_with(a)
    out = ctx.row_variance(C, uq.QUAD)
    sel = np.random.default_rng(3).choice(m, 32, replace=False)
    ref, bar = ref_long(a[sel], uq.QUAD, C)
    assert np.all(np.abs(out["var"][sel] - ref) <= bar)
    ctx.close()


# ---------------------------------------------------------------------------------------
# 6. two ranks over the peer-to-peer transport, one GPU
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_ranks_match_one_process(tmp_path, ta):
    world = 2
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="uq two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "uq_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    parts = [dict(np.load(tmp_path / f"uq_rank{r}.npz")) for r in range(world)]
    A, b, w = ta
    g = np.load(os.path.join(GOLDEN, "ta_stdev_reference.npz"))
    pt, s = make_solver("ANL")
    s.cov, s.fit, s.fit_sam = g["cov"], g["fit"], g["fit_sam"]
    order = np.concatenate([p["rows"] for p in parts])
    for meth in ("sam", "chol", "fullcov"):
        one = s._compute_stdev(A, method=meth)
        assert np.array_equal(np.concatenate([p[f"stdev_{meth}"] for p in parts]), one[order]), meth
    res = s.prediction_variance(A)
    assert np.array_equal(np.concatenate([p["preds"] for p in parts]), res["preds"][order])
    pt.free()


# ---------------------------------------------------------------------------------------
# 7. the active-learning example
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_active_learning_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "active_learning_uncertainty.py"), "--iterations", "3",
                        "--check"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "first ranking matches numpy" in r.stdout
    assert r.stdout.count("*ALL") >= 3

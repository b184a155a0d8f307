"""GPU: grouped K-fold spectral paths (fsnap_spectral_path, kernels E1 / E2 of csrc/fsnap_spectral.hip; Solver.spectral_path)
against the host route (``spectral_path.spectral_path_host``: fsnap_spectral_gram per problem on the same statistics) and
against oracles A / B of tests/spectral_path_cases.py within the bars recorded there; the edges, determinism, side effects,
refusals, the solver surface, two ranks, the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import solver_factory
from fitsnap_amd.solvers import spectral_path as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectral_path_cases as cs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("eig", "z", "info", "sets", "fits", "coef", "heldout")


def on_device(blocks):
    """(tensor that owns the memory, device address) of hand-made blocks."""
    import torch

    t = torch.from_numpy(np.array(blocks, dtype=np.float64, order="C")).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr()


def path_of_blocks(blocks, K, F, nsub, alphas, rconds, ctx=None, want_coef=True):
    t, ptr = on_device(blocks)
    own = ctx is None
    ctx = _capi.HipContext(0) if own else ctx
    try:
        return ctx.spectral_path(ptr, K, F, nsub, alphas, rconds, want_coef)
    finally:
        if own:
            ctx.close()
        del t


def run_case(name, nsub, ctx=None):
    A, b, w, fold, cls, blocks, K, F, alphas, rconds = cs.case(name, nsub)
    dev = path_of_blocks(blocks, K, F, nsub, alphas, rconds, ctx)
    host = cs.host_route(name, nsub)
    fo = cs.figures(name, nsub, dev, where="kernel")                       # admits every problem first
    fh = cs.against_host(name, nsub, dev, host, where="kernel")
    print(f"{name} nsub = {nsub}: against the oracles {fo}; against the host route {fh}; sweeps {dev[2][:, 1].astype(int).tolist()}",
          flush=True)
    cs.check_bars(fo, cs.ORACLE_FACTOR, ("kernel - oracle", name, nsub), name)
    cs.check_bars(fh, cs.HOST_FACTOR, ("kernel - host", name, nsub), name)
    return dev, host


@pytest.mark.gpu
@pytest.mark.parametrize("K", cs.SWEEP_K + cs.LDS_EDGE_K)
def test_geometry_sweep(K):
    """Odd sizes need a bye in the pairing; 64 / 128 are wave edges; 113 is the largest size whose eigenvectors stay in LDS
    (155 KiB of dynamic LDS) and 114 the first that takes the scratch.  F = 3, nsub = 1 and 3, 3 alphas (0, 1e-8, 1e-2
    lambda_max) x 2 rconds (0, one that drops the planted tail): ranks, n_live and status equal, values within the bars --
    every case is well scaled (asserted), so the eigenvalues are also held RELATIVE to each eigenvalue, against long-double
    Jacobi and against the host route --, held-out sums against the rows in long double."""
    for nsub in (1, 3):
        run_case(K, nsub)


@pytest.mark.gpu
def test_edges():
    ctx = _capi.HipContext(0)
    try:
        # a column touched by one fold only: dead in that refit
        dev, _ = run_case("lone", 1, ctx)
        assert dev[2][1, 0] == 30 and not dev[5][1, :, 5].any() and dev[5][0, :, 5].all()
        # a fold without rows: its refit is the fit on all rows, bit for bit, and it holds nothing out
        dev, _ = run_case("empty", 1, ctx)
        assert np.array_equal(dev[5][3], dev[4]) and np.array_equal(dev[0][3], dev[0][4]) and not dev[6][3].any()
        # a rank-deficient total: rank K - 1 at rcond = 1e-6 and at the floor
        dev, _ = run_case("dup", 1, ctx)
        assert np.all(dev[3][:, :, 0] == 30)
        A, b, w, fold, cls, blocks, K, F, alphas, rconds = cs.case(31)
        # no live column: one fold holds every row
        one = blocks.sum(axis=0, keepdims=True)
        dev = path_of_blocks(one, K, 1, 1, alphas, rconds, ctx)
        host = sp.spectral_path_host(one, K, alphas, rconds)
        assert dev[2][0, 0] == 0 and dev[2][0, 1] == 0 and not dev[0][0].any() and not dev[5][0].any() and not dev[3][0, :, :2].any()
        assert np.all(dev[6][0, :, 0, 1] == dev[6][0, :, 0, 2]) and np.all(dev[3][0, :, 2] == 0.0)
        cs.check_bars(cs.against_host_blocks(one, K, 1, alphas, rconds, dev, host), cs.HOST_FACTOR, "one fold")
        # rcond above 1: nothing is kept, beta = 0, held-out = bb
        blocks3, alphas, rconds = (cs.case(31, 3)[i] for i in (5, 8, 9))        # the same rows as 9 blocks: fold x row class
        assert blocks3.shape[0] == 3 * F
        dev = path_of_blocks(blocks3, K, F, 3, alphas[:1], [1.5], ctx)
        assert not dev[3][:, :, :2].any() and not dev[4].any() and not dev[5].any()
        assert np.array_equal(dev[6][..., 1], dev[6][..., 2]) and dev[6][..., 2].all()
        # Qa = Qr = 1, and coef_out NULL: the other outputs are the same bits
        full = path_of_blocks(blocks3, K, F, 3, alphas, rconds, ctx)
        single = path_of_blocks(blocks3, K, F, 3, alphas[1:2], rconds[1:], ctx)
        q = 1 * len(rconds) + 1
        assert np.array_equal(single[4][0], full[4][q]) and np.array_equal(single[5][:, 0], full[5][:, q])
        assert np.array_equal(single[6][:, 0], full[6][:, q]) and np.array_equal(single[3][:, 0], full[3][:, q])
        bare = path_of_blocks(blocks3, K, F, 3, alphas, rconds, ctx, want_coef=False)
        assert bare[5] is None and all(np.array_equal(bare[i], full[i]) for i in (0, 1, 2, 3, 4, 6))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_more_problems_than_compute_units():
    """K = 8, every one of 300 units its own fold: 301 problems stride over the workgroups."""
    K, F = 8, 300
    A, b, w, fold, cls = cs.planted_rows(8300, K, [12] * F)
    blocks = cs.blocks_numpy(A, b, w, fold, F)
    lmax = float(np.linalg.eigvalsh(blocks[:, :K * K].sum(axis=0).reshape(K, K))[-1])
    alphas, rconds = [0.0, 1e-6 * lmax], [0.0, 1e-3]
    dev = path_of_blocks(blocks, K, F, 1, alphas, rconds)
    host = sp.spectral_path_host(blocks, K, alphas, rconds)
    worst = cs.against_host_blocks(blocks, K, 1, alphas, rconds, dev, host, "300 folds")
    print(f"300 folds: against the host route {worst}", flush=True)
    cs.check_bars(worst, cs.HOST_FACTOR, "300 folds")
    assert np.all(dev[2][:, 0] == K) and np.all(dev[2][:, 5] == 0)


@pytest.mark.gpu
def test_bit_identical_runs_permuted_grids_and_folds():
    """Integer rows with unit weights: every sum of blocks is exact, so the total is the same bits whatever the order of the
    folds, and a problem's result must then be the same bits wherever it stands in the call."""
    K, F = 70, 5
    rng = np.random.default_rng(43)
    m = 1200
    A = rng.integers(-3, 4, (m, K)).astype(np.float64)
    b = (A[:, :9] @ rng.integers(-2, 3, 9) + rng.integers(-1, 2, m)).astype(np.float64)
    fold = rng.integers(0, F, m)
    cls = np.arange(m) % 2
    nsub = 2
    blocks = cs.blocks_numpy(A, b, np.ones(m), fold * nsub + cls, F * nsub)
    alphas, rconds = np.array([0.0, 3.0, 50.0]), np.array([0.0, 0.2])
    ctx = _capi.HipContext(0)
    try:
        first = path_of_blocks(blocks, K, F, nsub, alphas, rconds, ctx)
        second = path_of_blocks(blocks, K, F, nsub, alphas, rconds, ctx)
        assert all(np.array_equal(x, y) for x, y in zip(first, second))
        Qr = len(rconds)
        # the grid permuted and cut
        ap, rp = np.array([2, 0, 1]), np.array([1, 0])
        perm = path_of_blocks(blocks, K, F, nsub, alphas[ap], rconds[rp], ctx)
        qperm = (ap[:, None] * Qr + rp[None, :]).reshape(-1)
        sub = path_of_blocks(blocks, K, F, nsub, alphas[[0, 2]], rconds[[1]], ctx)
        qsub = np.array([0 * Qr + 1, 2 * Qr + 1])
        for i, name in enumerate(NAMES):
            if name in ("eig", "z", "info"):
                assert np.array_equal(first[i], perm[i]) and np.array_equal(first[i], sub[i]), name
                continue
            ax = 0 if name == "fits" else 1
            assert np.array_equal(np.take(first[i], qperm, axis=ax), perm[i]), name
            assert np.array_equal(np.take(first[i], qsub, axis=ax), sub[i]), name
        # the folds permuted and cut
        fperm = np.array([4, 2, 0, 3, 1])
        order = (fperm[:, None] * nsub + np.arange(nsub)[None, :]).reshape(-1)
        fp = path_of_blocks(blocks[order], K, F, nsub, alphas, rconds, ctx)
        for i, name in enumerate(NAMES):
            if name == "fits":
                assert np.array_equal(first[i], fp[i])
            elif name in ("coef", "heldout"):
                assert np.array_equal(first[i][fperm], fp[i]), name
            else:
                assert np.array_equal(first[i][np.r_[fperm, F]], fp[i]), name
    finally:
        ctx.close()


@pytest.mark.gpu
def test_entry_point_argument_checks():
    A, b, w, fold, cls, blocks, K, F, alphas, rconds = cs.case(3)
    t, ptr = on_device(blocks)
    ctx = _capi.HipContext(0)
    try:
        ctx.spectral_path(ptr, K, F, 1, alphas, rconds)
        t0 = ctx.spectral_path_times()
        lib = ctx._lib
        do = np.zeros(4096)
        good_a, good_r = np.array([0.0, 1.0]), np.array([0.0, 1e-3])

        def status(K=K, F=F, nsub=1, ptr=ptr, a=good_a, Qa=None, r=good_r, Qr=None, outs=(do,) * 7):
            """The status of the raw entry point: nothing in front of it can refuse first."""
            a = None if a is None else np.ascontiguousarray(a, dtype=np.float64)
            r = None if r is None else np.ascontiguousarray(r, dtype=np.float64)
            return lib.fsnap_spectral_path(ctx._h, K, F, nsub, _capi.c_void_p(ptr), _capi._ptr(a), len(good_a) if Qa is None else Qa,
                                           _capi._ptr(r), len(good_r) if Qr is None else Qr, *(_capi._ptr(x) for x in outs))

        assert status() == _capi.OK
        coefless = [do] * 7
        coefless[5] = None
        assert status(outs=tuple(coefless)) == _capi.OK                       # coef_out may be NULL
        big = (2 << 30) // (8 * (K * K + K + 3))                               # F * nsub blocks past FSNAP_CAT_STATS_MAX_BYTES
        bads = [dict(K=0), dict(K=145), dict(F=0), dict(nsub=0), dict(Qa=0), dict(Qr=0), dict(ptr=None), dict(a=None), dict(r=None),
                dict(a=[0.0, -1.0]), dict(a=[np.nan, 0.0]), dict(a=[np.inf, 0.0]), dict(r=[0.0, -1e-3]), dict(r=[np.nan, 0.0]),
                dict(nsub=big)]
        for i in (0, 1, 2, 3, 4, 6):
            outs = [do] * 7
            outs[i] = None
            bads.append(dict(outs=tuple(outs)))
        ctx.spectral_path(ptr, K, F, 1, alphas, rconds)
        t1 = ctx.spectral_path_times()
        # nothing is launched by a refused call: the outputs keep their bits, and the times of the last successful call stay
        # readable and unchanged (the entry point forgets them as soon as it has queued its first kernel)
        mark = np.full(4096, -7.25)
        for bad in bads:
            outs = tuple(None if x is None else mark for x in bad.get("outs", (do,) * 7))
            assert status(**{**bad, "outs": outs}) == _capi.E_ARG, bad
            assert np.all(mark == -7.25), bad
            assert ctx.spectral_path_times() == t1, bad
        # the binding turns the status into ValueError
        for change in ({"K": 145}, {"alphas": [-1.0]}, {"rconds": [np.nan]}, {"alphas": []}):
            kw = {**dict(d_stats_ptr=ptr, K=K, F=F, nsub=1, alphas=alphas, rconds=rconds), **change}
            with pytest.raises(ValueError):
                ctx.spectral_path(**kw)
        assert len(t0) == 2 and all(x >= 0.0 for x in t0)
    finally:
        ctx.close()
        del t


def fitted(kind, A, b, w, labels, section=None):
    """A RIDGE or SVD solver fitted on shared arrays that hold (A, b, w) with the labels in pt.fitsnap_dict."""
    pt = ParallelTools()
    d = {"SOLVER": {"solver": kind}}
    if section:
        d[kind] = dict(section)
    s = solver_factory.solver(kind, pt, Config(pt, d))
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


@pytest.mark.gpu
def test_ridge_on_the_ta_rows_and_side_effects(ta):
    """RIDGE.spectral_path at (its alpha, 0) is the ridge fit of the downloaded statistics within the bar; a perform_fit after
    the call returns the bits it returned before it; the two tables agree; host and device give equal picks."""
    A, b, w = ta
    m, K = A.shape
    conf = np.arange(m) // 50
    testing = np.zeros(m, dtype=bool)
    testing[1::4] = True
    pt, s = fitted("RIDGE", A, b, w, labels_of(conf, np.arange(m) % 3, testing), {"alpha": 1e-8})
    fit0 = s.fit.copy()
    alpha = 1e-8
    res = s.spectral_path(folds=5, seed=2, method="device", table="rows")
    assert res.alphas.tolist() == [alpha] and res.rconds.tolist() == [0.0] and res.fits.shape == (1, K)
    G, c, _ = s.last_statistics
    ref = _capi.solve(_capi.SOLVE_RIDGE, alpha, G, c)[0]
    lam = np.linalg.eigvalsh(G)
    bar = cs.ORACLE_FACTOR * cs.MEASURED_COEF * K * cs.EPS * lam[-1] / (max(lam[0], 0.0) + alpha)
    err = cs.scaled_err(G, res.fits[0], ref.astype(cs.LD))
    print(f"Ta: spectral fit against fsnap_solve {err:.2e} (bar {bar:.2e}); sweeps {res.sweeps.tolist()}", flush=True)
    assert err <= bar and np.all(res.status == 0) and np.all(res.rank == K)
    # a wider grid: both tables, both routes
    alphas, rconds = [0.0, 1e-8, 1e-4], [0.0, 1e-7]
    rows = s.spectral_path(alphas, rconds, folds=5, seed=2, method="device", table="rows")
    stats = s.spectral_path(alphas, rconds, folds=5, seed=2, method="device", table="stats")
    host = s.spectral_path(alphas, rconds, folds=5, seed=2, method="host", table="stats")
    assert np.array_equal(rows.fits, stats.fits) and list(rows.table.index.names) == ["alpha", "rcond", "Row_Type"]
    for a, r in rows.grid:
        assert rows.table.loc[(a, r, "*ALL"), "ncount"] == stats.table.loc[(a, r, "*ALL"), "ncount"]
        np.testing.assert_allclose(rows.table.loc[(a, r, "*ALL"), "w_rmse"], stats.table.loc[(a, r, "*ALL"), "w_rmse"], rtol=1e-9)
        for name in ("Energy", "Force", "Stress"):
            assert rows.table.loc[(a, r, name), "ncount"] == stats.table.loc[(a, r, name), "ncount"]
    assert (host.best, host.simplest) == (stats.best, stats.simplest) and np.array_equal(host.rank, stats.rank)
    assert stats.best_alpha == stats.grid[stats.best][0] and stats.simplest_rcond == stats.grid[stats.simplest][1]
    assert stats.dof[5, stats.simplest] <= stats.dof[5, stats.best]
    np.testing.assert_allclose(stats.gcv, (~testing).sum() * stats.train_sse[5] / ((~testing).sum() - stats.dof[5]) ** 2, rtol=1e-12)
    s.perform_fit()
    assert np.array_equal(s.fit, fit0)
    pt.free()


@pytest.mark.gpu
def test_fits_on_a_well_conditioned_set_match_the_oracle():
    from oracle import fitsnap_oracle as orc
    import bcs_cases

    A, b, w, conf, cls = bcs_cases.rows(916, 33, per=50)                       # 2 000 x 33
    A, b, w = np.array(A), np.array(b), np.array(w)
    K = A.shape[1]
    testing = np.arange(len(b)) % 13 == 0
    G = orc.normal_eq(A, b, w, testing)[0]
    assert np.linalg.cond(G) * K * cs.EPS < 1e-7
    labels = labels_of(conf, cls, testing)
    for kind, ref in (("RIDGE", orc.ridge_fit(A, b, w, 1e-8, testing=testing)),
                      ("SVD", orc.svd_fit(A, b, w, testing=testing))):
        pt, s = fitted(kind, A, b, w, labels)
        dev = s.spectral_path(folds=4, method="device", table="stats")
        host = s.spectral_path(folds=4, method="host", table="stats")
        assert dev.fits.shape == (1, K) and (dev.best, dev.simplest) == (host.best, host.simplest) == (0, 0)
        assert np.max(np.abs(dev.fits[0] - ref) / np.abs(ref)) < 1e-6, kind
        assert np.max(np.abs(dev.fits[0] - s.fit) / np.abs(s.fit)) < 1e-6, kind
        assert dev.rconds.tolist() == ([0.0] if kind == "RIDGE" else [1e-13]) and np.all(dev.rank == K)
        pt.free()
    pt, s = fitted("RIDGE", A, b, w, labels)
    with pytest.raises(ValueError, match="method must be"):
        s.spectral_path(method="gpu")
    with pytest.raises(ValueError, match="finite"):
        s.spectral_path(alphas=[-1.0])
    pt.free()
    pt = ParallelTools()
    lasso = solver_factory.solver("LASSO", pt, Config(pt, {"SOLVER": {"solver": "LASSO"}}))
    with pytest.raises(ValueError, match="has no spectral path"):
        lasso.spectral_path()
    ridge = solver_factory.solver("RIDGE", pt, Config(pt, {"SOLVER": {"solver": "RIDGE"}}))
    with pytest.raises(RuntimeError, match="perform_fit first"):
        ridge.spectral_path()
    tr = solver_factory.solver("RIDGE", pt, Config(pt, {"SOLVER": {"solver": "RIDGE"}, "EXTRAS": {"apply_transpose": 1}}))
    with pytest.raises(ValueError, match="apply_transpose"):
        tr.spectral_path()
    pt.free()


@pytest.mark.gpu
def test_two_ranks_on_one_gpu(tmp_path):
    """Two ranks (peer-to-peer transport, rows dealt round-robin so that every unit spans both): the same bits on both ranks and
    the one-process result (equal ranks and picks; numbers to the rounding of statistics summed in another order)."""
    import spectral_path_dist_worker as wk

    procs = []
    for rank in range(2):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE="2",
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="spectral path ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "spectral_path_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    two = [dict(np.load(tmp_path / f"spectral_rank{r}.npz")) for r in range(2)]
    for key in two[0]:
        assert np.array_equal(two[0][key], two[1][key], equal_nan=two[0][key].dtype.kind == "f"), key
    A, b, w, labels = wk.rows()
    pt, s = fitted("RIDGE", A, b, w, labels)
    one = wk.path_of(s)
    pt.free()
    got = two[0]
    assert np.array_equal(got["rank"], one.rank) and np.array_equal(got["status"], one.status)
    assert got["folds"].tolist() == [f"{k}={v}" for k, v in sorted(one.fold_of_unit.items())]
    assert got["index"].tolist() == [str(x) for x in one.table.index]
    assert got["best"] == one.best and got["simplest"] == one.simplest
    np.testing.assert_allclose(got["fits"], one.fits, rtol=0, atol=1e-9 * np.max(np.abs(one.fits)))
    np.testing.assert_allclose(got["eigenvalues"], one.eigenvalues, rtol=1e-9)
    np.testing.assert_allclose(got["cv_error"], one.cv_error, rtol=1e-8)
    np.testing.assert_allclose(got["table"], one.table.to_numpy(dtype=float), rtol=1e-7)


@pytest.mark.gpu
def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "spectral_path.py")], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "best" in r.stdout and "simplest" in r.stdout

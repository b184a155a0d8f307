"""GPU: the MERR log-posterior pass (fsnap_merr_eval, kernels M1-M3) against a numpy evaluation in extended precision,
its determinism, and the MERR solver class against the reference's own MERR runs (tests/golden/ta_merr_reference.npz,
made by tests/golden/make_golden_merr.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import solver_factory
from fitsnap_amd.solvers.merr import merr_gradient, merr_q

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def np_merr(A, b, w, mask, c, q, d, method):
    """(val, g, h) of fsnap_merr_eval, accumulated in long double."""
    L = np.longdouble
    keep = mask.astype(bool)
    x = w[keep, None].astype(L) * A[keep].astype(L)
    e = x @ c.astype(L) - w[keep].astype(L) * b[keep].astype(L)
    v = (x * x) @ q.astype(L) + L(d)
    if method == "abc":
        sv = np.sqrt(v)
        r = np.abs(e) - sv
        val = np.sum(-0.5 * r * r / L(0.01))
        al = -r / L(0.01) * np.sign(e)
        be = r / (L(0.02) * sv)
    else:
        val = np.sum(-0.5 * e * e / v - 0.5 * np.log(v))
        al = -e / v
        be = 0.5 * e * e / (v * v) - 0.5 / v
    return float(val), (x.T @ al).astype(np.float64), ((x * x).T @ be).astype(np.float64)


def _problem(m, K, seed, lda=None, nan_test_rows=False, zero_w=False, zero_cols=()):
    r = np.random.default_rng(seed)
    A = r.standard_normal((m, K)) * (1.0 + r.random(K))
    for j in zero_cols:
        A[:, j] = 0.0
    beta = r.standard_normal(K)
    b = A @ beta + 0.3 * r.standard_normal(m)
    w = 0.5 + r.random(m)
    mask = (r.random(m) < 0.85).astype(np.uint8)
    if m == 1:
        mask[0] = 1
    if zero_w:
        w[r.random(m) < 0.2] = 0.0
    if nan_test_rows:
        t = np.flatnonzero(mask == 0)
        A[t[: len(t) // 2], 0] = np.nan
        b[t[len(t) // 2:]] = np.inf
        w[t[::3]] = np.nan
    return A, b, w, mask, beta


def _ctx_for(A, b, w, mask, lda=None):
    ctx = _capi.HipContext(0)
    m, K = A.shape
    if lda is None:
        ctx.upload_rows(A, b)
        keep = None
    else:
        import torch
        dev = torch.zeros((m + 1) * lda, dtype=torch.float64, device="cuda:0")     # one row of padding past the end
        dev[: m * lda].view(m, lda)[:, :K] = torch.from_numpy(A).to("cuda:0")
        db = torch.from_numpy(b.copy()).to("cuda:0")
        ctx.bind_rows(dev.data_ptr(), m, K, lda, db.data_ptr())
        keep = (dev, db)
    ctx.set_weights(w, mask.astype(bool))
    return ctx, keep


def _params(K, seed, frac_emb=1.0):
    r = np.random.default_rng(seed)
    c = r.standard_normal(K)
    q = (0.05 + r.random(K)) ** 2
    q[r.random(K) > frac_emb] = 0.0
    return c, q


CASES = [  # (m, K, extras)
    (1, 1, {}), (7, 1, {}), (4097, 1, {}),
    (7, 31, {}), (4097, 31, {"nan_test_rows": True}), (100_000, 31, {"zero_w": True}),
    (4097, 128, {"zero_cols": (0, 77)}), (100_000, 128, {}),
    (7, 142, {}), (4097, 142, {"lda": 151}),
    (4097, 200, {"zero_w": True, "nan_test_rows": True}),
    (1, 288, {}), (4097, 288, {"lda": 293}),
    (7, 320, {}), (4097, 320, {"nan_test_rows": True, "zero_cols": (5,)}),
    (1, 600, {}), (4097, 600, {"lda": 601, "zero_w": True}),
]


@pytest.mark.parametrize("method", ["iid", "abc", "full"])
@pytest.mark.parametrize("m,K,extra", CASES, ids=[f"{m}x{K}" + "".join(f"-{k}" for k in e) for m, K, e in CASES])
def test_merr_eval_matches_extended_precision(m, K, extra, method):
    extra = dict(extra)
    lda = extra.pop("lda", None)
    A, b, w, mask, _ = _problem(m, K, 11 + m + K, **extra)
    ctx, keep = _ctx_for(A, b, w, mask, lda)
    try:
        for seed, frac in ((1, 1.0), (2, 0.4)):
            c, q = _params(K, seed, frac)
            d = 0.37
            val, g, h = ctx.merr_eval(method, c, q, d)
            rv, rg, rh = np_merr(A, b, w, mask, c, q, d, "abc" if method == "abc" else "iid")
            assert abs(val - rv) <= 1e-12 * max(abs(rv), 1e-300), (val, rv)
            assert np.max(np.abs(g - rg)) <= 1e-11 * max(np.max(np.abs(rg)), 1e-300)
            assert np.max(np.abs(h - rh)) <= 1e-11 * max(np.max(np.abs(rh)), 1e-300)
            for j in extra.get("zero_cols", ()):
                assert g[j] == 0.0 and h[j] == 0.0
    finally:
        ctx.close()


@pytest.mark.parametrize("mult", [0, 1])
def test_merr_gradient_composition_on_device(mult):
    # composed gradient of the device sums against central differences of the extended-precision value
    A, b, w, mask, beta = _problem(3000, 31, 5)
    ctx, _ = _ctx_for(A, b, w, mask)
    emb = np.array([0, 3, 4, 10, 30])
    r = np.random.default_rng(3)
    cf, sig = beta + 0.1 * r.standard_normal(31), 0.1 + r.random(len(emb))
    try:
        for method in ("iid", "abc"):
            val, g, h = ctx.merr_eval(method, cf, merr_q(cf, sig, emb, mult), 0.2)
            gc, gs = merr_gradient(cf, sig, emb, mult, g, h)
            x = np.concatenate([cf, sig])

            def L(x):
                return np_merr(A, b, w, mask, x[:31], merr_q(x[:31], x[31:], emb, mult), 0.2, method)[0]

            grad = np.concatenate([gc, gs])
            for k in (0, 3, 17, 31, 33, 35):
                hk = 1e-6 * max(1.0, abs(x[k]))
                xp, xm = x.copy(), x.copy()
                xp[k] += hk
                xm[k] -= hk
                fd = (L(xp) - L(xm)) / (2 * hk)
                assert abs(fd - grad[k]) <= 1e-5 * max(1.0, np.max(np.abs(grad))), (k, fd, grad[k])
    finally:
        ctx.close()


@pytest.mark.parametrize("K", [128, 600])
def test_merr_eval_is_deterministic(K):
    A, b, w, mask, _ = _problem(50_000, K, 9)
    ctx, _ = _ctx_for(A, b, w, mask)
    try:
        c, q = _params(K, 4)
        v1, g1, h1 = ctx.merr_eval("abc", c, q, 0.5)
        v2, g2, h2 = ctx.merr_eval("abc", c, q, 0.5)
        assert v1 == v2 and np.array_equal(g1, g2) and np.array_equal(h1, h2)
    finally:
        ctx.close()


def test_merr_eval_errors():
    ctx = _capi.HipContext(0)
    try:
        with pytest.raises(Exception):
            ctx.merr_eval("iid", np.zeros(3), np.zeros(3), 1.0)          # no rows bound
        A, b, w, mask, _ = _problem(100, 3, 1)
        ctx.upload_rows(A, b)
        ctx.set_weights(w, mask.astype(bool))
        with pytest.raises(ValueError):
            ctx.merr_eval("iid", np.zeros(4), np.zeros(4), 1.0)          # K mismatch (binding)
        with pytest.raises(ValueError):
            ctx.merr_eval("gauss", np.zeros(3), np.zeros(3), 1.0)        # unknown method (binding)
        lib = ctx._lib
        c = np.zeros(4)
        val = _capi.c_double(0.0)
        assert lib.fsnap_merr_eval(ctx._h, 0, 4, _capi._ptr(c), _capi._ptr(c), 1.0, _capi.byref(val), _capi._ptr(c),
                                   _capi._ptr(c)) == _capi.E_ARG        # K mismatch (C ABI)
        c = np.zeros(3)
        assert lib.fsnap_merr_eval(ctx._h, 7, 3, _capi._ptr(c), _capi._ptr(c), 1.0, _capi.byref(val), _capi._ptr(c),
                                   _capi._ptr(c)) == _capi.E_ARG        # unknown method (C ABI)
    finally:
        ctx.close()


# ---- the solver class against the reference's MERR --------------------------------------------------------------

@pytest.fixture(scope="module")
def merr_ref():
    return dict(np.load(os.path.join(GOLDEN, "ta_merr_reference.npz")))


def _ta_subset(ref):
    z = np.load(os.path.join(GOLDEN, "ta_abw.npz"))
    s = int(ref["row_stride"])
    return (np.ascontiguousarray(z["A"][::s]), np.ascontiguousarray(z["b"][::s]), np.ascontiguousarray(z["w"][::s]))


def _merr_solver(method, mult, cfs, extra=None):
    pt = ParallelTools()
    cfg = Config(pt, dict({"SOLVER": {"solver": "MERR", "merr_method": method, "merr_mult": mult, "merr_cfs": cfs}},
                          **(extra or {})))
    return pt, solver_factory.solver("MERR", pt, cfg)


TAGS = ["iid_add", "iid_mult", "abc_add", "abc_mult", "abc_add_cfs"]


@pytest.mark.parametrize("tag", TAGS)
def test_merr_class_reaches_the_reference_logpost(tag, merr_ref, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    A, b, w = _ta_subset(merr_ref)
    method, mult, cfs = str(merr_ref[f"{tag}_method"]), int(merr_ref[f"{tag}_mult"]), str(merr_ref[f"{tag}_cfs"])
    pt, s = _merr_solver(method, mult, cfs)
    np.random.seed(int(merr_ref["seed"]))
    s.perform_fit(A, b, w, trainall=True)
    # the data variance is the reference's (same posterior-noise estimate)
    assert abs(s.datavar - merr_ref[f"{tag}_datavar"]) <= 1e-9 * abs(merr_ref[f"{tag}_datavar"])
    # device log-posterior at the reference's own final vector
    Lref = float(merr_ref[f"{tag}_logpost"])
    f, _ = s.objective(merr_ref[f"{tag}_x"])
    assert abs(-f - Lref) <= 1e-12 * abs(Lref) + 1e-300, (-f, Lref)
    # the class ends at an equal or higher log-posterior
    assert s.logpost >= Lref - 1e-6 * abs(Lref), (s.logpost, Lref)
    K = A.shape[1]
    assert s.fit.shape == (K,) and s.cov.shape == (K, K)
    assert np.all(np.isfinite(s.fit)) and np.all(np.isfinite(s.cov))
    assert np.count_nonzero(s.cov - np.diag(np.diag(s.cov))) == 0
    emb = np.arange(K) if cfs == "all" else np.array([int(i) for i in cfs.split()])
    off = np.setdiff1d(np.arange(K), emb)
    assert np.all(np.diag(s.cov)[off] == 0.0)
    assert np.array_equal(np.load(tmp_path / "mean.npy"), s.fit)
    assert np.array_equal(np.load(tmp_path / "covariance.npy"), s.cov)
    pt.free()


def test_merr_class_backfills_zero_columns(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    A, b, w, _, _ = _problem(5000, 12, 21, zero_cols=(2, 7))
    pt, s = _merr_solver("iid", 1, "0 4 9")
    np.random.seed(1)
    s.perform_fit(A, b, w, trainall=True)
    assert s.fit[2] == 0.0 and s.fit[7] == 0.0
    # reduced columns 0 / 4 / 9 are full columns 0 / 5 / 11
    d = np.diag(s.cov)
    assert np.all(d[[1, 2, 3, 4, 6, 7, 8, 9, 10]] == 0.0) and d[0] > 0.0 and d[5] > 0.0 and d[11] > 0.0
    assert s.logpost >= -s.objective(s.params_ini)[0]
    pt.free()


def _np_logpost(x, aw, bw, ind, datavar, mult, method):
    """The reference's logpost_emb restated in numpy (diagonal 'full' is 'iid')."""
    nbas = aw.shape[1]
    cf, sig = x[:nbas], x[nbas:]
    if mult:
        sig = np.abs(cf[ind]) * sig
    ss = aw[:, ind] * sig
    err = aw @ cf - bw
    stds = np.sqrt(np.sum(ss * ss, axis=1) + datavar)
    if method == "abc":
        return -0.5 * np.sum(((np.abs(err) - stds) / 0.1) ** 2) - 0.5 * np.log(2 * np.pi) - np.log(0.1)
    return -0.5 * np.sum((err / stds) ** 2) - 0.5 * len(bw) * np.log(2 * np.pi) - np.sum(np.log(stds))


@pytest.mark.parametrize("method,mult", [("abc", 0), ("iid", 1)])
def test_merr_class_transpose_trick_and_samples(method, mult, tmp_path, monkeypatch):
    # apply_transpose: the "rows" are the K rows of (G, c), on a context of their own; the resident rows stay bound.  Data
    # variance (npt = K: with the reference's formula it is minus half the tiny SSE of the square system) and
    # log-posterior against numpy on (G, c).
    monkeypatch.chdir(tmp_path)
    A, b, w, _, _ = _problem(4000, 10, 8)
    pt, s = _merr_solver(method, mult, "all", {"SOLVER": {"solver": "MERR", "merr_method": method, "merr_mult": mult,
                                                           "nsam": 5}, "EXTRAS": {"apply_transpose": 1}})
    np.random.seed(2)
    s.perform_fit(A, b, w, trainall=True)
    assert np.all(np.isfinite(s.fit)) and s.fit_sam.shape == (5, 10)
    assert pt.hip().m == 4000
    G, c, _ = s.last_statistics                      # (G, c) of the fit, the rows of the transposed system
    aw, bw = w[:, None] * A, w * b
    assert np.max(np.abs(G - aw.T @ aw)) <= 1e-12 * np.max(np.abs(G))
    assert np.max(np.abs(c - aw.T @ bw)) <= 1e-12 * np.max(np.abs(c))
    keep = np.diag(G) != 0.0
    Gc = G[:, keep]
    nbas = Gc.shape[1]
    invptp = np.linalg.pinv(Gc.T @ Gc)
    invptp = 0.5 * (invptp + invptp.T)
    res = c - Gc @ (invptp @ (Gc.T @ c))
    datavar = (res @ res / 2.0) / ((len(c) - nbas) / 2.0 - 1.0)           # npt = K rows of the transposed system
    assert abs(s.datavar - datavar) <= 1e-12 * (c @ c)
    # the value at the start (sigmas drawn in (0, 1)) -- at the optimum some v_i = x_i^2 q + d approach the tiny d, and
    # the value is too ill-conditioned there for a tight comparison
    L0 = _np_logpost(s.params_ini, Gc, c, np.arange(nbas), s.datavar, mult, method)
    assert abs(s.logpost_ini - L0) <= 1e-10 * abs(L0), (s.logpost_ini, L0)
    assert s.logpost >= s.logpost_ini
    pt.free()


def test_merr_class_pace_width_completes(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    r = np.random.default_rng(142)
    m, K = 13_035, 142
    A = r.standard_normal((m, K)) * np.exp(r.standard_normal(K))
    b = A @ r.standard_normal(K) + 0.05 * r.standard_normal(m) * (1.0 + np.abs(A[:, 0]))
    w = 0.5 + r.random(m)
    pt, s = _merr_solver("iid", 0, "all")
    np.random.seed(0)
    s.perform_fit(A, b, w, trainall=True)
    L0 = -s.objective(s.params_ini)[0]
    assert np.isfinite(s.logpost) and s.logpost >= L0
    pt.free()


def test_merr_two_ranks_p2p_match_one_rank(tmp_path, merr_ref):
    world = 2
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="merr two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "merr_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    r0, r1 = (dict(np.load(tmp_path / f"merr_rank{r}.npz")) for r in range(world))
    # the workers seed numpy with their rank: both must start from rank 0's draw and take the same steps
    assert np.array_equal(r0["params_ini"], r1["params_ini"]) and int(r0["evaluations"]) == int(r1["evaluations"])
    assert np.array_equal(r0["params"], r1["params"]) and np.array_equal(r0["fit"], r1["fit"])
    assert np.array_equal(r0["f"], r1["f"]) and np.array_equal(r0["grad"], r1["grad"])
    # one rank over the same rows
    A, b, w = _ta_subset(merr_ref)
    pt, s = _merr_solver("iid", 0, "all")
    s.save_files = False
    np.random.seed(0)
    s.perform_fit(A, b, w, trainall=True)
    nbas = A.shape[1]
    assert np.array_equal(s.params_ini[nbas:], r0["params_ini"][nbas:])      # rank 0's random draw (seed 0)
    f1, g1 = s.objective(r0["x"])
    assert abs(r0["f"] - f1) <= 1e-12 * abs(f1)
    # (the gradient's components are sums with cancellation, summed in another order over two ranks: the bound of the
    # evaluation test against extended precision)
    assert np.max(np.abs(r0["grad"] - g1)) <= 1e-11 * np.max(np.abs(g1))
    pt.free()


def test_python_m_fitsnap3_runs_merr(tmp_path, monkeypatch):
    # an input with solver = MERR and the keys of the reference's docs, through the drop-in entry point: the fit is the
    # class's, and .snapcoeff, mean.npy and covariance.npy are written
    import runpy

    import pandas as pd

    from fitsnap_amd.io.outputs.snap import parse_snapcoeff

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_cli_cpu import TA_IN

    z = np.load(os.path.join(GOLDEN, "ta_abw.npz"))
    A, b, w = z["A"], z["b"], z["w"]
    np.save(tmp_path / "Descriptors.npy", A)
    np.save(tmp_path / "Truth-Ref.npy", b)
    np.save(tmp_path / "Weights.npy", w)
    m = len(b)
    df = pd.DataFrame({"Row_Type": ["Energy"] * 363 + ["Force"] * 12672 + ["Stress"] * 2178, "Groups": ["Ta"] * m,
                       "Configs": ["c"] * m, "Testing": [False] * m, "Atom_I": [0] * m, "Atom_Type": [0] * m})
    df.to_pickle(tmp_path / "FitSNAP.df")
    text = TA_IN.replace("dump_descriptors = 1", "dump_descriptors = 0")
    text = text.replace("solver = SVD", "solver = MERR\nmerr_method = iid\nmerr_mult = 0\nmerr_cfs = all\nnsam = 0")
    (tmp_path / "Ta.in").write_text(text)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", ["fitsnap3", "Ta.in", "--descriptors", str(tmp_path), "--overwrite"])
    np.random.seed(0)
    with pytest.raises(SystemExit) as e:
        runpy.run_module("fitsnap3", run_name="__main__", alter_sys=True)
    assert e.value.code == 0
    mean, cov = np.load(tmp_path / "mean.npy"), np.load(tmp_path / "covariance.npy")
    assert mean.shape == (31,) and cov.shape == (31, 31) and np.all(np.isfinite(mean)) and np.all(np.diag(cov) > 0.0)
    coeffs = parse_snapcoeff(tmp_path / "Ta_pot.snapcoeff")
    assert np.max(np.abs(coeffs - mean)) <= 1e-10 * np.max(np.abs(mean))
    # the CLI's result, evaluated by the class on the same rows, is the optimum the class reaches from the same start
    pt, s = _merr_solver("iid", 0, "all")
    s.save_files = False
    np.random.seed(0)
    s.perform_fit(np.ascontiguousarray(A), np.ascontiguousarray(b), np.ascontiguousarray(w), trainall=True)
    L_cli = -s.objective(np.concatenate([mean, np.sqrt(np.diag(cov))]))[0]
    assert L_cli >= -s.objective(s.params_ini)[0]
    assert abs(L_cli - s.logpost) <= 1e-6 * abs(s.logpost), (L_cli, s.logpost)
    pt.free()

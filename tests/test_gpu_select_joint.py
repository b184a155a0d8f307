"""GPU: joint unit scores (fsnap_joint_*, kernels J1 / J2 of csrc/fsnap_joint.hip; Solver.unit_scores / select_units) -- the
kernels against the long-double evaluation of their formulas over K, both spaces, dim S beyond the LDS limit and ragged
blocks, bit-identity under repeats, permutations and subsets of the units, the session rules, the whole selection against
per-step refits (tests/select_joint_cases.py) on clustered pools and the golden Ta rows, two ranks, and the example.

The bar of the kernel test.  Kernel and numpy mirror are float64 evaluations of one formula that differ in summation order
only (MFMA 4-term groups against BLAS), so the mirror's error against long double, measured on these very cases on the CPU
(profiles/select_joint_accuracy.txt), sets the scale: worst relative error 7.1e-14 (gain) and 1.0e-14 (reduction), which
is 3.7e-3 and 4.2e-4 of the rounding bound derived from the term counts (select_joint_cases.long_double_scores).  The GPU
bar is 4 x the mirror's worst relative error, and never below that bound: per unit max(4 x worst x |ref|, bound)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import select_joint as sj, solver_factory

import select_cases as sc
import select_joint_cases as jc
from conftest import ROOT

EPS = jc.EPS
MIRROR_WORST = {"gain": 7.1e-14, "reduction": 1.0e-14}     # numpy mirror against long double, relative, on the CPU


def ctx_with(a):
    ctx = _capi.HipContext(0)
    ctx.upload_rows(a, np.zeros(a.shape[0]))
    return ctx


def make_solver(name="ANL"):
    pt = ParallelTools()
    return pt, solver_factory.solver(name, pt, Config(pt, {"SOLVER": {"solver": name}}))


def session(p, cat=None, a=None, w=None):
    cat = p["cat"] if cat is None else cat
    ctx = ctx_with(p["A"] if a is None else a)
    rows, off = sj.unit_layout(cat, p["ncat"])
    ctx.joint_begin(rows, off, p["w"] if w is None else w)
    return ctx


# ---------------------------------------------------------------------------------------
# 1. kernels J1 / J2 against long double
# ---------------------------------------------------------------------------------------
def check_against_long_double(p, res, tag):
    ref = jc.long_double_case(p)
    live = p["sizes"] > 0
    worst = {}
    for i, crit in enumerate(("gain", "reduction")):
        got, want, bound = res[crit], ref[i], ref[2 + i]
        assert np.all(np.isnan(got[~live])), crit
        err = np.abs(got[live] - want[live])
        bar = np.maximum(4 * MIRROR_WORST[crit] * np.abs(want[live]), bound[live])
        rel = err / np.maximum(np.abs(want[live]), 1e-300)
        worst[crit] = (float(np.max(np.where(want[live] != 0, rel, 0.0))), float(np.max(err / np.maximum(bound[live], 1e-300))))
        print(f"{tag} {crit}: worst relative error {worst[crit][0]:.2e}, worst error {worst[crit][1]:.3g} of the term-count bound")
        assert np.all(err <= bar), (tag, crit, np.flatnonzero(err > bar), p["sizes"][live][err > bar])
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("K", jc.KERNEL_KS)
def test_kernels_against_long_double(K):
    p = jc.kernel_case(K)
    J = p["M"].shape[1]
    assert J == K
    ctx = session(p)
    res = ctx.joint_score(p["M"], p["tau"], p["B"])
    info = res["info"]
    live = p["sizes"] > 0
    assert np.array_equal(info[live, 0], np.minimum(p["sizes"][live], J)) and np.array_equal(info[live, 3], p["sizes"][live])
    assert np.array_equal(info[live, 1], (p["sizes"][live] <= J).astype(float))
    assert np.all(info[live, 2] >= 1.0 - 64 * K * EPS)                    # pivots of I + PSD
    assert res["gain"][7] == 0.0 and res["reduction"][7] == 0.0           # the unit of weight zero, exactly
    check_against_long_double(p, res, f"K={K} J={J}")
    # the gain alone (no target block): the same bits
    only = ctx.joint_score(p["M"], p["tau"])
    assert only["reduction"] is None and np.array_equal(only["gain"], res["gain"], equal_nan=True)
    # a factor with fewer columns than K (J and r not multiples of 16), another noise variance
    J2 = K - 5
    q = dict(p, M=np.ascontiguousarray(p["M"][:, :J2]), B=np.ascontiguousarray(p["B"][:J2, :K - 3]), tau=3.0 * p["tau"])
    res2 = ctx.joint_score(q["M"], q["tau"], q["B"])
    assert np.array_equal(res2["info"][live, 0], np.minimum(p["sizes"][live], J2))
    check_against_long_double(q, res2, f"K={K} J={J2}")
    ctx.close()


# ---------------------------------------------------------------------------------------
# 2. bit-identity
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 128, 160])
def test_bit_identical_under_repeats_permutations_and_subsets(K):
    p = jc.kernel_case(K, seed=1)
    ncat = p["ncat"]
    ctx = session(p)
    first = ctx.joint_score(p["M"], p["tau"], p["B"])
    again = ctx.joint_score(p["M"], p["tau"], p["B"])
    for k in ("gain", "reduction"):
        assert np.array_equal(first[k], again[k], equal_nan=True), k
    # retiring units: the others keep their bits, the retired ones get NaN
    rng = np.random.default_rng(K)
    live = np.flatnonzero(p["sizes"] > 0)
    gone = rng.choice(live, len(live) // 2, replace=False)
    for u in gone:
        ctx.joint_retire(u)
    rest = ctx.joint_score(p["M"], p["tau"], p["B"])
    keep = np.setdiff1d(live, gone)
    for k in ("gain", "reduction"):
        assert np.array_equal(rest[k][keep], first[k][keep]) and np.all(np.isnan(rest[k][gone])), k
    ctx.close()
    # the units renumbered: the same bits under the new numbers
    perm = rng.permutation(ncat)
    cat2 = np.where(p["cat"] >= 0, perm[np.maximum(p["cat"], 0)], -1).astype(np.int32)
    c2 = session(p, cat=cat2)
    r2 = c2.joint_score(p["M"], p["tau"], p["B"])
    c2.close()
    for k in ("gain", "reduction"):
        assert np.array_equal(r2[k][perm], first[k], equal_nan=True), k
    # a subset of the units, as a subset of the rows (another m, other positions) in another unit order
    sub = np.isin(p["cat"], keep[::2])
    a3 = np.ascontiguousarray(p["A"][sub])
    c3 = session(p, cat=cat2[sub], a=a3, w=p["w"][sub])
    r3 = c3.joint_score(p["M"], p["tau"], p["B"])
    c3.close()
    for k in ("gain", "reduction"):
        assert np.array_equal(r3[k][perm[keep[::2]]], first[k][keep[::2]]), k


# ---------------------------------------------------------------------------------------
# 3. session rules and argument errors
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_session_rules():
    K = 16
    a = np.ascontiguousarray(np.random.default_rng(2).standard_normal((500, K)))
    ctx = ctx_with(a)
    cat = (np.arange(500) % 7).astype(np.int32)
    rows, off = sj.unit_layout(cat, 7)
    M = np.eye(K)
    with pytest.raises(ValueError, match="session"):
        ctx.joint_score(M, 1.0)
    ctx.joint_begin(rows, off)
    g = ctx.joint_score(M, 0.5)["gain"]
    assert np.all(g > 0)
    ctx.row_variance(M, _capi.UQ_QUAD, cat=cat, ncat=7)                 # leaves the session alone
    assert np.array_equal(ctx.joint_score(M, 0.5)["gain"], g)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            ctx.joint_score(M, bad)
    with pytest.raises(ValueError):
        ctx.joint_score(np.eye(K + 1), 0.5)                             # K of other rows
    with pytest.raises(ValueError, match="target"):
        ctx.joint_score(M, 0.5, None, want_reduction=True)
    ctx.joint_retire(3)
    with pytest.raises(ValueError, match="not alive"):
        ctx.joint_retire(3)
    with pytest.raises(ValueError, match="not alive"):
        ctx.joint_retire(7)
    assert np.isnan(ctx.joint_score(M, 0.5)["gain"][3])
    for u in (0, 1, 2, 4, 5, 6):
        ctx.joint_retire(u)
    assert np.all(np.isnan(ctx.joint_score(M, 0.5, np.eye(K))["reduction"]))       # no live unit: a no-op
    # whatever ends a selection session ends this one
    ctx.joint_begin(rows, off)
    ctx.upload_rows(a, np.zeros(500))
    for call in (lambda: ctx.joint_score(M, 0.5), lambda: ctx.joint_retire(0)):
        with pytest.raises(ValueError, match="session"):
            call()
    ctx.joint_begin(rows, off)
    ctx.joint_end()
    with pytest.raises(ValueError, match="session"):
        ctx.joint_score(M, 0.5)
    # begin: bad layouts
    with pytest.raises(ValueError):
        ctx.joint_begin(np.array([0, 0, 1]), np.array([0, 3]))          # a row twice
    with pytest.raises(ValueError):
        ctx.joint_begin(np.array([0, 500]), np.array([0, 2]))           # out of range
    with pytest.raises(ValueError):
        ctx.joint_begin(np.array([0, 1, 2]), np.array([0, 2, 1, 3]))    # offsets decrease
    with pytest.raises(ValueError):
        ctx.joint_begin(rows, off, np.ones(499))
    # no rows at all
    ctx.drop_rows()
    ctx.joint_begin(np.zeros(0, dtype=np.int32), np.zeros(4, dtype=np.int64))
    assert np.all(np.isnan(ctx.joint_score(M, 0.5)["gain"]))
    ctx.close()


# ---------------------------------------------------------------------------------------
# 4. through Solver.unit_scores / select_units, against refits
# ---------------------------------------------------------------------------------------
def check_units(sol, A, cat, ncat, w, P0, tau, T, ids, criterion, picks_must_match, **kw):
    res = sol.select_units(jc.PICKS, a=A, w=w, categories=kw.pop("categories", cat), criterion=criterion, **kw)
    ref = jc.refit_greedy(A, cat, ncat, P0, tau, w, jc.PICKS, criterion, T)
    got = [ids[k] for k in res.keys]
    assert len(got) == jc.PICKS
    excused = 0
    for t in range(jc.PICKS):
        C0 = tau * sc.info_inverse(P0)[0]
        bar = float(np.nanmax(jc.refit_bars(A, cat, ncat, C0, tau, w, T, ref["kappa"][t])[0 if criterion == "gain" else 1]))
        if not picks_must_match and ref["gaps"][t] <= 2 * bar / abs(ref["scores"][t]):
            excused += 1
            if got[t] != ref["picks"][t]:
                break
            continue
        assert got[t] == ref["picks"][t], (t, got, ref["picks"])
        assert abs(res.scores[t] - ref["scores"][t]) <= bar
    assert excused <= jc.PICKS // 8
    kappa = ref["kappa"][-1]
    dev = np.linalg.norm(res.cov - ref["cov"]) / np.linalg.norm(ref["cov"])
    print(f"{criterion}: picks {got}, smallest gap {min(ref['gaps']):.1e}, excused {excused}, covariance off by {dev:.2e} "
          f"(bar {16 * kappa * EPS:.2e})")
    assert dev <= 16 * kappa * EPS                                   # the bar of tests/test_gpu_select.py
    assert res.dims == [min(int((cat == u).sum()), A.shape[1]) for u in got]
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("seed,K,units,size_hi", jc.POOLS)
def test_select_units_matches_refits(seed, K, units, size_hi):
    p = jc.pool(seed, K, units, size_hi)
    A, cat, ncat, w, s = p["A"], p["cat"], p["ncat"], p["w"], p["s"]
    pt, sol = make_solver()
    sol.cov = p["C0"]
    ident = {c: c for c in range(ncat)}
    for criterion in sj.CRITERIA:
        # target=None: the pool itself with row_scale, its Gram from the statistics kernel
        res = check_units(sol, A, cat, ncat, w, p["P0"], p["tau"], p["T"], ident, criterion, False, row_scale=s, noise=p["tau"])
        assert res.all_keys == list(range(ncat))
    one = sol.unit_scores(a=A, w=w, categories=cat, row_scale=s, noise=p["tau"])
    g, r, kappa = jc.refit_scores(A, cat, ncat, p["P0"], p["tau"], w, p["T"])
    gbar, rbar = jc.refit_bars(A, cat, ncat, p["C0"], p["tau"], w, p["T"], kappa)
    assert np.all(np.abs(one["gain"] - g) <= gbar) and np.all(np.abs(one["reduction"] - r) <= rbar)
    assert abs(one["total"] - np.trace(p["T"] @ p["C0"])) <= 16 * kappa * EPS * one["total"]
    assert np.array_equal(one["count"], np.bincount(cat, minlength=ncat)) and np.all(one["reduction"] <= one["total"])
    # the same target given as rows with a scale and as a Gram; a cost per unit; labels as units
    host = sj.unit_scores_host(A, cat, ncat, p["C0"], w, p["tau"], p["T"])
    for target in ((A, s), ("gram", p["T"])):
        alt = sol.unit_scores(a=A, w=w, categories=cat, criteria="reduction", target=target, noise=p["tau"])
        assert alt["gain"] is None and np.allclose(alt["reduction"], host["reduction"], rtol=1e-9, atol=0)
    cost = np.bincount(cat, minlength=ncat).astype(float) ** 3
    labels = [f"cfg{c}" for c in cat]
    costed = sol.select_units(3, a=A, w=w, categories=labels, unit_cost=cost, noise=p["tau"], cov=p["C0"])
    hc = sj.greedy_joint_host(A, cat, ncat, p["C0"], w, p["tau"], 3, "gain", unit_cost=cost)
    assert min(hc["gaps"]) > 1e-9 and costed.keys == [f"cfg{c}" for c in hc["picks"]]
    assert np.allclose(costed.initial_scores, hc["initial"], rtol=1e-10, atol=0)
    # argument errors through the public interface
    with pytest.raises(ValueError, match="criterion"):
        sol.select_units(2, a=A, categories=cat, criterion="sum", noise=p["tau"])
    with pytest.raises(ValueError):
        sol.unit_scores(a=A, categories=cat, target=np.ones((3, K + 1)), noise=p["tau"])
    with pytest.raises(ValueError, match="cost"):
        sol.unit_scores(a=A, categories=cat, unit_cost=-cost, noise=p["tau"])
    with pytest.raises(ValueError, match="noise"):
        sol.unit_scores(a=A, categories=cat, noise=-1.0)
    sol.sigmahat = None
    with pytest.raises(ValueError, match="noise variance"):
        sol.select_units(2, a=A, categories=cat)
    sol.cov = None
    with pytest.raises(ValueError, match="covariance"):
        sol.select_units(2, a=A, categories=cat, noise=p["tau"])
    pt.free()


@pytest.mark.gpu
def test_select_units_on_the_ta_rows(ta):
    A, b, w = ta
    ntr = 12000
    pt, s = make_solver()
    s.save_files = False
    pt.create_shared_array("a", ntr, A.shape[1])
    pt.create_shared_array("b", ntr)
    pt.create_shared_array("w", ntr)
    pt.shared_arrays["a"].array[:] = A[:ntr]
    pt.shared_arrays["b"].array[:] = b[:ntr]
    pt.shared_arrays["w"].array[:] = w[:ntr]
    pt.fitsnap_dict["Testing"] = [False] * ntr
    s.keep_resident = True
    s.perform_fit()
    assert s.sigmahat is not None and s.sigmahat > 0
    fit0 = s.fit.copy()
    Ap, wp = np.ascontiguousarray(A[ntr:]), np.ascontiguousarray(w[ntr:])
    cat, ncat = sc.ta_configurations(len(Ap))
    labels = [f"cfg{c}" for c in cat]
    ids = {f"cfg{c}": c for c in range(ncat)}
    Aw = A[:ntr] * w[:ntr, None]
    P0 = Aw.T @ Aw                                   # cov_nugget = 0
    T = Ap.T @ (wp[:, None] ** 2 * Ap)
    # kappa(P0) = 7e10 makes the refits' own bar wider than the gaps, yet the sequences are the reference's at every step
    for criterion in sj.CRITERIA:
        check_units(s, Ap, cat, ncat, wp, P0, s.sigmahat, T, ids, criterion, True, categories=labels, row_scale=wp ** 2)
    # the shared rows themselves as pool and target (a=None): the weights of the fit come back with the next fit
    cat_t, ncat_t = sc.ta_configurations(ntr, seed=6)
    res = s.select_units(4, categories=cat_t, criterion="reduction")
    host = sj.greedy_joint_host(A[:ntr], cat_t, ncat_t, s.cov, w[:ntr], s.sigmahat, 4, "reduction", A[:ntr].T @ A[:ntr])
    assert min(host["gaps"]) > 1e-9 and res.keys == host["picks"]
    s.perform_fit()
    assert np.allclose(s.fit, fit0, rtol=1e-9, atol=0)
    pt.free()


# ---------------------------------------------------------------------------------------
# 5. two ranks over the peer-to-peer transport, one GPU
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_ranks_match_one_process(tmp_path):
    world = 2
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="joint two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "select_joint_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    parts = [dict(np.load(tmp_path / f"joint_rank{r}.npz")) for r in range(world)]
    from select_joint_dist_worker import BATCH, pool
    p = pool()
    order = np.concatenate([q["rows"] for q in parts])                   # rank-major
    A, w, s, cat = np.ascontiguousarray(p["A"][order]), p["w"][order], p["s"][order], p["cat"][order]
    pt, sol = make_solver()
    sol.cov = p["C0"]
    for crit in sj.CRITERIA:
        one = sol.select_units(BATCH, a=A, w=w, categories=[f"cfg{c}" for c in cat], criterion=crit, row_scale=s, noise=p["tau"])
        picked = [int(k[3:]) for k in one.keys]
        for q in parts:
            assert q[f"{crit}_picked"].tolist() == picked and q[f"{crit}_dims"].tolist() == one.dims
            assert np.array_equal(q[f"{crit}_cov"], one.cov)               # the same rows in the same order: the same downdates
            if crit == "gain":
                assert np.array_equal(q[f"{crit}_scores"], one.scores)     # a unit's bits do not depend on the other units
            else:                                                          # the target Gram is a sum of two parts there
                assert np.allclose(q[f"{crit}_scores"], one.scores, rtol=1e-10, atol=0)
        init = dict(zip(one.all_keys, one.initial_scores))
        for q in parts:
            mine = np.array([init[f"cfg{c}"] for c in q[f"{crit}_keys"]])
            assert np.allclose(q[f"{crit}_initial"], mine, rtol=1e-10, atol=0)
        assert {c % world for c in picked} == {0, 1}                       # both ranks took part in the picks
    pt.free()


# ---------------------------------------------------------------------------------------
# 6. the example
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_active_learning_joint_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "active_learning_joint.py"), "--batch", "6", "--check"],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "joint selections match the numpy statement" in r.stdout
    assert "information gained" in r.stdout and "pool variance left" in r.stdout

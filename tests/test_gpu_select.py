"""GPU: greedy batch selection (fsnap_select_*, kernels of csrc/fsnap_select.hip; Solver.select_batch) -- the downdate kernel
against long double over K, J, m and lda, determinism under repeats, permutations, subsets and lda, the scores and the pick on
the device, the whole selection against per-step refits (tests/select_cases.py), residency of the training rows, a stale
session, two ranks, 10^6 rows and the example."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import select, solver_factory

import select_cases as sc
from conftest import ROOT

EPS = sc.EPS
GAP_MIN = 1e-9
OBJ = _capi.SELECT_OBJECTIVES


def rows(m, K, seed, lda=None):
    big = np.random.default_rng(seed).standard_normal((m, lda or K))
    return big[:, :K]                       # lda > K: a strided view, uploaded with its own leading dimension


def psd(K, seed):
    X = np.random.default_rng(seed).standard_normal((K + 3, K))
    return X.T @ X / (K + 3)


def ctx_with(a):
    ctx = _capi.HipContext(0)
    ctx.upload_rows(a, np.zeros(a.shape[0]))
    return ctx


def make_solver(name="ANL", extra=None):
    pt = ParallelTools()
    d = {"SOLVER": {"solver": name}}
    d.update(extra or {})
    return pt, solver_factory.solver(name, pt, Config(pt, d))


def drive(ctx, A, cat, ncat, C0, w, tau, batch, scale=None, objective="sum"):
    """The selection loop on the C-ABI session with select.py's factors: (picks, scores, factors, state)."""
    ctx.select_begin(C0, _capi.UQ_QUAD, scale=scale, cat=cat, ncat=ncat, objective=OBJ[objective])
    C = C0
    picks, scores, factors = [], [], []
    for _ in range(batch):
        c, s = ctx.select_pick()
        if c < 0:
            break
        V = select.downdate_factor(C, w[cat == c, None] * A[cat == c], tau)
        C = select.downdate_cov(C, V)
        ctx.select_downdate(V)
        picks.append(c)
        scores.append(s)
        factors.append(V)
    return picks, scores, factors, ctx.select_state()


# ---------------------------------------------------------------------------------------
# 1. kernel B1 against long double
# ---------------------------------------------------------------------------------------
KS = [1, 15, 16, 17, 31, 64, 128, 142, 144, 145, 256, 480] + [40, 80, 96, 112]     # + the other tile counts of B1
JS = [1, 15, 16, 17, 133, 300]
MS = [1, 63, 64, 65, 1000, 15213]


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_downdate_against_long_double(K):
    C0 = psd(K, K)
    for i, m in enumerate(MS):
        a = rows(m, K, 100 * K + m, K + 3 + i)                  # lda > K
        js = [JS[(i + 2 * t) % 6] for t in range(3)]            # every J with every parity of m over the loop
        Vs = [np.random.default_rng(K * 1000 + J + m).standard_normal((K, J)) / np.sqrt(8.0 * K * J) for J in js]
        ctx = ctx_with(a)
        cat = np.zeros(m, dtype=np.int32)
        ctx.select_begin(C0, _capi.UQ_QUAD, cat=cat, ncat=1)
        for V in Vs:
            ctx.select_downdate(V)
        var = ctx.select_state()["var"]
        ctx.close()
        # every row; for the largest products 1000 random rows plus the last 128 (the partly filled tail block)
        sel = np.arange(m) if m * K <= 1_000_000 else np.union1d(np.random.default_rng(m).choice(m, 1000, replace=False),
                                                                 np.arange(m - 128, m))
        ac = np.ascontiguousarray(a[sel])
        ref, bar = sc.long_double_var(ac, C0, Vs), sc.kernel_bar(ac, C0, Vs)
        worst = float(np.max(np.abs(var[sel] - ref) / bar))
        print(f"K={K} m={m} J={js}: worst error {worst:.3f} of the bar")
        assert np.all(np.abs(var[sel] - ref) <= bar), (K, m, js)


# ---------------------------------------------------------------------------------------
# 2. determinism
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 128, 160])
def test_bit_identical_under_repeat_permutation_subset_and_lda(K):
    p = sc.clustered(40 + K, K, n_pool=120, size_hi=200)
    A, cat, ncat, w, s = p["A"], p["cat"], p["ncat"], p["w"], p["s"]
    m = A.shape[0]
    ctx = ctx_with(A)
    picks, scores, Vs, st = drive(ctx, A, cat, ncat, p["C0"], w, p["tau"], 6, s)
    assert len(picks) == 6
    # the value B1 subtracts has the bits of the NORM pass
    ctx.select_begin(p["C0"], _capi.UQ_QUAD, scale=s, cat=cat, ncat=ncat)
    v0 = ctx.select_state()["var"]
    assert np.array_equal(v0, ctx.row_variance(p["C0"], _capi.UQ_QUAD)["var"])
    ctx.select_downdate(Vs[0])
    assert np.array_equal(ctx.select_state()["var"], v0 - ctx.row_variance(Vs[0], _capi.UQ_NORM)["var"])
    # repeat
    p2, s2, V2, st2 = drive(ctx, A, cat, ncat, p["C0"], w, p["tau"], 6, s)
    assert p2 == picks and s2 == scores and all(np.array_equal(x, y) for x, y in zip(Vs, V2))
    for k in ("var", "cat_sum", "cat_max", "alive"):
        assert np.array_equal(st[k], st2[k]), k
    ctx.close()
    rng = np.random.default_rng(5)
    # a row permutation with permuted categories: the same picks (the factors are recomputed from the permuted rows of X
    # and differ in rounding) ...
    perm = rng.permutation(m)
    c2 = ctx_with(np.ascontiguousarray(A[perm]))
    p3, _, _, _ = drive(c2, A[perm], cat[perm], ncat, p["C0"], w[perm], p["tau"], 6, s[perm])
    assert p3 == picks
    # ... and with the SAME factors the same bits per row
    c2.select_begin(p["C0"], _capi.UQ_QUAD, scale=s[perm], cat=cat[perm], ncat=ncat)
    for V in Vs:
        c2.select_downdate(V)
    assert np.array_equal(c2.select_state()["var"], st["var"][perm])
    c2.close()
    # lda: a strided view of the same rows, the same factors
    big = np.zeros((m, K + 5))
    big[:, :K] = A
    c3 = ctx_with(big[:, :K])
    p4, s4, V4, st4 = drive(c3, A, cat, ncat, p["C0"], w, p["tau"], 6, s)
    c3.close()
    assert p4 == picks and s4 == scores and np.array_equal(st4["var"], st["var"])
    # a subset of the rows (whole configurations missing, others thinned) with the SAME factors: the same bits per row
    sub = np.sort(rng.choice(m, m // 3, replace=False))
    c4 = ctx_with(np.ascontiguousarray(A[sub]))
    c4.select_begin(p["C0"], _capi.UQ_QUAD, scale=s[sub], cat=cat[sub], ncat=ncat)
    for V in Vs:
        c4.select_downdate(V)
    assert np.array_equal(c4.select_state()["var"], st["var"][sub])
    c4.close()

@pytest.mark.gpu
def test_begin_rejects_a_category_array_of_another_length():
    ctx = ctx_with(rows(100, 16, 1))
    with pytest.raises(ValueError):
        ctx.select_begin(np.eye(16), _capi.UQ_QUAD, cat=np.zeros(99, dtype=np.int32), ncat=1)
    with pytest.raises(ValueError):
        ctx.select_begin(np.eye(16), _capi.UQ_QUAD, cat=np.zeros(100, dtype=np.int32), ncat=1, objective=7)
    with pytest.raises(ValueError):
        ctx.select_begin(np.eye(17), _capi.UQ_QUAD, cat=np.zeros(100, dtype=np.int32), ncat=1)
    with pytest.raises(ValueError):
        ctx.select_pick()                                   # none of these began a session
    ctx.close()


# ---------------------------------------------------------------------------------------
# 3. scores and pick
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("objective", ["sum", "max", "mean"])
def test_scores_and_pick(objective):
    m, K, ncat = 15213, 31, 50
    a = np.ascontiguousarray(rows(m, K, 11))
    C0 = psd(K, 4)
    rng = np.random.default_rng(9)
    cat = rng.integers(-1, ncat - 3, m).astype(np.int32)        # scattered, some rows skipped, the last 3 categories empty
    cat[:3000] = 7                                               # one category over several chunks
    scale = rng.uniform(0.1, 3.0, m)
    ctx = ctx_with(a)
    ctx.select_begin(C0, _capi.UQ_QUAD, scale=scale, cat=cat, ncat=ncat, objective=OBJ[objective])
    ctx.select_downdate(rng.standard_normal((K, 5)) * 0.05)

    def check_state(alive_expected):
        st = ctx.select_state()
        sv = scale * st["var"]
        assert np.array_equal(st["alive"], alive_expected)
        for c in np.flatnonzero(alive_expected):
            sel = cat == c
            assert st["cat_count"][c] == sel.sum()
            ref = math.fsum(sv[sel])
            assert abs(st["cat_sum"][c] - ref) <= 1e-15 * abs(ref) * max(1, np.log2(sel.sum())), c
            assert st["cat_max"][c] == sv[sel].max()
        return st

    alive = np.array([(cat == c).any() for c in range(ncat)])
    assert not alive[-3:].any()
    st = check_state(alive)
    seen = []
    peek = ctx.select_pick(retire=False)
    assert ctx.select_pick(retire=False) == peek
    for step in range(ncat):
        sc_now = select.scores_of(st["cat_sum"], st["cat_max"], st["cat_count"], objective)
        c, s = ctx.select_pick()
        if step == 0:
            assert (c, s) == peek
        if c < 0:
            break
        assert alive[c] and c not in seen and c == select.best_live(sc_now, alive) and s == sc_now[c]
        seen.append(c)
        alive[c] = False
        if step % 9 == 0:
            ctx.select_downdate(rng.standard_normal((K, 3)) * 0.02)
            st = check_state(alive)
    assert len(seen) == ncat - 3 and not alive.any()
    assert ctx.select_pick() == (-1, 0.0) and ctx.select_pick() == (-1, 0.0)        # exhausted
    with pytest.raises(ValueError):
        ctx.select_retire(seen[0])
    # retire by hand: the category never comes back
    ctx.select_begin(C0, _capi.UQ_QUAD, scale=scale, cat=cat, ncat=ncat, objective=OBJ[objective])
    first = ctx.select_pick(retire=False)[0]
    ctx.select_retire(first)
    assert ctx.select_pick()[0] != first
    ctx.select_end()
    with pytest.raises(ValueError):
        ctx.select_state()
    ctx.close()


@pytest.mark.gpu
def test_ties_go_to_the_lowest_category():
    K = 16
    blk = rows(40, K, 3)
    a = np.ascontiguousarray(np.vstack([blk * 0.5, blk, blk, blk]))
    cat = np.repeat(np.array([0, 3, 1, 2], dtype=np.int32), 40)
    ctx = ctx_with(a)
    ctx.select_begin(np.eye(K), _capi.UQ_QUAD, cat=cat, ncat=4)
    st = ctx.select_state()
    assert st["cat_sum"][1] == st["cat_sum"][2] == st["cat_sum"][3] > st["cat_sum"][0]
    assert [ctx.select_pick()[0] for _ in range(5)] == [1, 2, 3, 0, -1]
    ctx.close()


# ---------------------------------------------------------------------------------------
# 4. end to end through Solver.select_batch, against per-step refits
# ---------------------------------------------------------------------------------------
def check_selection(res, keys_to_id, A, cat, ncat, P0, tau, w, scale, objective, batch, C0):
    ref = sc.refit_reference(A, cat, ncat, P0, tau, w, batch, scale, objective)
    assert min(ref["gaps"]) > GAP_MIN, ("bad input: choose another seed", ref["gaps"])
    got = [keys_to_id[k] for k in res.keys]
    assert got == ref["picks"], (got, ref["picks"])
    kappa = max(ref["kappa"])
    assert np.allclose(res.scores, ref["scores"], rtol=16 * kappa * EPS, atol=0)
    # the factors of these picks, for the kernel's bar
    C, Vs = C0, []
    for u in ref["picks"]:
        Vs.append(select.downdate_factor(C, w[cat == u, None] * A[cat == u], tau))
        C = select.downdate_cov(C, Vs[-1])
    assert res.ranks == [V.shape[1] for V in Vs]
    rv = ref["var"][-1]
    bar = 16 * ref["kappa"][-1] * EPS * np.abs(rv) + sc.kernel_bar(A, C0, Vs)
    err = np.abs(res.var - rv)
    print(f"{objective}: worst variance error {float(np.max(err / np.maximum(bar, 1e-300))):.3f} of the bar, kappa {kappa:.2e}, "
          f"min gap {min(ref['gaps']):.1e}")
    assert np.all(err <= bar)
    rc = ref["cov"][-1]
    assert np.linalg.norm(res.cov - rc) <= 16 * ref["kappa"][-1] * EPS * np.linalg.norm(rc)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("K,seed", [(31, 13), (128, 14)])
def test_select_batch_matches_refits(K, seed):
    p = sc.clustered(seed, K)
    A, cat, ncat, w, s = p["A"], p["cat"], p["ncat"], p["w"], p["s"]
    pt, sol = make_solver("ANL")
    sol.cov = p["C0"]
    ident = {c: c for c in range(ncat)}
    for objective in ("sum", "max", "mean"):
        res = sol.select_batch(16, a=A, w=w, categories=cat, row_scale=s, objective=objective, noise=p["tau"])
        assert len(res.keys) == 16 and res.all_keys == list(range(ncat))
        check_selection(res, ident, A, cat, ncat, p["P0"], p["tau"], w, s, objective, 16, p["C0"])
        pv = sol.prediction_variance(A, categories=cat, row_scale=s, want_preds=False)
        assert np.array_equal(res.initial_scores, pv["cat_" + objective])
    # labels as categories, no scale, unit weights; more picks asked for than there are units
    labels = ([f"g{c % 4}" for c in cat], [f"cfg{c}" for c in cat])
    few = cat < 5
    res = sol.select_batch(9, a=np.ascontiguousarray(A[few]), categories=tuple(np.asarray(col)[few].tolist() for col in labels),
                           noise=p["tau"], cov=p["C0"])
    assert len(res.keys) == 5 and sorted(res.keys) == sorted({(f"g{c % 4}", f"cfg{c}") for c in range(5)})
    pt.free()


@pytest.mark.gpu
def test_select_batch_on_the_ta_rows(ta):
    A, b, w = ta
    ntr = 12000
    pt, s = make_solver("ANL")
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
    Ap, wp = np.ascontiguousarray(A[ntr:]), np.ascontiguousarray(w[ntr:])
    cat, ncat = sc.ta_configurations(len(Ap))
    labels = [f"cfg{c}" for c in cat]
    ids = {f"cfg{c}": c for c in range(ncat)}
    Aw = A[:ntr] * w[:ntr, None]
    P0 = Aw.T @ Aw                                   # cov_nugget = 0
    for objective in ("sum", "mean"):
        res = s.select_batch(8, a=Ap, w=wp, categories=labels, objective=objective)      # noise: the fit's sigma^2
        check_selection(res, ids, Ap, cat, ncat, P0, s.sigmahat, wp, None, objective, 8, s.cov)
        pv = s.prediction_variance(Ap, categories=labels)
        assert np.array_equal(res.initial_scores, pv["cat_" + objective])
    # residency: the pool went to the second context, the next fit does not upload the training rows again
    main = pt.hip()
    calls = {"main": 0}
    real = main.upload_rows

    def count(*x, **k):
        calls["main"] += 1
        return real(*x, **k)

    main.upload_rows = count
    s.select_batch(3, a=Ap, w=wp, categories=labels)
    s.perform_fit()
    assert calls["main"] == 0
    # the shared rows themselves, with the shared weights
    cat_t, ncat_t = sc.ta_configurations(ntr, seed=6)
    res = s.select_batch(4, categories=cat_t)
    host = select.greedy_host(A[:ntr], cat_t, ncat_t, s.cov, w[:ntr], s.sigmahat, 4)
    assert res.keys == host["picks"]
    pt.free()


@pytest.mark.gpu
def test_stale_session():
    a = np.ascontiguousarray(rows(500, 16, 2))
    ctx = ctx_with(a)
    cat = (np.arange(500) % 7).astype(np.int32)
    ctx.select_begin(np.eye(16), _capi.UQ_QUAD, cat=cat, ncat=7)
    assert ctx.select_pick()[0] >= 0
    ctx.row_variance(np.eye(16), _capi.UQ_QUAD, cat=(cat + 1) % 7, ncat=7)       # leaves the session alone
    assert ctx.select_pick()[0] >= 0
    ctx.upload_rows(np.ascontiguousarray(rows(500, 16, 3)), np.zeros(500))
    for call in (ctx.select_pick, ctx.select_state, lambda: ctx.select_downdate(np.ones((16, 1))), lambda: ctx.select_retire(0)):
        with pytest.raises(ValueError, match="session"):
            call()
    ctx.select_begin(np.eye(16), _capi.UQ_QUAD, cat=cat, ncat=7)
    assert ctx.select_pick()[0] >= 0
    ctx.close()


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
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="select two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "select_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    parts = [dict(np.load(tmp_path / f"select_rank{r}.npz")) for r in range(world)]
    from select_dist_worker import BATCH, pool
    p = pool()
    order = np.concatenate([q["rows"] for q in parts])                   # rank-major
    A, w, s, cat = np.ascontiguousarray(p["A"][order]), p["w"][order], p["s"][order], p["cat"][order]
    pt, sol = make_solver("ANL")
    sol.cov = p["C0"]
    one = select.select_batch(sol, BATCH, a=A, w=w, categories=[f"cfg{c}" for c in cat], row_scale=s, noise=p["tau"],
                              keep_factors=True)
    for q in parts:
        assert [f"cfg{c}" for c in q["picked"]] == one.keys
        assert np.array_equal(q["scores"], one.scores) and np.array_equal(q["cov"], one.cov) and q["ranks"].tolist() == one.ranks
    same_v = all(np.array_equal(parts[0][f"V{t}"], V) for t, V in enumerate(sol._select_factors))
    bar = sc.kernel_bar(A, p["C0"], sol._select_factors)
    var = np.concatenate([q["var"] for q in parts])
    if same_v:
        assert np.array_equal(var, one.var)
    else:
        assert np.all(np.abs(var - one.var) <= 2 * bar)
    # both ranks took part in the picks
    owners = {int(c) % world for c in parts[0]["picked"]}
    assert owners == {0, 1}
    pt.free()


# ---------------------------------------------------------------------------------------
# 6. full size
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_million_rows_k128():
    p = sc.clustered(77, 128, n_pool=6000, size_lo=30, size_hi=300)
    A, cat, ncat, w = p["A"], p["cat"], p["ncat"], p["w"]
    assert A.shape[0] > 900_000
    pt, sol = make_solver("ANL")
    sol.cov = p["C0"]
    res = sol.select_batch(8, a=A, w=w, categories=cat, noise=p["tau"])
    host = select.greedy_host(A, cat, ncat, p["C0"], w, p["tau"], 8)
    assert len(host["picks"]) == 8 and min(host["gaps"]) > GAP_MIN, ("bad input: choose another seed", host["gaps"])
    assert res.keys == host["picks"]
    bar = sc.kernel_bar(A, p["C0"], host["factors"])
    err = np.abs(res.var - host["var"])
    for u, got, want in zip(host["picks"], res.scores, host["scores"]):      # a score: the sum of at most 300 such rows
        assert abs(got - want) <= bar[cat == u].sum() + 600 * EPS * abs(want)
    print(f"10^6 x 128: worst difference to the float64 run {float(np.max(err / bar)):.3f} of the bar")
    assert np.all(err <= bar)
    spot = np.random.default_rng(1).choice(A.shape[0], 64, replace=False)
    ref = sc.long_double_var(A[spot], p["C0"], host["factors"])
    assert np.all(np.abs(res.var[spot] - ref) <= bar[spot])
    pt.free()


# ---------------------------------------------------------------------------------------
# 7. the example
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_active_learning_batch_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "active_learning_batch.py"), "--batch", "8", "--check"],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "greedy batch matches the numpy statement" in r.stdout
    assert "total pool variance left" in r.stdout

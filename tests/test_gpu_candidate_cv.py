"""GPU: grouped K-fold cross-validation of weight candidates (``CandidateFits.cross_validate``, kernels V0, V1, V2 of
csrc/fsnap_cv.hip) against the refit on the rows (oracle R of tests/candidate_cv_cases.py) at bars of 10 x what the plain
numpy restatement of the kernels differs from that oracle by -- the geometry sweep through the C ABI, determinism and batch
invariance, dead columns and failed pivots, the Ta golden rows, the composed route beyond 144 columns and two ranks over the
peer-to-peer transport."""
import os
import subprocess
import sys

import numpy as np
import pytest

import candidate_cv_cases as cc
from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import CandidateFits, solver_factory
from fitsnap_amd.solvers import candidates_cv as ccv

from conftest import ROOT

F, C = cc.SWEEP_F, cc.SWEEP_C


def make_solver(name, extra=None):
    pt = ParallelTools()
    d = {"SOLVER": {"solver": name}}
    d.update(extra or {})
    return pt, solver_factory.solver(name, pt, Config(pt, d))


def prepared(ctx, A, b, w0, ccat):
    ctx.upload_rows(A, b)
    ctx.set_weights(w0, None)
    layout = ctx.cat_prepare(ccat, F * C)
    ctx.cat_normal_eq(layout)
    return layout


def labelled(A, b, w0, ccat):
    """The rows of a sweep case that have a category, with labels under which ``CandidateFits`` builds the same composite
    categories: category c = (group c // 2, energy | force), five units per fold, folds by mapping."""
    keep = ccat >= 0
    A, b, w0, ccat = np.ascontiguousarray(A[keep]), b[keep], w0[keep], ccat[keep]
    fold, c = ccat // C, ccat % C
    fs = {"Groups": [f"g{int(x) // 2}" for x in c], "Testing": [False] * len(b),
          "Row_Type": ["Force" if int(x) % 2 else "Energy" for x in c], "Configs": [f"f{int(f)}u{i % 5}" for i, f in enumerate(fold)]}
    folds = {f"f{f}u{u}": f for f in range(F) for u in range(5)}
    return A, b, w0, ccat, fs, folds


# ---------------------------------------------------------------------------------------
# 1. the sweep through the C ABI
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", cc.SWEEP_CASES)
def test_sweep_matches_the_refit_on_the_rows(name):
    A, b, w0, ccat, K = cc.sweep_case(name)
    S = cc.sweep_scales(name)
    ctx = _capi.HipContext(0)
    try:
        layout = prepared(ctx, A, b, w0, ccat)
        for ia in range(len(cc.ALPHA_FRACTIONS)):
            alpha, ref, ref_sums, counts, bl = cc.sweep_oracle(name, ia)
            runs = {}
            for P in cc.BATCHES:
                coef, info = ctx.cv_candidates(layout, alpha, S[:P], F, K)
                runs[P] = (coef, info, ctx.cv_candidate_rows(layout, coef, C))
            coef, info, sums = runs[cc.SWEEP_P]
            ka = cc.worst_backward(bl, S, F, C, K, alpha, coef) if not info[:, :, 0].any() else np.nan
            kb = cc.worst_heldout(sums, ref_sums, counts, S, F)
            kc = cc.worst_forward(coef, ref)
            print(f"{name} alpha {alpha:.2e}: backward {ka:.2e} held-out {kb:.2e} forward {kc:.2e} min pivot {info[:, :, 1].min():.2e}")
            assert not info[:, :, 0].any(), (name, alpha, np.argwhere(info[:, :, 0] != 0))      # status 0 for ALL problems
            assert ka <= cc.BACKWARD_BAR and kb <= cc.HELDOUT_REL and kc <= cc.FORWARD_REL, (name, alpha, ka, kb, kc)
            assert np.all(info[:, :, 2] == K) and info[:, :, 1].min() > cc.PIVOT_FLOOR
            per_cat = counts.reshape(F, C)
            n = (S * S) @ (per_cat.sum(axis=0)[None, :] - per_cat).T
            assert np.allclose(info[:, :, 3], n, rtol=1e-14, atol=0)
            # the weighted sums against the long-double ones, and empty composite categories
            has = ref_sums[:, :, 0] > 0
            assert np.all(np.abs(sums - ref_sums)[has] <= cc.HELDOUT_REL * ref_sums[has])
            assert np.all(sums[~has] == 0.0)
            # the 16-candidate tile edge: batches of 1 and 16 are the first problems of the batch of 17, bit for bit
            for P in cc.BATCHES[:-1]:
                for got, want in zip(runs[P], runs[cc.SWEEP_P]):
                    assert np.array_equal(got, want[:P]), (name, alpha, P)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------
# 2. determinism and batch invariance
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["65", "chunks"])
def test_bits_do_not_depend_on_the_run_or_the_batch(name):
    A, b, w0, ccat, K = cc.sweep_case(name)
    S = cc.sweep_scales(name)
    alpha = cc.sweep_oracle(name, 1)[0]
    ctx = _capi.HipContext(0)
    try:
        layout = prepared(ctx, A, b, w0, ccat)

        def run(Sb):
            coef, info = ctx.cv_candidates(layout, alpha, Sb, F, K)
            return coef, info, ctx.cv_candidate_rows(layout, coef, C)

        first, second = run(S), run(S)
        for x, y in zip(first, second):
            assert np.array_equal(x, y)
        perm = np.random.default_rng(3).permutation(cc.SWEEP_P)
        shuffled = run(S[perm])
        for x, y in zip(first, shuffled):
            assert np.array_equal(x[perm], y)
        for p in (0, 9, 16):
            alone = run(S[p:p + 1])
            for x, y in zip(first, alone):
                assert np.array_equal(x[p:p + 1], y), p
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------
# 3. dead columns and failed pivots
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dead_column_gets_zero():
    A, b, w0, ccat, K = cc.sweep_case("7")
    A = A.copy()
    A[ccat // C != 1, 2] = 0.0                     # fold 1 alone touches column 2
    S = cc.sweep_scales("7")[:4]
    bl = cc.blocks_ld(A, b, w0, ccat, F * C)
    ctx = _capi.HipContext(0)
    try:
        layout = prepared(ctx, A, b, w0, ccat)
        coef, info = ctx.cv_candidates(layout, 0.0, S, F, K)
    finally:
        ctx.close()
    assert not info[:, :, 0].any()
    assert np.array_equal(info[:, :, 2], np.tile([K, K - 1, K], (4, 1)))
    for p in range(4):
        for f in range(F):
            ref = np.asarray(cc.refit_ld(bl, S[p], f, F, C, K, 0.0), dtype=np.float64)
            assert (coef[p, f, 2] == 0.0) == (f == 1)
            assert np.max(np.abs(coef[p, f] - ref)) <= cc.FORWARD_REL * np.max(np.abs(ref)), (p, f)


@pytest.mark.gpu
def test_failed_pivot_is_status_1_for_its_problem_only_and_auto_solves_it_again():
    A, b, w0, ccat, fs, folds = labelled(*cc.sweep_case("31")[:4])
    K = A.shape[1]
    # column 3 repeats column 2 except on the rows of (fold 1, category 0): without fold 1, or with category 0 weighted
    # out, the two columns are one
    A = A.copy()
    differ = ccat == 1 * C + 0
    A[~differ, 3] = A[~differ, 2]
    # scales within a decade: a category 0 weighted down by 1e-7 would leave the two columns one in double precision too
    S = 10.0 ** np.random.default_rng(8).uniform(-0.5, 0.5, (4, C))
    S[1, 0] = 0.0
    fails = np.zeros((4, F), dtype=bool)
    fails[:, 1] = True
    fails[1, :] = True
    pt, s = make_solver("SVD")
    cf = CandidateFits(s, A, b, w0=w0, fs_dict=fs)
    assert cf.ncat == C
    dev = cf.cross_validate(S, folds=folds, method="device")
    assert np.array_equal(dev.status != 0, fails), dev.status
    assert np.all(np.isnan(dev.coef[fails])) and np.all(np.isfinite(dev.coef[~fails]))
    assert np.all(dev.min_pivot[fails] <= cc.PIVOT_TOL) and np.all(dev.min_pivot[~fails] > cc.PIVOT_FLOOR)
    assert np.all(dev.route == "device")
    # NaN sums for the failed (p, f) only: through the C ABI, per composite category
    ctx = pt.hip()
    raw = ctx.cv_candidate_rows(cf._cv[0], dev.coef, C).reshape(4, F, C, 4)
    counts = np.bincount(ccat, minlength=F * C).reshape(F, C)
    for p in range(4):
        for f in range(F):
            with_rows = counts[f] > 0
            assert np.all(np.isnan(raw[p, f][with_rows]) == fails[p, f]), (p, f)
    assert np.isnan(dev.cost({"Energy": 1.0, "Force": 1.0})).all()          # every candidate has a failed fold here
    auto = cf.cross_validate(S, folds=folds, method="auto")
    comp = cf.cross_validate(S, folds=folds, method="composed")
    assert np.array_equal(auto.route == "composed", fails) and np.all(comp.route == "composed")
    assert np.array_equal(auto.coef[fails], comp.coef[fails]) and np.all(np.isfinite(auto.coef))
    assert np.array_equal(auto.coef[~fails], dev.coef[~fails])               # all other problems are unchanged
    assert np.array_equal(auto.min_pivot, dev.min_pivot, equal_nan=True)
    assert not auto.status.any() and np.isfinite(auto.cost({"Energy": 1.0, "Force": 1.0})).all()
    # the sums of the problems that did not fail do not move either
    raw_auto = ctx.cv_candidate_rows(cf._cv[0], auto.coef, C).reshape(4, F, C, 4)
    assert np.array_equal(raw_auto[~fails], raw[~fails]) and np.all(np.isfinite(raw_auto))
    pt.free()


# ---------------------------------------------------------------------------------------
# 4. CandidateFits.cross_validate on the Ta golden rows
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["SVD", "RIDGE"])
def test_ta_cross_validation_matches_the_refits_on_the_rows(ta, ta_fits, name):
    A, b, _ = ta
    fs = cc.ta_labels(ta_fits)
    alpha = cc.TA_ALPHAS[name]
    pt, s = make_solver(name, {"RIDGE": {"alpha": alpha}} if name == "RIDGE" else None)
    cf = CandidateFits(s, A, b, fs_dict=fs)
    ref, ref_sums, counts, S, keys, ccat, bl = cc.ta_oracle(name)
    _, _, _, fold_of_unit, _ = cc.ta_layout(fs)
    assert cf.keys == keys
    assert np.array_equal(S, cf.scales_from_group_weights(cc.ta_candidates(sorted(set(fs["Groups"])), cc.TA_P, seed=11)))
    Cn, K, Fn = cf.ncat, A.shape[1], cc.TA_F
    betas0 = cf.fit(S)
    sums0 = cf.error_sums(betas0, S)
    own = cf._layout
    cv = cf.cross_validate(S, folds=Fn, by="Configs")
    assert cv.fold_of_unit == fold_of_unit and cv.coef.shape == (cc.TA_P, Fn, K)
    assert not cv.status.any() and np.all(cv.route == "device")
    ka = cc.worst_backward(bl, S, Fn, Cn, K, alpha, cv.coef)
    kc = cc.worst_forward(cv.coef, ref)
    want = ccv.pool_heldout(ref_sums, counts, S, Fn)
    has = want[:, :, 0] > 0
    kb = float(np.max(np.abs(cv.sums - want)[:, :, 1:][has] / want[:, :, 1:][has]))
    print(f"Ta {name}: backward {ka:.2e} held-out {kb:.2e} forward {kc:.2e} min pivot {cv.min_pivot.min():.2e}")
    assert ka <= cc.BACKWARD_BAR_TA and kb <= cc.HELDOUT_REL_TA and kc <= cc.FORWARD_REL_TA, (ka, kb, kc)
    assert np.array_equal(cv.sums[:, :, 0], want[:, :, 0]) and np.all(cv.sums[~has] == 0.0)
    # tables against oracle R
    oracle = ccv.CandidateCV(ref, cv.status, cv.min_pivot, cv.route, fold_of_unit, want, keys, S)
    index, values = cv.tables(frames=False)
    index_r, values_r = oracle.tables(frames=False)
    assert index == index_r and np.array_equal(values[:, :, 0], values_r[:, :, 0])
    fin = np.isfinite(values_r)
    assert np.array_equal(fin, np.isfinite(values))
    assert np.all(np.abs(values - values_r)[fin] <= cc.HELDOUT_REL_TA * np.abs(values_r)[fin])
    frames = cv.tables()
    assert len(frames) == cc.TA_P and np.array_equal(frames[3].to_numpy(), values[3], equal_nan=True)
    assert ("*ALL", "Force") in frames[0].index
    # cost against the numpy formula
    weights = {"Energy": 1.0, "Force": 0.3, "Stress": 0.01}
    rmse = cv.row_type_errors[:, :, 1]
    formula = sum(weights[t] * rmse[:, i] for i, t in enumerate(cv.row_types))
    assert np.allclose(cv.cost(weights), formula, rtol=1e-15, atol=0)
    assert np.all(np.abs(cv.cost(weights) - oracle.cost(weights)) <= cc.HELDOUT_REL_TA * oracle.cost(weights))
    # device against composed, on the composite layout the first call left (same tag: nothing is prepared again)
    tag = cf._cv[0]
    comp = cf.cross_validate(S, folds=Fn, by="Configs", method="composed")
    assert cf._cv[0] == tag and np.all(comp.route == "composed") and not comp.status.any()
    a, c_ = cv.row_type_errors[:, :, 1], comp.row_type_errors[:, :, 1]
    assert np.all(np.abs(a - c_) <= cc.HELDOUT_REL_TA * c_), np.max(np.abs(a - c_) / c_)
    # afterwards fit and errors return exactly what they returned before: the own layout is prepared again
    assert np.array_equal(cf.fit(S), betas0)
    assert cf._layout != own and pt.hip().cat_info()["layout"] == cf._layout
    assert np.array_equal(cf.error_sums(betas0, S), sums0)
    pt.free()


# ---------------------------------------------------------------------------------------
# 5. K = 145: beyond the kernel
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_k145_takes_the_composed_route():
    A0, b0, w00, ccat0, K = cc.sweep_case("145")
    A, b, w0, ccat, fs, folds = labelled(A0, b0, w00, ccat0)
    S = cc.sweep_scales("145")[:3]
    pt, s = make_solver("SVD")
    cf = CandidateFits(s, A, b, w0=w0, fs_dict=fs)
    with pytest.raises(ValueError, match="144"):
        cf.cross_validate(S, folds=folds, method="device")
    cv = cf.cross_validate(S, folds=folds, method="auto")
    assert np.all(cv.route == "composed") and not cv.status.any()
    ref, ref_sums, bl = cc.oracle_r_from(A, b, w0, ccat, S, F, C, 0.0)
    counts = np.bincount(ccat, minlength=F * C)
    want = ccv.pool_heldout(ref_sums, counts, S, F)
    kc = cc.worst_forward(cv.coef, np.asarray(ref, dtype=np.float64))
    kb = float(np.max(np.abs(cv.sums - want)[:, :, 1:3] / want[:, :, 1:3]))
    print(f"K = 145 composed: held-out {kb:.2e} forward {kc:.2e}")
    assert kc <= cc.FORWARD_REL and kb <= cc.HELDOUT_REL, (kc, kb)
    pt.free()


# ---------------------------------------------------------------------------------------
# 6. two ranks, peer-to-peer transport, one GPU
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_ranks_p2p_match_one_rank(tmp_path, ta, ta_fits):
    world = 2
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="candidate cv two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "candidate_cv_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    r0, r1 = (dict(np.load(tmp_path / f"cv_rank{r}.npz")) for r in range(world))
    for key in ("coef", "status", "sums", "cost", "fold_units", "fold_ids"):
        assert np.array_equal(r0[key], r1[key]), key                       # every rank holds the pooled result
    assert int(r0["split_units"]) > 0                                       # units with rows on both ranks exist
    A, b, _ = ta
    fs = cc.ta_labels(ta_fits)
    pt, s = make_solver("SVD")
    cf = CandidateFits(s, A, b, fs_dict=fs)
    S = cc.ta_layout(fs)[4]
    cv = cf.cross_validate(S, folds=cc.TA_F, by="Configs")
    # a unit split over the ranks lands in one fold: the folds are those of the one-rank call
    assert dict(zip(r0["fold_units"].tolist(), r0["fold_ids"].tolist())) == cv.fold_of_unit
    assert not r0["status"].any()
    # two ranks sum their statistics in another order than one
    assert cc.worst_forward(r0["coef"], cv.coef) <= cc.FORWARD_REL_TA
    assert np.array_equal(r0["sums"][:, :, 0], cv.sums[:, :, 0])
    has = cv.sums[:, :, 0] > 0
    assert np.all(np.abs(r0["sums"] - cv.sums)[:, :, 1:][has] <= cc.HELDOUT_REL_TA * cv.sums[:, :, 1:][has])
    values = cv.tables(frames=False)[1]
    fin = np.isfinite(values)
    assert np.array_equal(fin, np.isfinite(r0["tables"]))
    assert np.all(np.abs(r0["tables"] - values)[fin] <= cc.HELDOUT_REL_TA * np.abs(values)[fin])
    cost = cv.cost({"Energy": 1.0, "Force": 0.3, "Stress": 0.01})
    assert np.all(np.abs(r0["cost"] - cost) <= cc.HELDOUT_REL_TA * cost)
    pt.free()

"""GPU: the gradient of the cross-validated cost over the group weights (``fsnap_cv_candidates_grad``, kernels G1 and G2 of
csrc/fsnap_cvgrad.hip; ``CandidateFits.cross_validate_gradient`` / ``descend_weights``) against the long-double oracle of
tests/candidate_cvgrad_cases.py at bars of 10 x what the numpy restatement differs from it by -- the geometry sweep through the
C ABI, batch invariance and determinism, the scale invariant, the Python routes, failed problems, the Ta golden rows, the host
route beyond 144 columns, the descent and two ranks over the peer-to-peer transport."""
import os
import subprocess
import sys

import numpy as np
import pytest

import candidate_cv_cases as cc
import candidate_cvgrad_cases as gc
from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import CandidateFits, solver_factory
from fitsnap_amd.solvers import candidates_cv_grad as cg

from conftest import ROOT

F, C = cc.SWEEP_F, cc.SWEEP_C
WEIGHTS = {"Energy": 1.0, "Force": 0.3}                    # the type weights of the sweep cases (gc.case)


def make_solver(name, extra=None):
    pt = ParallelTools()
    d = {"SOLVER": {"solver": name}}
    d.update(extra or {})
    return pt, solver_factory.solver(name, pt, Config(pt, d))


def prepared(ctx, A, b, w0, ccat, ncat):
    ctx.upload_rows(A, b)
    ctx.set_weights(w0, None)
    layout = ctx.cat_prepare(ccat, ncat)
    ctx.cat_normal_eq(layout)
    return layout


def labelled(A, b, w0, ccat):
    """The rows of a sweep case that have a category, with labels under which ``CandidateFits`` builds the same composite
    categories: category c = (group c // 2, energy | force), five units per fold, folds by mapping (the construction of
    tests/test_gpu_candidate_cv.py)."""
    keep = ccat >= 0
    A, b, w0, ccat = np.ascontiguousarray(A[keep]), b[keep], w0[keep], ccat[keep]
    fold, c = ccat // C, ccat % C
    fs = {"Groups": [f"g{int(x) // 2}" for x in c], "Testing": [False] * len(b),
          "Row_Type": ["Force" if int(x) % 2 else "Energy" for x in c], "Configs": [f"f{int(f)}u{i % 5}" for i, f in enumerate(fold)]}
    folds = {f"f{f}u{u}": f for f in range(F) for u in range(5)}
    return A, b, w0, ccat, fs, folds


def run(ctx, layout, alpha, S, omega, coef):
    """(g, lam, grad_S, gla, info) of one ``fsnap_cv_candidates_grad`` call."""
    grad, gla, lam, info = ctx.cv_candidates_grad(layout, alpha, S, omega, coef, want_lambda=True)
    g = ctx.cv_candidates_grad_rhs(*coef.shape)
    return g, lam, grad, gla, info


# ---------------------------------------------------------------------------------------
# 1. the sweep through the C ABI: g, lambda, dJ/dS, dJ/dlog alpha, the scale invariant, the 16-candidate tile edge
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", gc.CASES)
def test_sweep_matches_the_long_double_adjoint(name):
    A, b, w0, ccat, K, Fn, Cn, S, tof, wt = gc.case(name)
    ctx = _capi.HipContext(0)
    try:
        layout = prepared(ctx, A, b, w0, ccat, Fn * Cn)
        for ia in range(len(cc.ALPHA_FRACTIONS)):
            ref = gc.oracle(name, ia)
            alpha, omega = ref["alpha"], gc.f64(ref["omega"])
            coef, cinfo = ctx.cv_candidates(layout, alpha, S, Fn, K)
            assert not cinfo[:, :, 0].any()
            runs = {Pb: run(ctx, layout, alpha, S[:Pb], omega[:Pb], coef[:Pb]) for Pb in cc.BATCHES}
            g, lam, grad, gla, info = runs[gc.P]
            assert not info[:, :, 0].any(), (name, alpha, np.argwhere(info[:, :, 0] != 0))      # status 0 for ALL problems
            kg, kl, kd, ka, ki = gc.errors(ref, g, lam, grad, gla, S)
            print(f"{name} alpha {alpha:.2e}: g {kg:.2e} lambda {kl:.2e} grad {kd:.2e} alpha {ka:.2e} invariant {ki:.2e} "
                  f"min pivot {info[:, :, 1].min():.2e}")
            assert kg <= gc.G_BAR and kl <= gc.LAMBDA_BAR and kd <= gc.GRAD_BAR and ka <= gc.ALPHA_BAR, (name, alpha, kg, kl, kd, ka)
            assert ki <= gc.INVARIANT_BAR, (name, alpha, ki)
            # the adjoint solve meets the pivots of the refit: the same system
            assert np.array_equal(info[:, :, 1], cinfo[:, :, 1])
            if alpha == 0.0:
                assert np.all(gla == 0)
            # batches of 1 and 16 are the first candidates of the batch of 17, bit for bit
            for Pb in cc.BATCHES[:-1]:
                for got, want in zip(runs[Pb], runs[gc.P]):
                    assert np.array_equal(got, want[:Pb]), (name, alpha, Pb)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------
# 2. determinism and batch invariance
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["65", gc.OWN])
def test_bits_do_not_depend_on_the_run_or_the_batch(name):
    A, b, w0, ccat, K, Fn, Cn, S, tof, wt = gc.case(name)
    ref = gc.oracle(name, 1)
    alpha, omega = ref["alpha"], gc.f64(ref["omega"])
    ctx = _capi.HipContext(0)
    try:
        layout = prepared(ctx, A, b, w0, ccat, Fn * Cn)
        coef, _ = ctx.cv_candidates(layout, alpha, S, Fn, K)
        first, second = run(ctx, layout, alpha, S, omega, coef), run(ctx, layout, alpha, S, omega, coef)
        for x, y in zip(first, second):
            assert np.array_equal(x, y)
        perm = np.random.default_rng(3).permutation(gc.P)
        shuffled = run(ctx, layout, alpha, S[perm], omega[perm], coef[perm])
        for x, y in zip(first, shuffled):
            assert np.array_equal(x[perm], y)
        for p in (0, 9, 16):
            alone = run(ctx, layout, alpha, S[p:p + 1], omega[p:p + 1], coef[p:p + 1])
            for x, y in zip(first, alone):
                assert np.array_equal(x[p:p + 1], y), p
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------
# 3. CandidateFits.cross_validate_gradient: device against host, the CandidateCV of the call, fit() / errors() afterwards
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_route_matches_the_host_route_and_leaves_everything_else_alone():
    name = "65"
    A, b, w0, ccat, fs, folds = labelled(*cc.sweep_case(name)[:4])
    S = cc.sweep_scales(name)
    ref = gc.oracle(name, 0)
    scale = gc.f64(ref["scale"])
    pt, s = make_solver("SVD")
    cf = CandidateFits(s, A, b, w0=w0, fs_dict=fs)
    assert cf.ncat == C
    betas0 = cf.fit(S)
    sums0 = cf.error_sums(betas0, S)
    for metric in cg.METRICS:
        dev = cf.cross_validate_gradient(S, WEIGHTS, metric=metric, folds=folds, method="device")
        host = cf.cross_validate_gradient(S, WEIGHTS, metric=metric, folds=folds, method="host")
        auto = cf.cross_validate_gradient(S, WEIGHTS, metric=metric, folds=folds)
        assert dev.method == "device" and host.method == "host" and auto.method == "device"
        assert not dev.status.any() and not host.status.any()
        assert np.array_equal(dev.cost, host.cost) and np.array_equal(dev.omega, host.omega)
        assert np.array_equal(auto.grad_S, dev.grad_S) and np.array_equal(auto.cost, dev.cost)
        assert np.array_equal(dev.grad_log, S * dev.grad_S) and np.all(dev.grad_log_alpha == 0)
        kd = gc.scaled_error(dev.grad_S, host.grad_S, scale)
        print(f"{metric}: device against host {kd:.2e} of the scale")
        assert kd <= gc.GRAD_BAR
        if metric == "rmse":
            # both routes against oracle R (its omega comes from its own held-out sums: HELDOUT_REL / 2 of relative error more)
            for r in (dev, host):
                assert gc.scaled_error(r.grad_S, ref["grad"], scale) <= gc.GRAD_BAR + cc.HELDOUT_REL
            assert np.all(np.abs(dev.cost - gc.f64(ref["J"])) <= cc.HELDOUT_REL * gc.f64(ref["J"]))
        # result.cv is cross_validate on the same S, bit for bit
        cv = cf.cross_validate(S, folds=folds, method="device")
        for key in ("coef", "status", "min_pivot", "sums", "base_sums"):
            assert np.array_equal(getattr(dev.cv, key), getattr(cv, key)), key
        assert np.array_equal(dev.cost, cg.objective(cv.base_sums, cf.keys, WEIGHTS, metric)[0])
    # a later fit() / errors() returns the bits it returned before
    assert np.array_equal(cf.fit(S), betas0) and np.array_equal(cf.error_sums(betas0, S), sums0)
    pt.free()


# ---------------------------------------------------------------------------------------
# 4. failed problems: NaN rows for exactly their candidates
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_failed_problem_gives_a_nan_row_for_its_candidate_only():
    A, b, w0, ccat, fs, folds = labelled(*cc.sweep_case("31")[:4])
    # the duplicated-column case of tests/test_gpu_candidate_cv.py, with the rows that tell the columns apart spread over all
    # folds so that some candidates are healthy: column 3 repeats column 2 except on the rows of category 0; a candidate that
    # weights category 0 out has two equal columns in every fold
    A = A.copy()
    differ = ccat % C == 0
    A[~differ, 3] = A[~differ, 2]
    S = 10.0 ** np.random.default_rng(8).uniform(-0.5, 0.5, (4, C))
    S[1, 0] = 0.0
    pt, s = make_solver("SVD")
    cf = CandidateFits(s, A, b, w0=w0, fs_dict=fs)
    others = [0, 2, 3]
    for method in ("device", "host"):
        r = cf.cross_validate_gradient(S, WEIGHTS, folds=folds, method=method)
        assert np.array_equal(r.status.any(axis=1), [False, True, False, False]), r.status
        assert np.isnan(r.grad_S[1]).all() and np.isnan(r.grad_log[1]).all() and np.isnan(r.cost[1]) and np.isnan(r.grad_log_alpha[1])
        assert np.isfinite(r.grad_S[others]).all() and np.isfinite(r.cost[others]).all()
        without = cf.cross_validate_gradient(S[others], WEIGHTS, folds=folds, method=method)
        assert not without.status.any()
        assert np.array_equal(r.grad_S[others], without.grad_S) and np.array_equal(r.cost[others], without.cost)
        assert np.array_equal(r.grad_log_alpha[others], without.grad_log_alpha)
    pt.free()


# ---------------------------------------------------------------------------------------
# 5. the Ta golden rows
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["SVD", "RIDGE"])
def test_ta_gradient_matches_the_long_double_adjoint(ta, ta_fits, name):
    A, b, _ = ta
    fs = cc.ta_labels(ta_fits)
    alpha = cc.TA_ALPHAS[name]
    ref = gc.ta_oracle(name)
    S, scale = ref["S"], gc.f64(ref["scale"])
    pt, s = make_solver(name, {"RIDGE": {"alpha": alpha}} if name == "RIDGE" else None)
    cf = CandidateFits(s, A, b, fs_dict=fs)
    assert cf.keys == ref["keys"]
    r = cf.cross_validate_gradient(S, gc.TA_WEIGHTS, folds=cc.TA_F, by="Configs")
    assert r.method == "device" and not r.status.any()
    # through the C ABI with the oracle's omega, as the constants were measured
    ctx = pt.hip()
    g, lam, grad, gla, info = run(ctx, cf._cv[0], alpha, S, gc.f64(ref["omega"]), r.cv.coef)
    kg, kl, kd, ka, ki = gc.errors(ref, g, lam, grad, gla, S)
    print(f"Ta {name}: g {kg:.2e} lambda {kl:.2e} grad {kd:.2e} alpha {ka:.2e} invariant {ki:.2e}")
    assert kg <= gc.G_BAR_TA and kl <= gc.LAMBDA_BAR_TA and kd <= gc.GRAD_BAR_TA and ka <= gc.ALPHA_BAR_TA, (kg, kl, kd, ka)
    assert ki <= gc.INVARIANT_BAR_TA
    # the method's own omega comes from its held-out sums: at most HELDOUT_REL_TA / 2 of relative error more, of terms whose
    # absolute sum is the scale
    J = gc.f64(ref["J"])
    assert np.all(np.abs(r.cost - J) <= cc.HELDOUT_REL_TA * J)
    assert gc.scaled_error(r.grad_S, ref["grad"], scale) <= gc.GRAD_BAR_TA + cc.HELDOUT_REL_TA
    testing = np.array([k[1] for k in cf.keys])
    assert np.all(r.omega[:, testing] == 0) and np.all(r.omega[:, ~testing] > 0)
    if alpha == 0.0:
        assert np.all(r.grad_log_alpha == 0)
    else:
        assert gc.scaled_error(r.grad_log_alpha, ref["gla"], ref["sa"]) <= gc.ALPHA_BAR_TA + cc.HELDOUT_REL_TA
    # with w0 = 1 the objective is CandidateCV.cost exactly
    assert np.array_equal(r.cost, r.cv.cost(gc.TA_WEIGHTS, "rmse"))
    pt.free()


# ---------------------------------------------------------------------------------------
# 6. K = 145: beyond the kernels
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_k145_takes_the_host_route():
    A0, b0, w00, ccat0, K = cc.sweep_case("145")
    A, b, w0, ccat, fs, folds = labelled(A0, b0, w00, ccat0)
    S = cc.sweep_scales("145")[:3]
    pt, s = make_solver("SVD")
    cf = CandidateFits(s, A, b, w0=w0, fs_dict=fs)
    with pytest.raises(ValueError, match="144"):
        cf.cross_validate_gradient(S, WEIGHTS, folds=folds, method="device")
    r = cf.cross_validate_gradient(S, WEIGHTS, folds=folds, method="auto")
    assert r.method == "host" and not r.status.any() and np.all(r.cv.route == "composed")
    ref = gc.oracle_from(A, b, w0, ccat, S, F, C, 0.0, np.arange(C) % 2, np.array([1.0, 0.3]), "rmse")
    kd = gc.scaled_error(r.grad_S, ref["grad"], ref["scale"])
    print(f"K = 145 host route: grad {kd:.2e}")
    assert kd <= gc.GRAD_BAR + cc.HELDOUT_REL
    pt.free()


# ---------------------------------------------------------------------------------------
# 7. the descent
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_descent_lowers_the_held_out_cost():
    A, b, w0, ccat, fs, folds = labelled(*cc.sweep_case("31")[:4])
    S0 = cc.sweep_scales("31")[:6]
    pt, s = make_solver("SVD")
    cf = CandidateFits(s, A, b, w0=w0, fs_dict=fs)
    S, hist, taken = cf.descend_weights(S0, WEIGHTS, steps=5, folds=folds)
    print("cost history:\n", hist)
    assert hist.shape == (6, 6) and taken.shape == (5, 6) and np.isfinite(hist).all()
    assert np.all(np.diff(hist, axis=0) <= 0)
    assert np.any(hist[-1] < hist[0])
    assert np.array_equal(np.sign(S), np.sign(S0))
    # the history ends at the cost of the returned scales, and the call is deterministic
    final = cf.cross_validate_gradient(S, WEIGHTS, folds=folds)
    assert np.array_equal(final.cost, hist[-1])
    again = cf.descend_weights(S0, WEIGHTS, steps=5, folds=folds)
    assert np.array_equal(again[0], S) and np.array_equal(again[1], hist) and np.array_equal(again[2], taken)
    pt.free()


# ---------------------------------------------------------------------------------------
# 8. two ranks, peer-to-peer transport, one GPU
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_ranks_p2p_match_one_rank(tmp_path, ta, ta_fits):
    """Both ranks return the same bits.  Against one process holding the rows in rank order they agree to rounding, not to the
    bit (measured on an MI355X: grad_S 2.2e-12 of the scale; cost, omega, coefficients and gradient all differ in the last
    digits): the per-(fold, category) blocks themselves differ, because two ranks add their chunk statistics as two partial sums
    and one addition where one process adds the chunks in sequence -- what tests/test_gpu_candidate_cv.py records for
    ``cross_validate``.  Given equal blocks the gradient kernels are bit-reproducible (the determinism test above)."""
    world = 2
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="candidate cv gradient two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "candidate_cvgrad_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    r0, r1 = (dict(np.load(tmp_path / f"cvgrad_rank{r}.npz")) for r in range(world))
    keys = ("cost", "grad_S", "grad_log", "grad_log_alpha", "omega", "status", "coef", "descent_S", "descent_history")
    for key in keys:
        assert np.array_equal(r0[key], r1[key]), key                       # every rank returns the same bits
    assert not r0["status"].any()
    # one process holding the rows in rank order
    A, b, _ = ta
    fs_all = cc.ta_labels(ta_fits)
    order = np.concatenate([np.flatnonzero((np.arange(len(b)) // 43 % world) == r) for r in range(world)])
    fs = {k: [v[i] for i in order] for k, v in fs_all.items()}
    pt, s = make_solver("RIDGE", {"RIDGE": {"alpha": cc.TA_ALPHAS["RIDGE"]}})
    cf = CandidateFits(s, np.ascontiguousarray(A[order]), np.ascontiguousarray(b[order]), fs_dict=fs)
    S = cc.ta_layout(fs_all)[4]
    one = cf.cross_validate_gradient(S, gc.TA_WEIGHTS, folds=cc.TA_F, by="Configs")
    same = {key: bool(np.array_equal(r0[key], getattr(one, key) if key != "coef" else one.cv.coef)) for key in keys[:7]}
    ref = gc.ta_oracle("RIDGE")
    scale = gc.f64(ref["scale"])
    kd = gc.scaled_error(r0["grad_S"], one.grad_S, scale)
    print(f"two ranks against one process: identical bits {same}; grad {kd:.2e} of the scale")
    # the ranks add their per-chunk statistics in another order than one process does (two partial sums, then one addition),
    # so the blocks -- and everything after them -- agree to rounding, not to the bit: the Ta bars, as for cross_validate
    assert kd <= gc.GRAD_BAR_TA + cc.HELDOUT_REL_TA
    assert np.all(np.abs(r0["cost"] - one.cost) <= cc.HELDOUT_REL_TA * one.cost)
    assert gc.scaled_error(r0["grad_S"], ref["grad"], scale) <= gc.GRAD_BAR_TA + cc.HELDOUT_REL_TA
    pt.free()

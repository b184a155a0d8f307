"""CPU: the gradient of the cross-validated cost over the group weights (solvers/candidates_cv_grad.py) -- the adjoint formulas
against central differences of the long-double objective, the scale invariant, the numpy restatement against the long-double
oracle at the recorded measurements, omega and J on hand-made sums, the descent against a stub evaluator, the C symbol and the
argument errors.  Nothing here touches a GPU."""
import os
import re

import numpy as np
import pytest

import candidate_cv_cases as cc
import candidate_cvgrad_cases as gc
from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import CandidateFits, solver_factory
from fitsnap_amd.solvers import candidates_cv as ccv
from fitsnap_amd.solvers import candidates_cv_grad as cg

LD = np.longdouble
ROOT = cc.ROOT
FD_H = LD(1e-5)
FD_BAR = 1e-6            # of the largest component: a wrong formula is off by O(1); float64 measured 8e-11 at h = 1e-5
FD_P = 3


# ---------------------------------------------------------------------------------------
# 1. oracle R against central differences of the long-double objective
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", cg.METRICS)
@pytest.mark.parametrize("name", ["1", "7", "31"])
def test_adjoint_formulas_match_central_differences(name, metric):
    A, b, w0, ccat, K, F, C, S, tof, wt = gc.case(name)
    # scales within a decade and a ridge term that matters, so that every component of the gradient is exercised
    S = 10.0 ** np.random.default_rng(5).uniform(-0.5, 0.5, (FD_P, C))
    alpha = cc.base_alpha(cc.blocks_numpy(A, b, w0, ccat, F * C), K, 1e-2)
    ref = gc.oracle_from(A, b, w0, ccat, S, F, C, alpha, tof, wt, metric)
    glog = np.asarray(S, dtype=LD) * ref["grad"]

    def J(Sx, ax):
        return gc.cost_ld(A, b, w0, ccat, Sx, F, C, ax, tof, wt, metric)

    fd = np.zeros((FD_P, C), dtype=LD)
    for c in range(C):
        up, dn = np.asarray(S, dtype=LD).copy(), np.asarray(S, dtype=LD).copy()
        up[:, c] *= np.exp(FD_H)
        dn[:, c] *= np.exp(-FD_H)
        fd[:, c] = (J(up, LD(alpha)) - J(dn, LD(alpha))) / (2 * FD_H)
    fda = (J(np.asarray(S, dtype=LD), LD(alpha) * np.exp(FD_H)) - J(np.asarray(S, dtype=LD), LD(alpha) * np.exp(-FD_H))) / (2 * FD_H)
    for p in range(FD_P):
        big = max(float(np.max(np.abs(glog[p]))), float(abs(ref["gla"][p])))
        dev = max(float(np.max(np.abs(fd[p] - glog[p]))), float(abs(fda[p] - ref["gla"][p]))) / big
        print(f"K = {K} {metric} candidate {p}: deviation {dev:.2e} of the largest component {big:.2e}; "
              f"dJ/dlog alpha {float(ref['gla'][p]):.2e}")
        assert dev <= FD_BAR, (name, metric, p, dev)
        assert float(abs(ref["gla"][p])) > 1e-3 * big          # the alpha derivative takes part in the comparison


# ---------------------------------------------------------------------------------------
# 2. the scale invariant, and oracle H against oracle R at the committed bars
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["7", "31", "65", gc.OWN])
def test_host_restatement_matches_the_oracle_and_keeps_the_scale_invariant(name):
    A, b, w0, ccat, K, F, C, S, tof, wt = gc.case(name)
    blocks = cc.blocks_numpy(A, b, w0, ccat, F * C)
    for ia in range(len(cc.ALPHA_FRACTIONS)):                  # alpha = 0 and alpha > 0
        ref = gc.oracle(name, ia)
        g, lam, grad, gla = gc.host_result(blocks, S, gc.f64(ref["omega"]), F, C, K, ref["alpha"])
        kg, kl, kd, ka, ki = gc.errors(ref, g, lam, grad, gla, S)
        print(f"{name} alpha {ref['alpha']:.2e}: g {kg:.2e} lambda {kl:.2e} grad {kd:.2e} alpha {ka:.2e} invariant {ki:.2e}")
        # oracle H is what the constants were measured on: it stays within them (to the last digit printed)
        assert kg <= 1.05 * gc.MEASURED_G and kl <= 1.05 * gc.MEASURED_LAMBDA and kd <= 1.05 * gc.MEASURED_GRAD
        assert ka <= 1.05 * gc.MEASURED_ALPHA
        assert ki <= gc.INVARIANT_BAR
        if ia == 0:
            assert np.all(gla == 0)                            # alpha = 0: the log-gradient of a candidate sums to zero
        # the oracle itself keeps the invariant far below the bar
        assert gc.invariant_error(ref, gc.f64(ref["grad"]), gc.f64(ref["gla"]), S) <= gc.MEASURED_INVARIANT
        if name == gc.OWN:
            assert np.all(gc.f64(ref["omega"])[:, tof == 2] == 0) and np.all(gc.f64(ref["omega"])[:, tof != 2] > 0)


# ---------------------------------------------------------------------------------------
# 3. omega and J from CandidateCV-shaped sums
# ---------------------------------------------------------------------------------------
def _hand_made():
    keys = [("a", False, "Energy"), ("a", False, "Force"), ("a", True, "Energy"), ("b", False, "Energy"), ("b", False, "Force"),
            ("b", False, "Stress"), ("c", False, "Virial")]
    rng = np.random.default_rng(2)
    P, C = 3, len(keys)
    base = np.zeros((P, C, 5))
    base[:, :, 0] = [4, 10, 3, 6, 20, 5, 0]                   # the Virial category holds no row: n_t = 0
    base[:, :, 1:] = rng.uniform(1.0, 2.0, (P, C, 4)) * base[:, :, :1]
    base[:, 6, 1:] = 0.0
    return keys, base


def test_omega_is_zero_for_testing_categories_weightless_types_and_empty_types():
    keys, base = _hand_made()
    weights = {"Energy": 1.0, "Force": 0.3, "Stress": 0.0, "Virial": 2.0}
    for metric in cg.METRICS:
        J, omega, row_types = cg.objective(base, keys, {k: v for k, v in weights.items() if k != "Virial"}, metric)
        assert row_types == ["Energy", "Force", "Stress", "Virial"] and np.isfinite(J).all()
        assert np.all(omega[:, 2] == 0)                        # testing
        assert np.all(omega[:, 5] == 0)                        # weight 0
        assert np.all(omega[:, 6] == 0)                        # missing from the mapping: weight 0
        assert np.all(omega[:, [0, 3]] > 0) and np.array_equal(omega[:, 0], omega[:, 3])   # one coefficient per row type
        E = base[:, 0, 4] + base[:, 3, 4]
        want = 1.0 / (2 * np.sqrt(E / 10) * 10) if metric == "rmse" else np.full(3, 1.0 / 10)
        assert np.allclose(omega[:, 0], want, rtol=1e-15, atol=0)
        Ef = base[:, 1, 4] + base[:, 4, 4]
        wantJ = np.sqrt(E / 10) + 0.3 * np.sqrt(Ef / 30) if metric == "rmse" else E / 10 + 0.3 * Ef / 30
        assert np.allclose(J, wantJ, rtol=1e-15, atol=0)
        # a type without a row: n_t = 0 gives omega 0 (and, as in CandidateCV.cost, a NaN cost)
        J2, omega2, _ = cg.objective(base, keys, weights, metric)
        assert np.all(omega2[:, 6] == 0) and np.isnan(J2).all() and np.array_equal(omega2[:, :6], omega[:, :6])


def test_cost_is_the_cost_of_candidate_cv_when_the_base_weight_is_one():
    keys, base = _hand_made()
    base[:, :, 3] = base[:, :, 1]                              # w0 = 1: the weighted sums are the plain ones
    base[:, :, 4] = base[:, :, 2]
    S = np.random.default_rng(3).uniform(0.1, 3.0, base.shape[:2])
    pooled = base.copy()
    pooled[:, :, 3] *= np.abs(S)
    pooled[:, :, 4] *= S * S
    cv = ccv.CandidateCV(np.zeros((3, 2, 1)), np.zeros((3, 2), dtype=int), np.ones((3, 2)), None, {}, pooled, keys, S, base)
    weights = {"Energy": 1.0, "Force": 0.3, "Stress": 0.01}
    assert np.array_equal(cg.objective(cv.base_sums, keys, weights, "rmse")[0], cv.cost(weights, "rmse"))
    assert np.array_equal(cg.objective(cv.base_sums, keys, [1.0, 0.3, 0.01, 0.0], "rmse")[0], cv.cost(weights, "rmse"))


# ---------------------------------------------------------------------------------------
# 4. the descent against a stub evaluator
# ---------------------------------------------------------------------------------------
class Quadratic:
    """J[p] = sum_c a_c (log|S[p, c]| - t_c)^2 over the entries with S != 0; candidate ``nan_at`` is NaN throughout."""

    def __init__(self, a, t, nan_at=None):
        self.a, self.t, self.nan_at = np.asarray(a, dtype=float), np.asarray(t, dtype=float), nan_at
        self.evaluations, self.trials = [], []

    def _cost(self, S):
        with np.errstate(divide="ignore"):
            th = np.where(S != 0, np.log(np.abs(S)), 0.0)
        d = np.where(S != 0, th - self.t, 0.0)
        J = (self.a * d * d).sum(axis=1)
        if self.nan_at is not None:
            J[self.nan_at] = np.nan
        return J, 2 * self.a * d

    def evaluate(self, S):
        self.evaluations.append(S.copy())
        J, g = self._cost(S)
        if self.nan_at is not None:
            g[self.nan_at] = np.nan
        return J, g

    def trial_cost(self, S):
        self.trials.append(S.copy())
        return self._cost(S)[0]


def test_descent_halves_doubles_and_never_increases_the_cost():
    q = Quadratic([1.0, 4.0, 0.5], [0.3, -0.2, 1.0])
    S0 = np.array([[1.0, 2.0, 0.5], [3.0, 0.0, -1.5], [0.2, 0.1, 4.0]])
    S, hist, taken = cg.armijo_descent(q.evaluate, q.trial_cost, S0, steps=6, eta0=0.5, c1=1e-4, max_halvings=8)
    assert hist.shape == (7, 3) and taken.shape == (6, 3) and len(q.evaluations) == 6
    assert np.all(np.diff(hist, axis=0) <= 0) and np.all(hist[-1] < hist[0])
    assert S[1, 1] == 0.0 and np.all(np.array(q.trials)[:, 1, 1] == 0.0)       # S = 0 stays 0
    assert S[1, 2] < 0                                                          # signs are kept
    assert np.array_equal(hist[-1], q._cost(S)[0])                              # the history ends at the returned point
    # the curvature 2 a = 8 of coordinate 1 makes eta = 0.5 overshoot (|1 - 8 eta| > 1): the first accepted step is a halved one
    assert taken[0, 0] == 0.25 and taken[0, 2] == 0.25
    # an accepted step doubles eta; a refused trial halves it: every accepted eta is a power of two times eta0, and the step
    # after an accepted one starts from twice its size
    for p in range(3):
        for it in range(5):
            if taken[it, p] > 0 and taken[it + 1, p] > 0:
                ratio = taken[it + 1, p] / taken[it, p]
                assert ratio in (2.0, 1.0, 0.5, 0.25, 0.125), (p, it, ratio)
    # one gradient call per iteration; every line-search round is ONE trial call over all P points
    assert all(t.shape == S0.shape for t in q.trials) and len(q.trials) >= 6


def test_descent_with_a_hopeless_start_gives_up_after_max_halvings_and_leaves_it():
    # candidate 0 sits in a cost that any step increases (a stub that reports a wrong, ascending gradient)
    q = Quadratic([1.0], [0.0])

    def wrong(S):
        J, g = q.evaluate(S)
        return J, -g

    S0 = np.array([[2.0]])
    S, hist, taken = cg.armijo_descent(wrong, q.trial_cost, S0, steps=2, eta0=0.5, max_halvings=3)
    assert np.array_equal(S, S0) and np.all(taken == 0) and np.all(hist == hist[0])
    assert len(q.trials) == 2 * 4                                               # max_halvings + 1 rounds per iteration
    etas = [np.log(t[0, 0] / 2.0) for t in q.trials]                            # theta moved by eta * 2 log 2
    assert np.allclose(np.array(etas[:4]) / etas[0], [1, 0.5, 0.25, 0.125], rtol=1e-12)
    assert np.isclose(etas[4] / etas[0], 0.0625, rtol=1e-12)                    # the halved eta is kept for the next iteration


def test_descent_leaves_a_nan_candidate_alone_without_disturbing_the_others():
    a, t = [1.0, 4.0, 0.5], [0.3, -0.2, 1.0]
    S0 = np.array([[1.0, 2.0, 0.5], [3.0, 0.7, 1.5], [0.2, 0.1, 4.0]])
    clean = Quadratic(a, t)
    S_ref, hist_ref, taken_ref = cg.armijo_descent(clean.evaluate, clean.trial_cost, S0, steps=4)
    q = Quadratic(a, t, nan_at=1)
    S, hist, taken = cg.armijo_descent(q.evaluate, q.trial_cost, S0, steps=4)
    assert np.array_equal(S[1], S0[1]) and np.isnan(hist[:, 1]).all() and np.all(taken[:, 1] == 0)
    for p in (0, 2):
        assert np.array_equal(S[p], S_ref[p]) and np.array_equal(hist[:, p], hist_ref[:, p])
        assert np.array_equal(taken[:, p], taken_ref[:, p])
    assert all(np.array_equal(tr[1], S0[1]) for tr in q.trials)


def test_zero_steps_returns_the_cost_of_the_start():
    q = Quadratic([1.0], [0.0])
    S, hist, taken = cg.armijo_descent(q.evaluate, q.trial_cost, np.array([[2.0]]), steps=0)
    assert hist.shape == (1, 1) and taken.shape == (0, 1) and hist[0, 0] == np.log(2.0) ** 2 and not q.evaluations


# ---------------------------------------------------------------------------------------
# 5. the C symbol and the argument errors
# ---------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fsnap_hip.h")).read()
    proto = re.search(r"int fsnap_cv_candidates_grad\(([^;]*)\);", header)
    assert proto and proto.group(1).count(",") + 1 == len(_capi.SIGNATURES["fsnap_cv_candidates_grad"][1]) == 14
    lib = _capi.load_library()
    assert hasattr(lib, "fsnap_cv_candidates_grad") and callable(getattr(_capi.HipContext, "cv_candidates_grad"))
    assert '"fsnap_cvgrad.hip"' in open(os.path.join(ROOT, "fitsnap_amd", "build.py")).read()
    # a NULL context is refused before anything touches a GPU
    assert lib.fsnap_cv_candidates_grad(None, 1, 0.0, None, None, None, 1, 2, 1, 1, None, None, None, None) == _capi.E_ARG


def test_argument_errors():
    assert cg.choose_method("auto", 144) == "device" and cg.choose_method("auto", 145) == "host"
    assert cg.choose_method("host", 10) == "host" and cg.choose_method("device", 144) == "device"
    with pytest.raises(ValueError, match="144"):
        cg.choose_method("device", 145)
    with pytest.raises(ValueError, match="method"):
        cg.choose_method("composed", 10)
    keys, base = _hand_made()
    with pytest.raises(ValueError, match="metric"):
        cg.objective(base, keys, {"Energy": 1.0}, "mae")
    with pytest.raises(ValueError, match="Pressure"):
        cg.objective(base, keys, {"Pressure": 1.0})
    with pytest.raises(ValueError):
        cg.objective(base, keys, [1.0, 2.0])
    with pytest.raises(ValueError):
        cg.armijo_descent(None, None, np.ones((2, 2)), steps=-1)
    with pytest.raises(ValueError):
        cg.armijo_descent(None, None, np.ones((2, 2)), eta0=0.0)
    with pytest.raises(ValueError):
        cg.armijo_descent(None, None, np.ones(2))


def test_the_methods_refuse_before_touching_the_gpu():
    rng = np.random.default_rng(0)
    m, K = 24, 3
    fs = {"Groups": ["g"] * m, "Testing": [False] * m, "Row_Type": ["Energy", "Force"] * (m // 2)}
    pt = ParallelTools()
    s = solver_factory.solver("SVD", pt, Config(pt, {"SOLVER": {"solver": "SVD"}}))
    cf = CandidateFits(s, rng.standard_normal((m, K)), rng.standard_normal(m), fs_dict=fs)
    S = np.ones((2, cf.ncat))
    weights = {"Energy": 1.0, "Force": 0.3}
    with pytest.raises(ValueError, match="metric"):
        cf.cross_validate_gradient(S, weights, metric="mae")
    with pytest.raises(ValueError, match="method"):
        cf.cross_validate_gradient(S, weights, method="composed")
    with pytest.raises(ValueError, match="Stress"):
        cf.cross_validate_gradient(S, {"Stress": 1.0})
    with pytest.raises(ValueError):
        cf.cross_validate_gradient(np.ones((2, cf.ncat + 1)), weights)
    with pytest.raises(KeyError):
        cf.cross_validate_gradient(S, weights)                     # no Configs labels
    with pytest.raises(ValueError):
        cf.descend_weights(np.ones((2, cf.ncat + 1)), weights)
    assert cf._cv is None and cf._layout is None
